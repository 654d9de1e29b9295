// pointcloud.hip's multi-block exclusive scan, which pc_register.hip calls too.
#pragma once
#include "common.h"

namespace rcmvs {

// in[0 .. n) -> out[0 .. n), out[n] = the total; bsum: ceil(n / RCMVS_PC_SCAN_TILE) + 1 ints of work
void pc_scan(const int* in, int n, int* bsum, int* out, hipStream_t st);

}  // namespace rcmvs
