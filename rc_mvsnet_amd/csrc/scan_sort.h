// The mesh kernels' shared building blocks, defined once in scan_sort.hip: the three-level exclusive scan of one array, the kernel
// that zeroes a few uint64 totals, the check of a scan work area, and one 8-bit pass of the stable LSD radix sort.
#pragma once
#include "common.h"

namespace rcmvs {

constexpr int SS_BLOCK = 256;                                     // every kernel here runs workgroups of this size
constexpr int SS_TILE = 2048;                                     // elements per workgroup of the scan, per level
constexpr int SS_TOP = 1024;                                      // ceil(2^31 / 2048 / 2048) = 512 sums at the top level
constexpr int SS_WORK = 2 * SS_TOP;                               // a work area: SS_TOP uint64, then ceil(n / SS_TILE) + 1 ints

// out[0 .. n] = the exclusive prefix sums of in[0 .. n), *total = the sum (total null: kept in the work area's last top slot,
// which no scan of at most 2^31 elements reaches); e0 / e1 as in RCMVS_LAUNCH_TIMED (either may be null).
// T: unsigned char or int, no element negative, every sum below 2^32.
template <class T>
void scan3(const T* in, long long n, int* out, int* work, unsigned long long* total, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// 0 when scan_work can be a work area, else the refusal in what's name
int scan_work_check(const char* what, const int* scan_work);

// p[0 .. n) = 0, n <= SS_BLOCK: one workgroup
__global__ __launch_bounds__(SS_BLOCK) void zero_u64_kernel(unsigned long long* __restrict__ p, int n);

// One pass of the sort of (key, index) pairs on bits shift .. shift + 7 (K: unsigned long long or unsigned), blocks of SS_BLOCK keys:
// hist[d * nblk + b] = the keys of block b whose digit is d; after an exclusive scan of hist into start, the scatter is stable.
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_hist_kernel(const K* __restrict__ key, long long n, int shift, long long nblk, int* __restrict__ hist);
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_scatter_kernel(const K* __restrict__ key_in, const int* __restrict__ idx_in, long long n,
                                                                 int shift, long long nblk, const int* __restrict__ start,
                                                                 K* __restrict__ key_out, int* __restrict__ idx_out);

extern template void scan3<unsigned char>(const unsigned char*, long long, int*, int*, unsigned long long*, hipStream_t, hipEvent_t, hipEvent_t);
extern template void scan3<int>(const int*, long long, int*, int*, unsigned long long*, hipStream_t, hipEvent_t, hipEvent_t);
extern template __global__ void radix_hist_kernel<unsigned long long>(const unsigned long long* __restrict__, long long, int, long long, int* __restrict__);
extern template __global__ void radix_hist_kernel<unsigned>(const unsigned* __restrict__, long long, int, long long, int* __restrict__);
extern template __global__ void radix_scatter_kernel<unsigned long long>(const unsigned long long* __restrict__, const int* __restrict__, long long, int,
                                                                         long long, const int* __restrict__, unsigned long long* __restrict__,
                                                                         int* __restrict__);
extern template __global__ void radix_scatter_kernel<unsigned>(const unsigned* __restrict__, const int* __restrict__, long long, int, long long,
                                                               const int* __restrict__, unsigned* __restrict__, int* __restrict__);

}  // namespace rcmvs
