// What the mesh kernels share (callers: mesh_clean.hip, mesh_decimate.hip, mesh_holes.hip, mesh_normals.hip, mesh_render.hip,
// mesh_texture.hip, and pc_register.hip for the radix pass).  Inline here: the flat thread id, the grid sizes and the overlap
// checks of the 256-thread families.  Defined once in scan_sort.hip:
//   scan3            the three-level exclusive scan of one array
//   scan_work_check  the check of a scan work area
//   zero_kernel      p[0 .. n) = 0
//   radix_hist_kernel, radix_scatter_kernel   one 8-bit pass of the stable LSD radix sort of (key, index) pairs
//   radix_passes, radix_sort                  the passes a largest key needs, and the loop over them
//   segments_kernel  where each key's run starts and ends in the sorted keys
#pragma once
#include <cstdint>

#include "common.h"

namespace rcmvs {

constexpr int SS_BLOCK = 256;                                     // every kernel here runs workgroups of this size
constexpr int SS_TILE = 2048;                                     // elements per workgroup of the scan, per level
constexpr int SS_TOP = 1024;                                      // ceil(2^31 / 2048 / 2048) = 512 sums at the top level
constexpr int SS_WORK = 2 * SS_TOP;                               // a work area: SS_TOP uint64, then ceil(n / SS_TILE) + 1 ints

// ---- one thread per element, workgroups of SS_BLOCK -----------------------------------------------------------------------------
__device__ inline long long gid() { return (long long)blockIdx.x * SS_BLOCK + threadIdx.x; }
inline unsigned blocks(long long n) { return (unsigned)(n > 0 ? cdiv(n, SS_BLOCK) : 1); }
inline unsigned capped_blocks(long long n) { return blocks(n) < 65536u ? blocks(n) : 65536u; }      // for kernels that stride by the grid

// ---- argument checks --------------------------------------------------------------------------------------------------------------
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// every output and work buffer, ptr[0 .. outputs), against everything after it in ptr[0 .. all): 0, else the refusal in what's name
inline int buffers_overlap(const char* what, const void* const* ptr, const size_t* len, int outputs, int all) {
    for (int i = 0; i < outputs; ++i)
        for (int j = i + 1; j < all; ++j) RCMVS_REQUIRE(!ranges_overlap(ptr[i], len[i], ptr[j], len[j]), "%s: an output or work buffer overlaps another buffer", what);
    return 0;
}

// 0 when scan_work can be a work area, else the refusal in what's name
int scan_work_check(const char* what, const int* scan_work);

// ---- scan -------------------------------------------------------------------------------------------------------------------------
// out[0 .. n] = the exclusive prefix sums of in[0 .. n), *total = the sum (total null: kept in the work area's last top slot,
// which no scan of at most 2^31 elements reaches); e0 / e1 as in RCMVS_LAUNCH_TIMED (either may be null).
// T: unsigned char or int, no element negative, every sum below 2^32.
template <class T>
void scan3(const T* in, long long n, int* out, int* work, unsigned long long* total, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// p[0 .. n) = 0 (T: int or unsigned long long), one thread per element
template <class T>
__global__ __launch_bounds__(SS_BLOCK) void zero_kernel(T* __restrict__ p, long long n);

// ---- sort -------------------------------------------------------------------------------------------------------------------------
// One pass of the sort of (key, index) pairs on bits shift .. shift + 7 (K: unsigned long long or unsigned), blocks of SS_BLOCK keys:
// hist[d * nblk + b] = the keys of block b whose digit is d; after an exclusive scan of hist into start, the scatter is stable.
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_hist_kernel(const K* __restrict__ key, long long n, int shift, long long nblk, int* __restrict__ hist);
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_scatter_kernel(const K* __restrict__ key_in, const int* __restrict__ idx_in, long long n,
                                                                 int shift, long long nblk, const int* __restrict__ start,
                                                                 K* __restrict__ key_out, int* __restrict__ idx_out);

// the 8-bit passes that sort keys up to largest_key: max(1, ceil(bits / 8))
int radix_passes(unsigned long long largest_key);

// `passes` stable passes from (*ka, *ia), pass p on bits 8p .. 8p + 7 (hist: 256 ceil(n / SS_BLOCK) ints, hist_start: one more,
// scan_work: a work area); on return *ka / *ia point at the buffers that hold the sorted pairs.  Nothing is launched for n <= 0.
template <class K>
void radix_sort(K** ka, int** ia, K** kb, int** ib, long long n, int passes, int* hist, int* hist_start, int* scan_work, hipStream_t st);

// seg[2k], seg[2k + 1] = where the run of key k starts and ends in the n sorted keys; keys >= m are sentinels and are skipped, and
// the rows of keys that do not occur keep what they held (the callers zero seg first)
__global__ __launch_bounds__(SS_BLOCK) void segments_kernel(const unsigned* __restrict__ sorted_key, long long n, int m, int* __restrict__ seg);

extern template void scan3<unsigned char>(const unsigned char*, long long, int*, int*, unsigned long long*, hipStream_t, hipEvent_t, hipEvent_t);
extern template void scan3<int>(const int*, long long, int*, int*, unsigned long long*, hipStream_t, hipEvent_t, hipEvent_t);
extern template __global__ void zero_kernel<int>(int* __restrict__, long long);
extern template __global__ void zero_kernel<unsigned long long>(unsigned long long* __restrict__, long long);
extern template __global__ void radix_hist_kernel<unsigned long long>(const unsigned long long* __restrict__, long long, int, long long, int* __restrict__);
extern template __global__ void radix_hist_kernel<unsigned>(const unsigned* __restrict__, long long, int, long long, int* __restrict__);
extern template __global__ void radix_scatter_kernel<unsigned long long>(const unsigned long long* __restrict__, const int* __restrict__, long long, int,
                                                                         long long, const int* __restrict__, unsigned long long* __restrict__,
                                                                         int* __restrict__);
extern template __global__ void radix_scatter_kernel<unsigned>(const unsigned* __restrict__, const int* __restrict__, long long, int, long long,
                                                               const int* __restrict__, unsigned* __restrict__, int* __restrict__);
extern template void radix_sort<unsigned long long>(unsigned long long**, int**, unsigned long long**, int**, long long, int, int*, int*, int*, hipStream_t);
extern template void radix_sort<unsigned>(unsigned**, int**, unsigned**, int**, long long, int, int*, int*, int*, hipStream_t);

}  // namespace rcmvs
