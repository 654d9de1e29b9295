// The one three-level scan, the one radix sort and the small kernels around them that the mesh kernels share (declared in
// scan_sort.h; callers: mesh_clean.hip, mesh_decimate.hip, mesh_holes.hip, mesh_normals.hip, mesh_texture.hip, and pc_register.hip
// for the radix pass).
//
//   scan    Flags or counts -> exclusive prefix sums in three levels: tiles of 2048, 2048 tile sums, at most 1024 top sums by one
//           thread; 64-bit above the tile level.  The work area holds the top sums (uint64), then one unsigned per tile.
//   radix   Per-block digit histograms in LDS, digit-major (digit, block) table; after the caller's scan of that table a stable
//           scatter whose in-block rank comes from wave ballots (the keys of the same digit in the lanes and waves before).
//   sort    radix_sort: the loop hist -> scan3 of the table -> scatter -> swap buffers, as many passes as radix_passes says.
//   seg     segments_kernel: one thread per sorted key writes where its key's run starts or ends.
//   zero    zero_kernel: one thread per element.
// gfx950 only; __syncthreads, ballots, plain loads and stores and integer LDS atomics (tests/emu compiles this file too).
#include "scan_sort.h"
#include "tsdf_mesh_cells.h"                                      // tm_block_sum, tm_block_exclusive (256 threads)

namespace rcmvs {

constexpr int SS_PER = SS_TILE / SS_BLOCK;
constexpr int SS_WAVES = SS_BLOCK / WAVE;
static_assert(SS_BLOCK == TM_BLOCK, "tm_block_sum and tm_block_exclusive reduce TM_BLOCK threads");
static_assert(SS_BLOCK == 256, "a radix block's threads are its 256 digits' histogram slots");

using u64 = unsigned long long;

// ---- the three-level scan of one array (T: bytes or non-negative ints; every sum below 2^32) --------------------------------
template <class T>
__global__ __launch_bounds__(SS_BLOCK) void tile_sum_kernel(const T* __restrict__ in, long long n, unsigned* __restrict__ tile) {
    __shared__ unsigned sh[SS_BLOCK];
    const long long base = (long long)blockIdx.x * SS_TILE + (long long)threadIdx.x * SS_PER;
    unsigned s = 0;
    for (int q = 0; q < SS_PER; ++q)
        if (base + q < n) s += (unsigned)in[base + q];
    const unsigned t = tm_block_sum(s, sh);
    if (threadIdx.x == 0) tile[blockIdx.x] = t;
}

__global__ __launch_bounds__(SS_BLOCK) void scan_up_kernel(const unsigned* __restrict__ tile, int nb1, u64* __restrict__ top) {
    __shared__ u64 sh[SS_BLOCK];
    const long long base = (long long)blockIdx.x * SS_TILE + (long long)threadIdx.x * SS_PER;
    u64 a = 0;
    for (int q = 0; q < SS_PER; ++q)
        if (base + q < nb1) a += tile[base + q];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = SS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) top[blockIdx.x] = sh[0];
}

__global__ void scan_top_kernel(u64* __restrict__ top, int nb2, u64* __restrict__ total) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u64 run = 0;
    for (int b = 0; b < nb2; ++b) { const u64 c = top[b]; top[b] = run; run += c; }
    *total = run;
}

__global__ __launch_bounds__(SS_BLOCK) void scan_mid_kernel(unsigned* __restrict__ tile, int nb1, const u64* __restrict__ top) {
    __shared__ unsigned sh[SS_BLOCK];
    const long long base = (long long)blockIdx.x * SS_TILE + (long long)threadIdx.x * SS_PER;
    unsigned c[SS_PER], s = 0;
#pragma unroll
    for (int q = 0; q < SS_PER; ++q) { c[q] = base + q < nb1 ? tile[base + q] : 0u; s += c[q]; }
    unsigned run = tm_block_exclusive(s, sh) + (unsigned)top[blockIdx.x];
#pragma unroll
    for (int q = 0; q < SS_PER; ++q) { if (base + q < nb1) tile[base + q] = run; run += c[q]; }
}

template <class T>
__global__ __launch_bounds__(SS_BLOCK) void scan_down_kernel(const T* __restrict__ in, long long n, const unsigned* __restrict__ tile,
                                                             const u64* __restrict__ total, int* __restrict__ out) {
    __shared__ unsigned sh[SS_BLOCK];
    const long long base = (long long)blockIdx.x * SS_TILE + (long long)threadIdx.x * SS_PER;
    unsigned c[SS_PER], s = 0;
#pragma unroll
    for (int q = 0; q < SS_PER; ++q) { c[q] = base + q < n ? (unsigned)in[base + q] : 0u; s += c[q]; }
    unsigned run = tm_block_exclusive(s, sh) + tile[blockIdx.x];
#pragma unroll
    for (int q = 0; q < SS_PER; ++q) { if (base + q < n) out[base + q] = (int)run; run += c[q]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = (int)(unsigned)*total;
}

template <class T>
void scan3(const T* in, long long n, int* out, int* work, u64* total, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    const int nb1 = (int)(n > 0 ? cdiv(n, SS_TILE) : 1), nb2 = (int)cdiv(nb1, SS_TILE);
    u64* top = reinterpret_cast<u64*>(work);
    unsigned* tile = reinterpret_cast<unsigned*>(work) + SS_WORK;
    if (!total) total = top + (SS_TOP - 1);
    hipEvent_t none = nullptr;
    RCMVS_LAUNCH_TIMED(tile_sum_kernel<T>, dim3(nb1), dim3(SS_BLOCK), 0, st, e0, none, in, n, tile);
    hipLaunchKernelGGL(scan_up_kernel, dim3(nb2), dim3(SS_BLOCK), 0, st, tile, nb1, top);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(64), 0, st, top, nb2, total);
    hipLaunchKernelGGL(scan_mid_kernel, dim3(nb2), dim3(SS_BLOCK), 0, st, tile, nb1, top);
    RCMVS_LAUNCH_TIMED(scan_down_kernel<T>, dim3(nb1), dim3(SS_BLOCK), 0, st, none, e1, in, n, tile, total, out);
}

template void scan3<unsigned char>(const unsigned char*, long long, int*, int*, u64*, hipStream_t, hipEvent_t, hipEvent_t);
template void scan3<int>(const int*, long long, int*, int*, u64*, hipStream_t, hipEvent_t, hipEvent_t);

int scan_work_check(const char* what, const int* scan_work) {
    RCMVS_REQUIRE(scan_work, "%s: null pointer", what);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(scan_work) & 7) == 0, "%s: scan_work must be 8-byte aligned", what);
    return 0;
}

template <class T>
__global__ __launch_bounds__(SS_BLOCK) void zero_kernel(T* __restrict__ p, long long n) {
    const long long i = gid();
    if (i < n) p[i] = 0;
}

template __global__ void zero_kernel<int>(int* __restrict__, long long);
template __global__ void zero_kernel<u64>(u64* __restrict__, long long);

// ---- one pass of the radix sort of (key, index) pairs --------------------------------------------------------------------------
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_hist_kernel(const K* __restrict__ key, long long n, int shift, long long nblk,
                                                              int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (i < n) atomicAdd(&h[(int)((key[i] >> shift) & (K)255)], 1);
    __syncthreads();
    hist[(long long)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// stable: a key goes to start[digit][block] + the keys of the same digit before it in the block (waves before it, lanes before it)
template <class K>
__global__ __launch_bounds__(SS_BLOCK) void radix_scatter_kernel(const K* __restrict__ key_in, const int* __restrict__ idx_in, long long n,
                                                                 int shift, long long nblk, const int* __restrict__ start,
                                                                 K* __restrict__ key_out, int* __restrict__ idx_out) {
    __shared__ int wh[SS_WAVES][256];
#pragma unroll
    for (int w = 0; w < SS_WAVES; ++w) wh[w][threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * SS_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const K k = valid ? key_in[i] : (K)0;
    const int d = (int)((k >> shift) & (K)255);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
    }
    const int before = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && before == 0) wh[wave][d] = __popcll(peers);
    __syncthreads();
    if (valid) {
        long long dst = (long long)start[(long long)d * nblk + blockIdx.x] + before;
        for (int w = 0; w < wave; ++w) dst += wh[w][d];
        if (dst >= 0 && dst < n) {
            key_out[dst] = k;
            idx_out[dst] = idx_in[i];
        }
    }
}

template __global__ void radix_hist_kernel<u64>(const u64* __restrict__, long long, int, long long, int* __restrict__);
template __global__ void radix_hist_kernel<unsigned>(const unsigned* __restrict__, long long, int, long long, int* __restrict__);
template __global__ void radix_scatter_kernel<u64>(const u64* __restrict__, const int* __restrict__, long long, int, long long, const int* __restrict__,
                                                   u64* __restrict__, int* __restrict__);
template __global__ void radix_scatter_kernel<unsigned>(const unsigned* __restrict__, const int* __restrict__, long long, int, long long,
                                                        const int* __restrict__, unsigned* __restrict__, int* __restrict__);

// ---- the passes ---------------------------------------------------------------------------------------------------------------------
int radix_passes(u64 largest_key) {
    int bits = 0;
    for (u64 top = largest_key; top; top >>= 1) ++bits;
    const int passes = (bits + 7) / 8;
    return passes < 1 ? 1 : passes;
}

template <class K>
void radix_sort(K** ka, int** ia, K** kb, int** ib, long long n, int passes, int* hist, int* hist_start, int* scan_work, hipStream_t st) {
    if (n <= 0) return;
    const long long nblk = cdiv(n, SS_BLOCK);
    hipEvent_t none = nullptr;
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(radix_hist_kernel<K>, dim3((unsigned)nblk), dim3(SS_BLOCK), 0, st, *ka, n, 8 * p, nblk, hist);
        scan3<int>(hist, 256 * nblk, hist_start, scan_work, nullptr, st, none, none);
        hipLaunchKernelGGL(radix_scatter_kernel<K>, dim3((unsigned)nblk), dim3(SS_BLOCK), 0, st, *ka, *ia, n, 8 * p, nblk, hist_start, *kb, *ib);
        K* tk = *ka; *ka = *kb; *kb = tk;
        int* ti = *ia; *ia = *ib; *ib = ti;
    }
}

template void radix_sort<u64>(u64**, int**, u64**, int**, long long, int, int*, int*, int*, hipStream_t);
template void radix_sort<unsigned>(unsigned**, int**, unsigned**, int**, long long, int, int*, int*, int*, hipStream_t);

// ---- segments of the sorted keys ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void segments_kernel(const unsigned* __restrict__ key, long long n, int m, int* __restrict__ seg) {
    const long long i = gid();
    if (i >= n) return;
    const unsigned k = key[i];
    if (k >= (unsigned)m) return;
    if (i == 0 || key[i - 1] != k) seg[2 * (size_t)k] = (int)i;
    if (i == n - 1 || key[i + 1] != k) seg[2 * (size_t)k + 1] = (int)(i + 1);
}

}  // namespace rcmvs
