// Device pieces of the TSDF kernels that the dense volume (tsdf_mesh.hip) and the block-sparse one (tsdf_sparse.hip) share: a
// voxel's walk through the views of one launch, a voxel's flags, a cube's edge mask, a tetrahedron's case,
// the block-wide sums and the upper two levels of the count scan.  One text, so the
// two volumes cannot drift apart in a bit.  Arithmetic and tables are tsdf_mesh_math.h's.
#pragma once
#include "tsdf_mesh.h"
#include "tsdf_mesh_math.h"

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int TM_BLOCK = 256;
constexpr int TM_TILE = RCMVS_TSDF_SCAN_TILE;
constexpr int TM_PER = TM_TILE / TM_BLOCK;                        // 8 voxels (or tile sums) per thread

// A voxel's state in registers
struct TmState {
    float d, w, r, g, b;
};

// The views of one launch for the voxel centre (px, py, pz): one fp32 add per view in view order.
__device__ __forceinline__ TmState tm_integrate_voxel(const float* __restrict__ depth, const unsigned char* __restrict__ rgb, int n, int H, int W,
                                                      const tsdf::Cams& cams, double trunc, double px, double py, double pz, bool colour, TmState s) {
    float d = s.d, w = s.w, r = s.r, gr = s.g, b = s.b;
    const size_t plane = (size_t)H * (size_t)W;
    for (int v = 0; v < n; ++v) {
        double val;
        int pix;
        if (!tsdf::observe(cams.c[v], px, py, pz, depth + (size_t)v * plane, H, W, trunc, &val, &pix)) continue;
        d += (float)val;
        w += 1.0f;
        if (colour) {
            const unsigned char* c = rgb + ((size_t)v * plane + (size_t)pix) * 3;
            r += (float)c[0];
            gr += (float)c[1];
            b += (float)c[2];
        }
    }
    return TmState{d, w, r, gr, b};
}

// bit 0: observed, bit 1: inside.  With w >= min_weight >= 1 the value (double)dsum / (double)w is < 0 exactly when dsum < 0 and w
// is finite (the quotient of an fp32 by an fp32 cannot underflow in fp64; dsum / inf is -0, which is not < 0), so the flags need
// no division; the emit kernel divides where it needs the value itself.
__device__ inline int tm_flags(const float* __restrict__ dsum, const float* __restrict__ wsum, int v, float min_weight) {
    const float w = wsum[v];
    if (!(w >= min_weight)) return 0;
    return (dsum[v] < 0.0f && w <= 3.402823466e+38f) ? 3 : 1;
}

__device__ inline unsigned tm_edge_mask(const int* f) {
    unsigned m = 0;
    if (f[0] & 1) {
#pragma unroll
        for (int c = 1; c < 8; ++c)
            if ((f[c] & 1) && ((f[c] ^ f[0]) & 2)) m |= 1u << (c - 1);
    }
    return m;
}

// the case of tetrahedron t, or 0 (no triangles) when one of its corners is not observed
__device__ inline int tm_tet_case(const int* f, int t) {
    int m = 0, obs = 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int fl = f[tsdf::tet_corner(t, c)];
        obs &= fl;
        m |= ((fl >> 1) & 1) << c;
    }
    return (obs & 1) ? m : 0;
}

// ---- block-wide sums, and the upper levels of the scan of per-tile sums (TM_TOP: the capacity of the top level) --------------
__device__ inline unsigned tm_block_sum(unsigned v, unsigned* sh) {     // sum of v over the block, in every thread; sh: TM_BLOCK
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = TM_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const unsigned r = sh[0];
    __syncthreads();
    return r;
}

__device__ inline unsigned tm_block_exclusive(unsigned v, unsigned* sh) {   // exclusive prefix of v over the block; sh: TM_BLOCK
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < TM_BLOCK; o <<= 1) {
        const unsigned t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const unsigned r = sh[threadIdx.x] - v;
    __syncthreads();
    return r;
}

// sums of TM_TILE tile sums, in 64 bits
template <int TM_TOP>
__global__ __launch_bounds__(TM_BLOCK) void tsdf_scan_up_kernel(const unsigned* __restrict__ tile_v, const unsigned* __restrict__ tile_t, int nb1,
                                                                unsigned long long* __restrict__ top) {
    __shared__ unsigned long long sh[2][TM_BLOCK];
    const long long base = (long long)blockIdx.x * TM_TILE + (long long)threadIdx.x * TM_PER;
    unsigned long long a = 0, b = 0;
    for (int q = 0; q < TM_PER; ++q)
        if (base + q < nb1) { a += tile_v[base + q]; b += tile_t[base + q]; }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = TM_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { top[blockIdx.x] = sh[0][0]; top[TM_TOP + blockIdx.x] = sh[1][0]; }
}

// the top level in place: top[0..nb2) and top[TM_TOP..TM_TOP+nb2) -> exclusive prefixes; totals = the two sums
template <int TM_TOP>
__global__ void tsdf_scan_top_kernel(unsigned long long* __restrict__ top, int nb2, unsigned long long* __restrict__ totals) {
    if (threadIdx.x > 1 || blockIdx.x != 0) return;
    unsigned long long* t = top + (size_t)threadIdx.x * TM_TOP;
    unsigned long long run = 0;
    for (int b = 0; b < nb2; ++b) { const unsigned long long c = t[b]; t[b] = run; run += c; }
    totals[threadIdx.x] = run;
}

// tile sums -> their exclusive prefixes, in place (32 bit, wrapping)
template <int TM_TOP>
__global__ __launch_bounds__(TM_BLOCK) void tsdf_scan_mid_kernel(unsigned* __restrict__ tile_v, unsigned* __restrict__ tile_t, int nb1,
                                                                 const unsigned long long* __restrict__ top) {
    __shared__ unsigned sh[TM_BLOCK];
    const long long base = (long long)blockIdx.x * TM_TILE + (long long)threadIdx.x * TM_PER;
    for (int which = 0; which < 2; ++which) {
        unsigned* tile = which ? tile_t : tile_v;
        unsigned c[TM_PER], s = 0;
#pragma unroll
        for (int q = 0; q < TM_PER; ++q) { c[q] = base + q < nb1 ? tile[base + q] : 0u; s += c[q]; }
        unsigned run = tm_block_exclusive(s, sh) + (unsigned)top[which * TM_TOP + blockIdx.x];
#pragma unroll
        for (int q = 0; q < TM_PER; ++q) { if (base + q < nb1) tile[base + q] = run; run += c[q]; }
    }
}

}  // namespace rcmvs
