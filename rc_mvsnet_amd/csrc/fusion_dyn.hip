// Depth-map fusion with dynamic consistency and one point per surface (csrc/fusion_dyn.h; DESIGN.md, "Dynamic consistency and one
// point per surface").  The fixed filter of fusion.hip asks for num_consistent sources inside ONE pair of thresholds; here a pixel
// is kept when n sources agree within n times the base thresholds for some n of [level_lo, level_hi] -- a few views tightly or
// many loosely -- and, optionally, a fused point marks the source pixels it accounts for so that later reference views skip them.
// gfx950 only.
//
// One thread per reference pixel walks the N sources, as fuse_view_kernel does, with the same addressing.  The level thresholds
// are wave-uniform (kernel arguments, formed once on the host), the per-level counts live in registers (every loop over levels
// is unrolled, so no array is indexed by a run-time value), and there is no LDS and no atomic.  The marks need the sampling
// positions of the sources again AFTER the pixel is known to be kept; they are formed a second time by the same function
// (fu::source_position: three small matrix products and two divisions, no memory access) only for kept pixels of a launch that
// has a `used` array, which keeps 2 N floats per thread out of scratch.
//
// Why the marks cannot race: the launch reads plane ref_idx of `used` only, a mark is written to planes other than ref_idx only
// (a source that is the reference view itself is skipped), and every mark is the byte 1 written by a plain store.  No thread reads
// what another thread of the launch writes, and two threads that hit one byte write the same value.
#include "common.h"
#include "fusion_dyn.h"
#include "fusion_dyn_math.h"

namespace rcmvs {

constexpr int FD_BLOCK = 256;

struct DynSrc { int v[RCMVS_FUSE_MAX_SRC]; };

__global__ __launch_bounds__(FD_BLOCK) void fuse_view_dyn_kernel(
    const float* __restrict__ depth_all, int ref_idx, DynSrc src, const float* __restrict__ conf, const float* __restrict__ img,
    const double* __restrict__ mats, float prob_thresh, fu::Levels L, unsigned char* used, unsigned char* __restrict__ masks,
    unsigned char* __restrict__ level, float* __restrict__ depth_avg, float* __restrict__ xyz, unsigned char* __restrict__ rgb,
    float* __restrict__ dbg_depth, unsigned char* __restrict__ dbg_level, float* __restrict__ dbg_xy, int N, int H, int W) {
    const int p = blockIdx.x * FD_BLOCK + threadIdx.x;
    const int plane = H * W;
    if (p >= plane) return;
    const int y = p / W, x = p - y * W;
    const float d_ref = depth_all[(long long)ref_idx * plane + p];
    const fu::Pixel px = fu::fuse_pixel(mats, depth_all, src.v, N, L, H, W, x, y, d_ref, dbg_depth, dbg_level, dbg_xy);
    const bool photo = conf[p] > prob_thresh, geo = px.level != 0;
    const bool claimed = photo && geo && used != nullptr && used[(long long)ref_idx * plane + p] != 0;
    const bool keep = photo && geo && !claimed;
    masks[p] = photo; masks[plane + p] = geo; masks[2ll * plane + p] = keep; masks[3ll * plane + p] = claimed;
    level[p] = (unsigned char)px.level;
    depth_avg[p] = (float)px.avg;
    double wpt[3];
    fu::world_point(mats, x, y, px.avg, wpt);
    const long long p3 = (long long)p * 3;                       // H*W may reach 2^30 - 1: p * 3 does not fit 32 bits
    xyz[p3 + 0] = (float)wpt[0]; xyz[p3 + 1] = (float)wpt[1]; xyz[p3 + 2] = (float)wpt[2];
    if (img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[p3 + c] = (unsigned char)(int)(img[p3 + c] * 255.0f);
    }
    if (used != nullptr && keep) {
        for (int i = 0; i < N; ++i) {
            if (!((px.hi_bits >> i) & 1u) || src.v[i] == ref_idx) continue;
            double xs, ys;
            fu::source_position(mats, mats + fu::REF_MATS + i * fu::SRC_MATS, x, y, d_ref, &xs, &ys);
            int mx, my;
            if (fu::mark_pixel((float)xs, (float)ys, H, W, &mx, &my)) used[(long long)src.v[i] * plane + (long long)my * W + mx] = 1;
        }
    }
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_fuse_view_dyn(const float* depth_all, int n_views, int ref_idx, const int* src_idx_host, const float* conf,
                                   const float* img, const double* mats, float prob_thresh, int level_lo, int level_hi, double dist_base,
                                   float rel_base, unsigned char* used, unsigned char* masks, unsigned char* level, float* depth_avg,
                                   float* xyz, unsigned char* rgb, float* dbg_depth, unsigned char* dbg_level, float* dbg_xy, int N, int H,
                                   int W, void* stream) {
    RCMVS_REQUIRE(depth_all && src_idx_host && conf && mats && masks && level && depth_avg && xyz, "fuse_view_dyn: null pointer");
    RCMVS_REQUIRE((img == nullptr) == (rgb == nullptr), "fuse_view_dyn: img and rgb must be given together");
    RCMVS_REQUIRE(N >= 1 && N <= RCMVS_FUSE_MAX_SRC, "fuse_view_dyn: %d source views (1..%d)", N, RCMVS_FUSE_MAX_SRC);
    RCMVS_REQUIRE(level_lo >= 1 && level_lo <= level_hi && level_hi <= RCMVS_FUSE_MAX_SRC, "fuse_view_dyn: levels %d..%d (1 <= lo <= hi <= %d)",
                  level_lo, level_hi, RCMVS_FUSE_MAX_SRC);
    RCMVS_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 30) && n_views > 0, "fuse_view_dyn: bad dims H=%d W=%d n_views=%d", H, W, n_views);
    RCMVS_REQUIRE(ref_idx >= 0 && ref_idx < n_views, "fuse_view_dyn: reference view index %d outside the %d views", ref_idx, n_views);
    DynSrc s;
    for (int n = 0; n < RCMVS_FUSE_MAX_SRC; ++n) s.v[n] = n < N ? src_idx_host[n] : 0;
    for (int n = 0; n < N; ++n)
        RCMVS_REQUIRE(s.v[n] >= 0 && s.v[n] < n_views, "fuse_view_dyn: source view index %d outside the %d views", s.v[n], n_views);
    static_assert(fu::DYN_MAX_LEVEL == RCMVS_FUSE_MAX_SRC, "one level per source view at the most");
    const fu::Levels L = fu::levels(level_lo, level_hi, dist_base, rel_base);
    hipLaunchKernelGGL(fuse_view_dyn_kernel, dim3((H * W + FD_BLOCK - 1) / FD_BLOCK), dim3(FD_BLOCK), 0, as_stream(stream),
                       depth_all, ref_idx, s, conf, img, mats, prob_thresh, L, used, masks, level, depth_avg, xyz, rgb,
                       dbg_depth, dbg_level, dbg_xy, N, H, W);
    return launch_status("fuse_view_dyn");
}
