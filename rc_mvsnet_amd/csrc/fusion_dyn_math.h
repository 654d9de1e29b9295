// Per-pixel arithmetic of the DYNAMIC depth-map fusion filter (csrc/fusion_dyn.hip; DESIGN.md, "Dynamic consistency and one point
// per surface").  Plain C++ shared by the kernel, the CPU emulation and tests/fusion_dyn_math_check.cpp; tests/fusion_dyn_oracle.py
// restates it in numpy without calling it.
//
// The chain of one (reference pixel, source view) pair up to dist (fp64), rel (fp32), d_rep, x_src and y_src is fu::reproject's
// (fusion_math.h): the same operations in the same order with the same float32 cast points, contraction off.  Only what is done
// with dist and rel differs.  Source i PASSES LEVEL n when dist_i < (double)n * dist_base and rel_i < (float)n * rel_base, each
// product one rounded operation, every comparison with NaN false.  The products depend on nothing per pixel, so the host takes them
// once (levels()) and the kernel receives the two tables by value.
#pragma once
#include "fusion_math.h"

namespace rcmvs {
namespace fu {

constexpr int DYN_MAX_LEVEL = 16;                                  // == RCMVS_FUSE_MAX_SRC

#pragma clang fp contract(off)
struct Levels {
    double dist_t[DYN_MAX_LEVEL];                                  // [n - 1] = (double)n * dist_base
    float rel_t[DYN_MAX_LEVEL];                                    // [n - 1] = (float)n * rel_base
    int lo, hi;                                                    // 1 <= lo <= hi <= DYN_MAX_LEVEL
};

RCMVS_HD Levels levels(int lo, int hi, double dist_base, float rel_base) {
    Levels L;
    for (int n = 1; n <= DYN_MAX_LEVEL; ++n) {
        L.dist_t[n - 1] = (double)n * dist_base;
        L.rel_t[n - 1] = (float)n * rel_base;
    }
    L.lo = lo; L.hi = hi;
    return L;
}

// the sampling position of reference pixel (x, y) at depth d_ref in one source view: the first half of fu::reproject
RCMVS_HD void source_position(const double* rm, const double* sm, int x, int y, float d_ref, double* xs, double* ys) {
    const double d = (double)d_ref;
    double p[3], q[3], k[3];
    mul3(rm, (double)x * d, (double)y * d, d, p);                      // reference camera space
    mul34(sm, p, q);                                                   // source camera space
    mul3(sm + 12, q[0], q[1], q[2], k);
    *xs = k[0] / k[2]; *ys = k[1] / k[2];
}

struct Raw { double dist; float rel, d_rep, x_src, y_src; };

// fu::reproject without its two thresholds: the distances themselves
RCMVS_HD Raw reproject_raw(const double* rm, const double* sm, const float* depth_src, int H, int W, int x, int y, float d_ref) {
    double xs, ys, p[3], q[3], k[3];
    source_position(rm, sm, x, y, d_ref, &xs, &ys);
    Raw r;
    r.x_src = (float)xs; r.y_src = (float)ys;
    const double s = (double)remap_linear(depth_src, H, W, r.x_src, r.y_src);
    mul3(sm + 21, xs * s, ys * s, s, p);                               // back into source camera space at the sampled depth
    mul34(sm + 30, p, q);                                              // reference camera space
    r.d_rep = (float)q[2];
    mul3(rm + 9, q[0], q[1], q[2], k);
    const float xr = (float)(k[0] / k[2]), yr = (float)(k[1] / k[2]);
    const double dx = (double)xr - (double)x, dy = (double)yr - (double)y;
    r.dist = sqrt(dx * dx + dy * dy);
    r.rel = fabsf(r.d_rep - d_ref) / d_ref;
    return r;
}

// bit n - 1 set when the source passes level n, for n in [lo, hi]
RCMVS_HD unsigned pass_bits(const Levels& L, double dist, float rel) {
    unsigned bits = 0;
#pragma unroll
    for (int n = 1; n <= DYN_MAX_LEVEL; ++n) {
        const bool in = n >= L.lo && n <= L.hi;
        const bool pass = (dist < L.dist_t[n - 1]) && (rel < L.rel_t[n - 1]);
        bits |= (in && pass) ? (1u << (n - 1)) : 0u;
    }
    return bits;
}

// The 16 per-level counts, each at most 16, as bytes of four words (level n in byte (n - 1) % 4 of word (n - 1) / 4): four
// registers instead of sixteen, and four additions per source.
struct Counts { unsigned w[DYN_MAX_LEVEL / 4]; };
RCMVS_HD void count_add(Counts& c, unsigned bits) {
#pragma unroll
    for (int k = 0; k < DYN_MAX_LEVEL / 4; ++k) {
        const unsigned four = (bits >> (4 * k)) & 15u;                 // bits 0..3 -> bytes 0..3
        c.w[k] += (four & 1u) | ((four & 2u) << 7) | ((four & 4u) << 14) | ((four & 8u) << 21);
    }
}
RCMVS_HD int count_of(const Counts& c, int n) { return (int)((c.w[(n - 1) / 4] >> (8 * ((n - 1) % 4))) & 255u); }

// the smallest level of [lo, hi] set in bits, 0 for none
RCMVS_HD int lowest_level(unsigned bits) {
    int level = 0;
#pragma unroll
    for (int n = DYN_MAX_LEVEL; n >= 1; --n) level = (bits >> (n - 1)) & 1u ? n : level;
    return level;
}

// The pixel a fused point accounts for in a source view: the nearest pixel of the sampling position, ties to even, or false where
// remap_linear's far guard or the image bounds reject the position.
RCMVS_HD bool mark_pixel(float x_src, float y_src, int H, int W, int* mx, int* my) {
    const float fx32 = x_src * 32.0f, fy32 = y_src * 32.0f;
    if (!(fabsf(fx32) < 1.0e9f) || !(fabsf(fy32) < 1.0e9f)) return false;
    *mx = (int)rintf(x_src); *my = (int)rintf(y_src);
    return *mx >= 0 && *mx < W && *my >= 0 && *my < H;
}

// One reference pixel against its N sources: the per-level counts, the level, the averaged depth.
struct Pixel {
    int level;                                                     // smallest n in [lo, hi] with count_n >= n, 0 for none
    int count_hi;                                                  // sources that pass level hi
    unsigned hi_bits;                                              // bit i: source i passes level hi
    double avg;                                                    // (double)(acc + d_ref) / (double)(count_hi + 1)
};

// src_view[n] indexes depth_all; dbg_* may be NULL; stride = H * W, p = y * W + x
RCMVS_HD Pixel fuse_pixel(const double* mats, const float* depth_all, const int* src_view, int N, const Levels& L, int H, int W,
                          int x, int y, float d_ref, float* dbg_depth, unsigned char* dbg_level, float* dbg_xy) {
    const long long plane = (long long)H * W, p = (long long)y * W + x;
    Counts cnt = {{0u, 0u, 0u, 0u}};
    Pixel out;
    out.hi_bits = 0;
    float acc = 0.0f;                                              // 0 + d_1 + d_2 + ... in float32, a failing source adds 0
    for (int i = 0; i < N; ++i) {
        const Raw r = reproject_raw(mats, mats + REF_MATS + i * SRC_MATS, depth_all + (long long)src_view[i] * plane, H, W, x, y, d_ref);
        const unsigned bits = pass_bits(L, r.dist, r.rel);
        count_add(cnt, bits);
        const bool pass_hi = (bits >> (L.hi - 1)) & 1u;
        const float d = pass_hi ? r.d_rep : 0.0f;
        acc += d;
        out.hi_bits |= pass_hi ? (1u << i) : 0u;
        if (dbg_depth) dbg_depth[i * plane + p] = d;
        if (dbg_level) dbg_level[i * plane + p] = (unsigned char)lowest_level(bits);
        if (dbg_xy) { dbg_xy[(i * plane + p) * 2] = r.x_src; dbg_xy[(i * plane + p) * 2 + 1] = r.y_src; }
    }
    unsigned reached = 0;
#pragma unroll
    for (int n = 1; n <= DYN_MAX_LEVEL; ++n) reached |= (n >= L.lo && n <= L.hi && count_of(cnt, n) >= n) ? (1u << (n - 1)) : 0u;
    out.level = lowest_level(reached);
    out.count_hi = 0;
#pragma unroll
    for (int n = 1; n <= DYN_MAX_LEVEL; ++n) out.count_hi = n == L.hi ? count_of(cnt, n) : out.count_hi;
    out.avg = (double)(acc + d_ref) / (double)(out.count_hi + 1);
    return out;
}

}  // namespace fu
}  // namespace rcmvs
