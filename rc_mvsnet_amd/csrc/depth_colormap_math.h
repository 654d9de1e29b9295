// Per-value arithmetic of the depth colour map (csrc/depth_colormap.hip), shared by the GPU kernels and the CPU emulation of
// tests/emu: the reference's write_depth_img_2 (eval_rcmvsnet_tanks.py:141-154) in the precision numpy and matplotlib use for
// an fp32 map -- each step in the precision numpy evaluates it in, under `fp contract(off)` in the order written.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RCMVS_HD __host__ __device__ inline
#else
#define RCMVS_HD inline
#endif

namespace rcmvs {
namespace dcm {

#pragma clang fp contract(off)

RCMVS_HD unsigned int float_bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
RCMVS_HD float bits_float(unsigned int u) { float f; memcpy(&f, &u, 4); return f; }

// An integer key with the order of the fp32 values: negative values have all bits flipped, the others the sign bit set.
// -0 sorts directly below +0; a NaN sorts outside the infinities (the kernels flag a NaN and never use its rank).
RCMVS_HD unsigned int order_key(float f) {
    const unsigned int u = float_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RCMVS_HD float key_value(unsigned int k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// numpy's default ('linear') percentile of n values, the part that does not need the data: the virtual index (n - 1) * q formed
// in fp32 (numpy 2.x takes the dtype of q / 100, which for an fp32 map is fp32), its floor and the interpolation weight.
struct Rank { unsigned int lo, hi; float g; };
inline Rank percentile_rank(long long n, double percentile) {
    const float q = (float)percentile / 100.0f;
    const float v = (float)(n - 1) * q;
    const float fl = floorf(v);
    Rank r;
    long long lo = (long long)fl;
    if (lo > n - 1) lo = n - 1;                    // a virtual index at or past the last value selects the last value twice
    if (lo < 0) lo = 0;
    r.lo = (unsigned int)lo;
    r.hi = (unsigned int)(lo + 1 < n ? lo + 1 : n - 1);
    r.g = v - fl;
    return r;
}

// numpy's _lerp of the two neighbouring order statistics a <= b with weight g
RCMVS_HD float lerp(float a, float b, float g) {
    const float d = b - a;
    if (g < 0.5f) { const float t = d * g; return a + t; }
    const float h = 1.0f - g;
    const float t = d * h;
    return b - t;
}

// Normalize(vmin, vmax) then Colormap.__call__ of a 256-entry map: -> index into the table, 256 = the "bad" colour (0, 0, 0).
// Normalize holds vmin and vmax as fp64 scalars and works in place on the fp32 map, so numpy evaluates `map -= vmin` and
// `map /= (vmax - vmin)` in fp64 and rounds each result to fp32: the numerator is the correctly rounded fp32 difference, the
// quotient an fp64 division of that numerator by the fp64 difference, rounded once more (tests/golden/tanks_eval.npz, case
// "wide", tells this from an all-fp32 and from an all-fp64 Normalize; within a factor of two of vmin all three agree).
// vmin == vmax gives 0 everywhere; the colour map then scales by 256 in fp32: x * 256 == 256 is the last entry and not "over";
// below 0 is the first, 256 and above the last entry (the map's default under / over colours); a NaN is bad.
RCMVS_HD int colour_index(float d, float vmin, float vmax) {
    float x;
    if (vmin == vmax) {
        x = 0.0f;
    } else {
        const float num = (float)((double)d - (double)vmin);
        const double den = (double)vmax - (double)vmin;
        x = (float)((double)num / den);
    }
    const float xa = x * 256.0f;
    if (xa != xa) return 256;
    if (xa == 256.0f) return 255;
    if (xa < 0.0f) return 0;
    if (xa >= 256.0f) return 255;
    return (int)xa;
}

}  // namespace dcm
}  // namespace rcmvs
