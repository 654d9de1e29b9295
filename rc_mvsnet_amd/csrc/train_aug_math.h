// Per-pixel arithmetic of the training loader's image preparation (datasets/dtu_train.py:90-161 of the reference): the uint8
// stage of transforms.ColorJitter as torchvision's PIL backend computes it -- ImageEnhance.Brightness / Contrast / Color and
// the HSV round trip of adjust_hue, each producing a new uint8 image -- restated so that every byte equals Pillow's.
// Plain C++ shared by train_aug.hip and the CPU loop harness of tests/test_train_aug_cpu.py (test infrastructure).
//
// Pillow's arithmetic (libImaging/Convert.c, Blend.c) mixes float and double; the precisions below are the ones that give
// zero mismatches over all 2^24 inputs of each conversion and must not be "simplified": the three hue quotients are fp32, the
// hue sum is fp64 rounded to fp32, the wrap into [0,1) is fp64 rounded to fp32, the scaling to bytes is fp64.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RCMVS_HD __host__ __device__ inline
#else
#define RCMVS_HD inline
#endif

namespace rcmvs {
namespace ta {

// ColorJitter's four operations, numbered as torchvision's fn_idx
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

// One view's parameters as the host uploads them: 8 32-bit words.
struct ViewParams {
    float factor[4];      // brightness, contrast, saturation factors (>= 0) and the hue factor in [-0.5, 0.5]
    int order[4];         // a permutation of 0..3: the operations in the order they are applied
};

// per-view exact integer sums of the statistics pass (8 words of 64 bits)
enum { SUM_X = 0, SUM_XX = 3, SUM_L = 6, SUM_WORDS = 8 };

#pragma clang fp contract(off)
// image.convert("L"): ITU-R 601-2 luma in 16.16 fixed point
RCMVS_HD int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImageEnhance's Image.blend(degenerate, image, factor) on one byte: interpolation for 0 <= f <= 1 (truncated), extrapolation
// with clipping beyond; the clipped form covers both because the interpolated value never leaves [0, 255].
RCMVS_HD int blend(int d, int x, float f) {
    const float t = (float)d + f * ((float)x - (float)d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// adjust_hue's uint8 shift: np.uint8(hue_factor * 255), i.e. truncation toward zero, then wrap-around
RCMVS_HD int hue_shift(float hue_factor) { return (int)((double)hue_factor * 255.0) & 255; }

// the degenerate image of ImageEnhance.Contrast: int(mean(L) + 0.5) from the exact sum of L over n pixels
RCMVS_HD int contrast_mean(unsigned long long sum_l, long long n) { return (int)((double)sum_l / (double)n + 0.5); }

RCMVS_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// image.convert("HSV") on one pixel (Convert.c rgb2hsv_row)
RCMVS_HD void rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    V = mx;
    if (mx == mn) { H = 0; S = 0; return; }
    const float cr = (float)(mx - mn);
    S = clip8((int)((double)(cr / (float)mx) * 255.0));
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    double hs;
    if (r == mx) hs = (double)bc - (double)gc;
    else if (g == mx) hs = 2.0 + (double)rc - (double)bc;
    else hs = 4.0 + (double)gc - (double)rc;
    const float h = (float)hs;
    const double w = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6]: fmod(w, 1.0) = w - floor(w), exact in fp64
    const float hw = (float)(w - floor(w));
    H = clip8((int)((double)hw * 255.0));
}

// image.convert("RGB") from HSV on one pixel (Convert.c hsv2rgb_row, colorsys form)
RCMVS_HD void hsv2rgb(int H, int S, int V, int& r, int& g, int& b) {
    if (S == 0) { r = g = b = V; return; }
    const double fs = (double)S / 255.0, h6 = (double)H * 6.0 / 255.0;
    const double fi = floor(h6), f = h6 - fi;
    const double v = (double)V;
    const int p = clip8((int)rint(v * (1.0 - fs)));
    const int q = clip8((int)rint(v * (1.0 - fs * f)));
    const int t = clip8((int)rint(v * (1.0 - fs * (1.0 - f))));
    switch ((int)fi % 6) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

// One operation on one pixel.  mean_l is only read by the contrast operation.
RCMVS_HD void apply_op(int op, const ViewParams& vp, int mean_l, int& r, int& g, int& b) {
    if (op == OP_BRIGHTNESS) {
        const float f = vp.factor[OP_BRIGHTNESS];
        r = blend(0, r, f); g = blend(0, g, f); b = blend(0, b, f);
    } else if (op == OP_CONTRAST) {
        const float f = vp.factor[OP_CONTRAST];
        r = blend(mean_l, r, f); g = blend(mean_l, g, f); b = blend(mean_l, b, f);
    } else if (op == OP_SATURATION) {
        const float f = vp.factor[OP_SATURATION];
        const int l = luma(r, g, b);
        r = blend(l, r, f); g = blend(l, g, f); b = blend(l, b, f);
    } else {
        int H, S, V;
        rgb2hsv(r, g, b, H, S, V);
        hsv2rgb((H + hue_shift(vp.factor[OP_HUE])) & 255, S, V, r, g, b);   // the round trip runs for a zero shift too (it is lossy)
    }
}

// The operations that precede contrast (what the statistics pass applies before it takes L).
RCMVS_HD void jitter_before_contrast(const ViewParams& vp, int& r, int& g, int& b) {
    for (int k = 0; k < 4 && vp.order[k] != OP_CONTRAST; ++k) apply_op(vp.order[k], vp, 0, r, g, b);
}

// All four operations.
RCMVS_HD void jitter(const ViewParams& vp, int mean_l, int& r, int& g, int& b) {
    for (int k = 0; k < 4; ++k) apply_op(vp.order[k], vp, mean_l, r, g, b);
}

// center_image (datasets/dtu_train.py:156-161) for one byte value from the exact sums of a channel: fp64, rounded once.
RCMVS_HD float centered(int x, unsigned long long sum_x, unsigned long long sum_xx, long long n) {
    const double mean = (double)sum_x / (double)n;
    double var = (double)sum_xx / (double)n - mean * mean;   // population variance; exactly 0 for a constant channel
    if (var < 0.0) var = 0.0;
    return (float)(((double)x - mean) / (sqrt(var) + 1e-8));
}

// 0 when the parameters are usable, else the number of the first rule they break (train_aug.hip words the message)
RCMVS_HD int params_fault(const ViewParams& vp) {
    int seen = 0;
    for (int k = 0; k < 4; ++k) {
        if (vp.order[k] < 0 || vp.order[k] > 3) return 1;
        seen |= 1 << vp.order[k];
    }
    if (seen != 15) return 1;
    for (int k = 0; k < 3; ++k)
        if (!(vp.factor[k] >= 0.0f) || std::isinf(vp.factor[k])) return 2;
    if (!(vp.factor[OP_HUE] >= -0.5f && vp.factor[OP_HUE] <= 0.5f)) return 3;
    return 0;
}

}  // namespace ta
}  // namespace rcmvs
