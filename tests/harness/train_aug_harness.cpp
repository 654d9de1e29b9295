// CPU loop harness around rc_mvsnet_amd/csrc/train_aug_math.h for tests/test_train_aug_cpu.py.  Test infrastructure only.
#include "../../rc_mvsnet_amd/csrc/train_aug_math.h"

using namespace rcmvs::ta;

// all 2^24 triples, index (a << 16) | (b << 8) | c -> 3 bytes each
extern "C" void h_rgb2hsv_cube(unsigned char* out) {
    for (int i = 0; i < (1 << 24); ++i) {
        int H, S, V;
        rgb2hsv(i >> 16, (i >> 8) & 255, i & 255, H, S, V);
        out[3 * i] = (unsigned char)H; out[3 * i + 1] = (unsigned char)S; out[3 * i + 2] = (unsigned char)V;
    }
}

extern "C" void h_hsv2rgb_cube(unsigned char* out) {
    for (int i = 0; i < (1 << 24); ++i) {
        int r, g, b;
        hsv2rgb(i >> 16, (i >> 8) & 255, i & 255, r, g, b);
        out[3 * i] = (unsigned char)r; out[3 * i + 1] = (unsigned char)g; out[3 * i + 2] = (unsigned char)b;
    }
}

// ColorJitter of one (n pixels, 3) uint8 image: params = ViewParams (8 words).  Returns params_fault().
extern "C" int h_jitter(const unsigned char* src, unsigned char* out, long long n, const void* params) {
    const ViewParams vp = *static_cast<const ViewParams*>(params);
    const int fault = params_fault(vp);
    if (fault) return fault;
    unsigned long long sum_l = 0;
    for (long long i = 0; i < n; ++i) {
        int r = src[3 * i], g = src[3 * i + 1], b = src[3 * i + 2];
        jitter_before_contrast(vp, r, g, b);
        sum_l += (unsigned long long)luma(r, g, b);
    }
    const int mean_l = contrast_mean(sum_l, n);
    for (long long i = 0; i < n; ++i) {
        int r = src[3 * i], g = src[3 * i + 1], b = src[3 * i + 2];
        jitter(vp, mean_l, r, g, b);
        out[3 * i] = (unsigned char)r; out[3 * i + 1] = (unsigned char)g; out[3 * i + 2] = (unsigned char)b;
    }
    return 0;
}

// center_image of one channel-interleaved image -> (3, n) fp32
extern "C" void h_center(const unsigned char* src, float* out, long long n) {
    for (int c = 0; c < 3; ++c) {
        unsigned long long sx = 0, sxx = 0;
        for (long long i = 0; i < n; ++i) { const unsigned long long x = src[3 * i + c]; sx += x; sxx += x * x; }
        for (long long i = 0; i < n; ++i) out[c * n + i] = centered(src[3 * i + c], sx, sxx, n);
    }
}
