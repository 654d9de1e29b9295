// Image undistortion of the COLMAP import (rc_mvsnet_amd/colmap_import.py): an image of a camera with polynomial (Brown)
// distortion resampled to the pinhole camera of the same principal point and size, one launch per image.
//
//   A thread owns four consecutive pixels of the flat h * w pixel index: their 12 bytes start at a multiple of 12, so from a
//   4-byte aligned dst they leave as three aligned 32-bit stores (the last partial group, and an unaligned dst, as byte stores);
//   row and column come from the flat index.  Per pixel about forty fp64 operations give the source position; a position that
//   is not inside the image (NaN and +-inf included) writes (0, 0, 0) and counts as blank, and is never turned into an index.
//   A valid one reads its four neighbours (indices clamped into the image by ud::footprint) and blends them in fp64.
//   The blank count is added lanes -> waves -> block, then one integer atomic per block that has any: two runs give the same
//   bytes and the same count.  The camera and the eight coefficients travel as kernel arguments.
// Arithmetic in undistort_math.h.  gfx950 only; plain integer atomics, __syncthreads and shuffles (tests/emu compiles this file too).
#include <cstdint>

#include "common.h"
#include "undistort.h"
#include "undistort_math.h"

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int UD_BLOCK = 256;
constexpr int UD_WAVES = UD_BLOCK / WAVE;
constexpr int UD_PIXELS = 4;                                      // per thread: 12 bytes = three 32-bit words

__global__ __launch_bounds__(UD_BLOCK) void undistort_rgb8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h,
                                                                  int w, ud::Camera cam, int* __restrict__ blank) {
    __shared__ int sh_blank[UD_WAVES];
    const int n = h * w;                                          // 3 n < 2^31 (checked by the entry point)
    const int groups = (int)cdiv(n, UD_PIXELS);
    const int g = (int)blockIdx.x * UD_BLOCK + (int)threadIdx.x;   // groups <= 2^31 / 12, so neither product overflows
    int mine = 0;
    if (g < groups) {
        const int p0 = g * UD_PIXELS;
        const int cnt = n - p0 < UD_PIXELS ? n - p0 : UD_PIXELS;
        unsigned char b[3 * UD_PIXELS];
#pragma unroll
        for (int q = 0; q < UD_PIXELS; ++q) {
            b[3 * q] = b[3 * q + 1] = b[3 * q + 2] = 0;
            if (q >= cnt) continue;
            const int p = p0 + q, j = p / w, i = p - j * w;
            double us, vs;
            ud::source_position(cam, i, j, &us, &vs);
            if (!ud::valid(us, vs, w, h)) {
                mine += 1;
                continue;
            }
            int x0, x1, y0, y1;
            double ax, ay;
            ud::footprint(us, w, &x0, &x1, &ax);
            ud::footprint(vs, h, &y0, &y1, &ay);
            const unsigned char* __restrict__ r0 = src + 3 * (y0 * w);
            const unsigned char* __restrict__ r1 = src + 3 * (y1 * w);
#pragma unroll
            for (int c = 0; c < 3; ++c) b[3 * q + c] = ud::blend(r0[3 * x0 + c], r0[3 * x1 + c], r1[3 * x0 + c], r1[3 * x1 + c], ax, ay);
        }
        unsigned char* o = dst + 3 * p0;
        if (cnt == UD_PIXELS && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                o4[q] = (unsigned int)b[4 * q] | ((unsigned int)b[4 * q + 1] << 8) | ((unsigned int)b[4 * q + 2] << 16) | ((unsigned int)b[4 * q + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 3 * UD_PIXELS; ++k)
                if (k < 3 * cnt) o[k] = b[k];
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0) sh_blank[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < UD_WAVES; ++k) t += sh_blank[k];
        if (t) atomicAdd(blank, t);
    }
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_undistort_rgb8_timed(const unsigned char* src, unsigned char* dst, int h, int w, double fx, double fy, double cx, double cy,
                                          double fxo, double fyo, const double* dist8, int* blank, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(src && dst && dist8 && blank, "undistort_rgb8: null pointer");
    RCMVS_REQUIRE(src != dst, "undistort_rgb8: dst must differ from src (every output pixel gathers from the whole source)");
    RCMVS_REQUIRE(h >= 1 && w >= 1 && (long long)h * w * 3 < (1ll << 31), "undistort_rgb8: bad dims h=%d w=%d (each >= 1, h * w * 3 < 2^31)", h, w);
    RCMVS_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fxo) && std::isfinite(fyo) && fx > 0.0 && fy > 0.0 && fxo > 0.0 && fyo > 0.0,
                  "undistort_rgb8: focal lengths %g, %g -> %g, %g (finite, positive)", fx, fy, fxo, fyo);
    RCMVS_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "undistort_rgb8: principal point %g, %g (finite)", cx, cy);
    ud::Camera cam = {fx, fy, cx, cy, fxo, fyo, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (int k = 0; k < 8; ++k) {
        RCMVS_REQUIRE(std::isfinite(dist8[k]), "undistort_rgb8: coefficient %d is %g (finite; the order is k1 k2 p1 p2 k3 k4 k5 k6)", k, dist8[k]);
        cam.d[k] = dist8[k];
    }
    hipStream_t st = as_stream(stream);
    const hipError_t e = hipMemsetAsync(blank, 0, sizeof(int), st);
    if (e != hipSuccess) return fail((int)e, "undistort_rgb8: %s", hipGetErrorString(e));
    const unsigned blocks = (unsigned)cdiv(cdiv((long long)h * w, UD_PIXELS), UD_BLOCK);
    RCMVS_LAUNCH_TIMED(undistort_rgb8_kernel, dim3(blocks), dim3(UD_BLOCK), 0, st, static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1), src, dst, h,
                       w, cam, blank);
    return launch_status("undistort_rgb8");
}

extern "C" int rcmvs_undistort_rgb8(const unsigned char* src, unsigned char* dst, int h, int w, double fx, double fy, double cx, double cy,
                                    double fxo, double fyo, const double* dist8, int* blank, void* stream) {
    return rcmvs_undistort_rgb8_timed(src, dst, h, w, fx, fy, cx, cy, fxo, fyo, dist8, blank, nullptr, nullptr, stream);
}
