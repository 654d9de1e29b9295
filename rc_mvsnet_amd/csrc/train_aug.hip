// Image preparation of the training loader on the device (datasets/dtu_train.py:90-161,266-268 of the reference): the V decoded
// views of one item, uint8 (V, H, W, 3), become the three fp32 (V, 3, H, W) tensors the training iteration reads --
//   imgs        ToTensor + Normalize                                  (transform_seg)
//   center_imgs (x - mean_c) / (sqrt(var_c) + 1e-8) per view, channel (center_image)
//   imgs_aug    ColorJitter on the bytes, / 255, pow(gamma), clamp, Normalize (transform_aug)
// ColorJitter's bytes equal Pillow's bit for bit (train_aug_math.h).  Two launches for all views (view on blockIdx.y):
//   1. statistics: the exact integer sums contrast and center_image need -- sum of L of the image as it is when contrast's
//      turn comes, sum x and sum x^2 per channel of the raw image.  Per-thread ints, wave shuffle, one 64-bit atomic per
//      block and sum: integer addition, so the result does not depend on the order the blocks retire in.
//   2. apply: a byte has 256 values, so everything after the bytes is a table -- 3 x 256 floats each for imgs and imgs_aug
//      (built by the host with torch's own ops, so pow / clamp / Normalize are torch's), and one for center_imgs that every
//      block forms in fp64 from the sums.  The tables sit in LDS (9 KB); a thread runs four neighbouring pixels through the
//      four operations and stores 16 B per lane to each of the nine output planes.
// 3 B read and 36 B written per pixel; DESIGN.md section 4 ("Training loader") has the measured times.  gfx950 only; plain atomics, shuffles
// and __syncthreads (tests/emu compiles this file too).
#include "common.h"
#include "train_aug_math.h"

namespace rcmvs {

constexpr int TA_BLOCK = 256;
constexpr int TA_PIX = 4;             // neighbouring pixels per thread in the apply pass: one float4 per output plane
constexpr int TA_STAT_PIX = 8;        // pixels per thread in the statistics pass

__global__ __launch_bounds__(TA_BLOCK) void train_stats_kernel(const unsigned char* __restrict__ src, const ta::ViewParams* __restrict__ params,
                                                               unsigned long long* __restrict__ sums, int HW) {
    __shared__ unsigned long long part[TA_BLOCK / WAVE][7];
    const int v = blockIdx.y;
    const ta::ViewParams vp = params[v];
    const unsigned char* s = src + (long long)v * HW * 3;
    unsigned int acc[7] = {0, 0, 0, 0, 0, 0, 0};                       // 8 pixels: at most 8 * 255^2 each
    const long long p0 = ((long long)blockIdx.x * TA_BLOCK + threadIdx.x) * TA_STAT_PIX;
    for (int j = 0; j < TA_STAT_PIX; ++j) {
        const long long p = p0 + j;
        if (p >= HW) break;
        int r = s[p * 3], g = s[p * 3 + 1], b = s[p * 3 + 2];
        acc[ta::SUM_X] += r; acc[ta::SUM_X + 1] += g; acc[ta::SUM_X + 2] += b;
        acc[ta::SUM_XX] += r * r; acc[ta::SUM_XX + 1] += g * g; acc[ta::SUM_XX + 2] += b * b;
        ta::jitter_before_contrast(vp, r, g, b);
        acc[ta::SUM_L] += ta::luma(r, g, b);
    }
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        unsigned int a = acc[k];                                        // a wave's sum: at most 64 * 8 * 255^2 < 2^32
        for (int off = WAVE / 2; off > 0; off >>= 1) a += __shfl_down(a, off);
        if (lane == 0) part[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        unsigned long long t = 0;
        for (int w = 0; w < TA_BLOCK / WAVE; ++w) t += part[w][threadIdx.x];
        atomicAdd(&sums[(long long)v * ta::SUM_WORDS + threadIdx.x], t);
    }
}

__global__ __launch_bounds__(TA_BLOCK) void train_apply_kernel(const unsigned char* __restrict__ src, const ta::ViewParams* __restrict__ params,
                                                               const unsigned long long* __restrict__ sums, const float* __restrict__ lut_seg,
                                                               const float* __restrict__ lut_aug, float* __restrict__ imgs,
                                                               float* __restrict__ center, float* __restrict__ aug,
                                                               unsigned char* __restrict__ u8_out, int HW, int vec) {
    __shared__ float t_seg[768], t_cen[768], t_aug[768];
    const int v = blockIdx.y;
    const unsigned long long* sv = sums + (long long)v * ta::SUM_WORDS;
    for (int i = threadIdx.x; i < 768; i += TA_BLOCK) {
        const int c = i >> 8;
        t_seg[i] = lut_seg[i];
        t_aug[i] = lut_aug[v * 768 + i];
        t_cen[i] = ta::centered(i & 255, sv[ta::SUM_X + c], sv[ta::SUM_XX + c], HW);
    }
    __syncthreads();
    const ta::ViewParams vp = params[v];
    const int mean_l = ta::contrast_mean(sv[ta::SUM_L], HW);
    const long long p0 = ((long long)blockIdx.x * TA_BLOCK + threadIdx.x) * TA_PIX;
    if (p0 >= HW) return;
    const int n = HW - p0 < TA_PIX ? (int)(HW - p0) : TA_PIX;
    const unsigned char* s = src + ((long long)v * HW + p0) * 3;
    float o[9][TA_PIX];
#pragma unroll
    for (int j = 0; j < TA_PIX; ++j) {
        if (j < n) {
            int r = s[j * 3], g = s[j * 3 + 1], b = s[j * 3 + 2];
            o[0][j] = t_seg[r]; o[1][j] = t_seg[256 + g]; o[2][j] = t_seg[512 + b];
            o[3][j] = t_cen[r]; o[4][j] = t_cen[256 + g]; o[5][j] = t_cen[512 + b];
            ta::jitter(vp, mean_l, r, g, b);
            o[6][j] = t_aug[r]; o[7][j] = t_aug[256 + g]; o[8][j] = t_aug[512 + b];
            if (u8_out) {
                unsigned char* u = u8_out + ((long long)v * HW + p0 + j) * 3;
                u[0] = (unsigned char)r; u[1] = (unsigned char)g; u[2] = (unsigned char)b;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k][j] = 0.0f;
        }
    }
    float* outs[3] = {imgs, center, aug};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float* dst = outs[k / 3] + ((long long)v * 3 + k % 3) * HW + p0;
        if (vec) {                                                     // H W is a multiple of 4 and the bases are 16-byte aligned: n == 4
            *reinterpret_cast<float4*>(dst) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        } else {
#pragma unroll
            for (int j = 0; j < TA_PIX; ++j)
                if (j < n) dst[j] = o[k][j];
        }
    }
}

static int check_params(const char* what, const void* params_host, int V) {
    const ta::ViewParams* p = static_cast<const ta::ViewParams*>(params_host);
    for (int v = 0; v < V; ++v) {
        const int fault = ta::params_fault(p[v]);
        RCMVS_REQUIRE(fault != 1, "%s: view %d: order (%d %d %d %d) is not a permutation of 0..3", what, v, p[v].order[0], p[v].order[1],
                      p[v].order[2], p[v].order[3]);
        RCMVS_REQUIRE(fault != 2, "%s: view %d: factors (%g %g %g) must be finite and >= 0", what, v, (double)p[v].factor[0],
                      (double)p[v].factor[1], (double)p[v].factor[2]);
        RCMVS_REQUIRE(fault != 3, "%s: view %d: hue factor %g is outside [-0.5, 0.5]", what, v, (double)p[v].factor[3]);
    }
    return 0;
}

static int check_dims(const char* what, int V, int H, int W) {
    RCMVS_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "%s: bad image size %dx%d", what, H, W);
    RCMVS_REQUIRE(V >= 1 && V <= 65535, "%s: V=%d is outside 1..65535", what, V);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_train_image_stats(const unsigned char* src, int V, int H, int W, const void* params_host, const void* params_dev,
                                       unsigned long long* sums, void* stream) {
    RCMVS_REQUIRE(src && params_host && params_dev && sums, "train_image_stats: null pointer");
    if (int rc = check_dims("train_image_stats", V, H, W)) return rc;
    if (int rc = check_params("train_image_stats", params_host, V)) return rc;
    const int HW = H * W;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * ta::SUM_WORDS * V, st) != hipSuccess) return launch_status("train_image_stats: memset");
    hipLaunchKernelGGL(train_stats_kernel, dim3((unsigned)cdiv(HW, TA_BLOCK * TA_STAT_PIX), V), dim3(TA_BLOCK), 0, st, src,
                       static_cast<const ta::ViewParams*>(params_dev), sums, HW);
    return launch_status("train_image_stats");
}

extern "C" int rcmvs_train_image_apply(const unsigned char* src, int V, int H, int W, const void* params_host, const void* params_dev,
                                       const unsigned long long* sums, const float* lut_seg, const float* lut_aug, float* imgs,
                                       float* center_imgs, float* imgs_aug, unsigned char* u8_out, void* stream) {
    RCMVS_REQUIRE(src && params_host && params_dev && sums && lut_seg && lut_aug && imgs && center_imgs && imgs_aug,
                  "train_image_apply: null pointer");
    if (int rc = check_dims("train_image_apply", V, H, W)) return rc;
    if (int rc = check_params("train_image_apply", params_host, V)) return rc;
    const int HW = H * W;
    const int vec = HW % TA_PIX == 0 && ((reinterpret_cast<uintptr_t>(imgs) | reinterpret_cast<uintptr_t>(center_imgs) |
                                          reinterpret_cast<uintptr_t>(imgs_aug)) & 15) == 0;
    hipLaunchKernelGGL(train_apply_kernel, dim3((unsigned)cdiv(HW, TA_BLOCK * TA_PIX), V), dim3(TA_BLOCK), 0, as_stream(stream), src,
                       static_cast<const ta::ViewParams*>(params_dev), sums, lut_seg, lut_aug, imgs, center_imgs, imgs_aug, u8_out, HW, vec);
    return launch_status("train_image_apply");
}
