// COLMAP import (rc_mvsnet_amd/colmap_import.py): the two passes of the community converter that grow with the model, on a
// sparse model held as device arrays (centres, points, per image an ascending CSR list of point indices):
//
//   scores    one wave per image pair i < j (a block holds four pairs of one row).  Early out when the two id ranges do not
//             overlap; lanes stride over the shorter list and binary-search the longer one (the lower bound only moves up, so
//             each search starts where the lane's previous one ended); each lane adds its weights in ascending order, a fixed
//             xor butterfly adds the lanes, lane 0 stores (i,j) and (j,i).  No atomics, no scratch: two runs give the same bits.
//   top       one block per row: k rounds of "the best partner after the previous pick" in the order (score descending, index
//             ascending), reduced lanes -> waves -> block; partners with score 0 are never listed.
//   depth     one block per image: z of every listed point as an order-preserving 64-bit key in a global work buffer, then per
//             rank an MSB-first radix select (8 passes of an LDS digit histogram over the keys that match the prefix so far).
// Arithmetic in view_select_math.h.  gfx950 only; plain LDS integer atomics, __syncthreads and shuffles (tests/emu compiles this
// file too).
#include <climits>

#include "common.h"
#include "view_select.h"
#include "view_select_math.h"

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int VS_BLOCK = 256;
constexpr int VS_WAVES = VS_BLOCK / WAVE;

// list of image i as positions [lo, hi) of ids, clamped into [0, nnz] whatever offsets holds
__device__ inline void vs_list(const long long* __restrict__ offsets, int i, long long nnz, long long* lo, long long* hi) {
    long long a = offsets[i], b = offsets[i + 1];
    a = a < 0 ? 0 : (a > nnz ? nnz : a);
    b = b < a ? a : (b > nnz ? nnz : b);
    *lo = a;
    *hi = b;
}

// ---- pair scores ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_BLOCK) void vs_pair_scores_kernel(const double* __restrict__ centres, int n, const double* __restrict__ points,
                                                                  long long m, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ ids, long long nnz, double theta0, double sigma1,
                                                                  double sigma2, int chunks, double* __restrict__ scores) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (int)(blockIdx.x / (unsigned)chunks);
    const int j = (int)(blockIdx.x % (unsigned)chunks) * VS_WAVES + wave;
    if (i >= n || j >= n || j < i) return;                        // uniform over the wave
    if (j == i) {
        if (lane == 0) scores[(long long)i * n + i] = 0.0;
        return;
    }
    long long a0, a1, b0, b1;
    vs_list(offsets, i, nnz, &a0, &a1);
    vs_list(offsets, j, nnz, &b0, &b1);
    double acc = 0.0;
    if (a1 > a0 && b1 > b0 && ids[a1 - 1] >= ids[b0] && ids[b1 - 1] >= ids[a0]) {
        const bool i_short = a1 - a0 <= b1 - b0;
        const long long s0 = i_short ? a0 : b0, s1 = i_short ? a1 : b1;
        const long long l0 = i_short ? b0 : a0, l1 = i_short ? b1 : a1;
        const double ci[3] = {centres[3 * i + 0], centres[3 * i + 1], centres[3 * i + 2]};
        const double cj[3] = {centres[3 * j + 0], centres[3 * j + 1], centres[3 * j + 2]};
        long long from = l0;
        for (long long s = s0 + lane; s < s1; s += WAVE) {
            const int p = ids[s];
            long long lo = from, hi = l1;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (ids[mid] < p) lo = mid + 1; else hi = mid;
            }
            from = lo;
            if (lo < l1 && ids[lo] == p && p >= 0 && (long long)p < m) {
                const double* x = points + 3ll * p;
                const double xp[3] = {x[0], x[1], x[2]};
                acc += vs::weight(vs::angle_deg(ci, cj, xp), theta0, sigma1, sigma2);
            }
        }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        scores[(long long)i * n + j] = acc;
        scores[(long long)j * n + i] = acc;
    }
}

// ---- top views ------------------------------------------------------------------------------------------------------
__device__ inline bool vs_better(double s, int i, double bs, int bi) { return s > bs || (s == bs && i < bi); }

__global__ __launch_bounds__(VS_BLOCK) void vs_top_views_kernel(const double* __restrict__ scores, int n, int k, int* __restrict__ top_ids,
                                                                double* __restrict__ top_scores, int* __restrict__ counts) {
    __shared__ double sh_s[VS_WAVES];
    __shared__ int sh_i[VS_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const double* __restrict__ s = scores + (long long)row * n;
    int c = 0;
    for (int j = tid; j < n; j += VS_BLOCK) c += (j != row && s[j] > 0.0) ? 1 : 0;
    for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) sh_i[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < VS_WAVES; ++w) t += sh_i[w];
        counts[row] = t;
    }
    __syncthreads();
    double prev_s = INFINITY;
    int prev_i = -1;
    for (int r = 0; r < k; ++r) {
        double bs = 0.0;                                          // none yet: a listed partner has score > 0
        int bi = INT_MAX;
        for (int j = tid; j < n; j += VS_BLOCK) {
            const double v = s[j];
            if (j == row || !(v > 0.0)) continue;
            const bool after = v < prev_s || (v == prev_s && j > prev_i);
            if (after && vs_better(v, j, bs, bi)) { bs = v; bi = j; }
        }
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o);
            const int oi = __shfl_xor(bi, o);
            if (vs_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { sh_s[wave] = bs; sh_i[wave] = bi; }
        __syncthreads();
        bs = sh_s[0]; bi = sh_i[0];
        for (int w = 1; w < VS_WAVES; ++w)
            if (vs_better(sh_s[w], sh_i[w], bs, bi)) { bs = sh_s[w]; bi = sh_i[w]; }
        __syncthreads();
        if (tid == 0) {
            top_ids[(long long)row * k + r] = bi == INT_MAX ? -1 : bi;
            top_scores[(long long)row * k + r] = bi == INT_MAX ? 0.0 : bs;
        }
        prev_s = bs; prev_i = bi;                                 // none: (0, INT_MAX), after which nothing positive comes
    }
}

// ---- depth order statistics -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_BLOCK) void vs_depth_ranks_kernel(const double* __restrict__ points, long long m, const double* __restrict__ zrow,
                                                                  const long long* __restrict__ offsets, const int* __restrict__ ids,
                                                                  long long nnz, const int* __restrict__ ranks, unsigned long long* zkey,
                                                                  double* __restrict__ out) {
    __shared__ int hist[256];
    __shared__ unsigned long long sh_prefix;
    __shared__ int sh_rank;
    const int img = blockIdx.x, tid = threadIdx.x;
    long long lo, hi;
    vs_list(offsets, img, nnz, &lo, &hi);
    const double r[4] = {zrow[4 * img + 0], zrow[4 * img + 1], zrow[4 * img + 2], zrow[4 * img + 3]};
    for (long long s = lo + tid; s < hi; s += VS_BLOCK) {
        const int p = ids[s];
        double z = NAN;
        if (p >= 0 && (long long)p < m) {
            const double x[3] = {points[3ll * p + 0], points[3ll * p + 1], points[3ll * p + 2]};
            z = vs::depth(r, x);
        }
        zkey[s] = vs::order_key(z);
    }
    __syncthreads();
    const long long c = hi - lo;
    for (int q = 0; q < 2; ++q) {
        int rank = ranks[2 * img + q];
        if (rank < 0 || (long long)rank >= c) {                   // uniform over the block
            if (tid == 0) out[2 * img + q] = NAN;
            continue;
        }
        unsigned long long prefix = 0ull;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (long long s = lo + tid; s < hi; s += VS_BLOCK) {
                const unsigned long long key = zkey[s];
                if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, d = 0;
                for (; d < 255; ++d) {
                    if (cum + hist[d] > rank) break;
                    cum += hist[d];
                }
                sh_prefix = prefix | ((unsigned long long)d << shift);
                sh_rank = rank - cum;
            }
            __syncthreads();
            prefix = sh_prefix;
            rank = sh_rank;
        }
        if (tid == 0) out[2 * img + q] = vs::key_value(prefix);
    }
}

}  // namespace rcmvs

using namespace rcmvs;

static int vs_model_ok(const char* what, int n, long long m, long long nnz) {
    RCMVS_REQUIRE(n >= 1 && n <= RCMVS_VS_MAX_IMAGES, "%s: %d images (1 .. %d)", what, n, RCMVS_VS_MAX_IMAGES);
    RCMVS_REQUIRE(m >= 1 && m < (1ll << 31), "%s: m=%lld points (1 .. 2^31-1)", what, m);
    RCMVS_REQUIRE(nnz >= 1, "%s: nnz=%lld observations (at least 1)", what, nnz);
    return 0;
}

extern "C" int rcmvs_vs_pair_scores(const double* centres, int n, const double* points, long long m, const long long* offsets, const int* ids,
                                    long long nnz, double theta0, double sigma1, double sigma2, double* scores, void* stream) {
    RCMVS_REQUIRE(centres && points && offsets && ids && scores, "vs_pair_scores: null pointer");
    if (vs_model_ok("vs_pair_scores", n, m, nnz)) return -1;
    RCMVS_REQUIRE(std::isfinite(theta0) && std::isfinite(sigma1) && std::isfinite(sigma2) && sigma1 > 0.0 && sigma2 > 0.0,
                  "vs_pair_scores: theta0 %g, sigma1 %g, sigma2 %g (finite, sigmas positive)", theta0, sigma1, sigma2);
    const int chunks = (int)cdiv(n, VS_WAVES);
    hipLaunchKernelGGL(vs_pair_scores_kernel, dim3((unsigned)((long long)n * chunks)), dim3(VS_BLOCK), 0, as_stream(stream), centres, n, points, m,
                       offsets, ids, nnz, theta0, sigma1, sigma2, chunks, scores);
    return launch_status("vs_pair_scores");
}

extern "C" int rcmvs_vs_top_views(const double* scores, int n, int k, int* top_ids, double* top_scores, int* counts, void* stream) {
    RCMVS_REQUIRE(scores && top_ids && top_scores && counts, "vs_top_views: null pointer");
    RCMVS_REQUIRE(n >= 1 && n <= RCMVS_VS_MAX_IMAGES, "vs_top_views: %d images (1 .. %d)", n, RCMVS_VS_MAX_IMAGES);
    RCMVS_REQUIRE(k >= 1 && k <= RCMVS_VS_MAX_SRC, "vs_top_views: k=%d (1 .. %d)", k, RCMVS_VS_MAX_SRC);
    hipLaunchKernelGGL(vs_top_views_kernel, dim3(n), dim3(VS_BLOCK), 0, as_stream(stream), scores, n, k, top_ids, top_scores, counts);
    return launch_status("vs_top_views");
}

extern "C" int rcmvs_vs_depth_ranks(const double* points, long long m, const double* zrow, int n, const long long* offsets, const int* ids,
                                    long long nnz, const int* ranks, unsigned long long* zkey, double* out, void* stream) {
    RCMVS_REQUIRE(points && zrow && offsets && ids && ranks && zkey && out, "vs_depth_ranks: null pointer");
    if (vs_model_ok("vs_depth_ranks", n, m, nnz)) return -1;
    hipLaunchKernelGGL(vs_depth_ranks_kernel, dim3(n), dim3(VS_BLOCK), 0, as_stream(stream), points, m, zrow, offsets, ids, nnz, ranks, zkey, out);
    return launch_status("vs_depth_ranks");
}
