// The colour-mapped depth image of the reference's Tanks-and-Temples evaluation (eval_rcmvsnet_tanks.py:141-154 write_depth_img_2):
// vmin = depth.min(), vmax = np.percentile(depth, 95), Normalize(vmin, vmax), magma_r, truncation to 8 bits -- on the device, with
// no host read between the phases.  On the host this is numpy's partition plus a float64 RGBA array from matplotlib, tens of
// milliseconds for a 1056 x 1920 map; here it is three counting passes and one colouring pass over the map.
//
// The percentile is exact: numpy's linear method needs the order statistics of ranks lo = floor((n - 1) q) and lo + 1, found by a
// radix select over an order-preserving integer key of the fp32 bits, digits of 11, 11 and 10 bits.  A counting pass keeps one
// histogram per wanted rank in LDS (one, while both ranks still share their prefix), fed by per-thread runs of equal digits (a
// depth map's leading bits hardly change, so most LDS atomics would otherwise hit one counter), and adds each non-empty bin to the
// global histogram of that pass with one atomic.  Every block of the NEXT launch scans that histogram for the bin holding each rank
// (2048 counters from L2, against 32 KB of pixels per block) -- so no launch waits on a last block and there is no ticket; block 0
// also leaves the chosen prefix and the rank within it in a device word for the launch after.  The first pass takes the minimum
// (as the maximum of the inverted key) and flags a NaN, for which numpy's percentile and minimum are both NaN.  The colouring pass
// resolves the last digit, interpolates vmax as numpy does, writes (vmin, vmax, NaN flag) and maps every pixel through the
// 256-entry table held in LDS.  Counting is integer work and the arithmetic is csrc/depth_colormap_math.h under contraction off,
// in the precision numpy and matplotlib evaluate each step in: two runs are bit-identical and the image equals the reference's byte for byte (tests/golden/tanks_eval.npz).
// The workspace is cleared at the start of every call (one memset node), so a lost launch leaves nothing behind.
// gfx950 only; plain atomics, shuffles and __syncthreads (tests/emu compiles this file too).
#include "common.h"
#include "depth_colormap_math.h"

#pragma clang fp contract(off)

namespace rcmvs {
namespace dcm {

constexpr int BLOCK = 256;
constexpr int CHUNKS = 8;                       // float4 chunks per thread: 8192 pixels per block, 248 blocks at 1056 x 1920
constexpr int PASSES = 3;
constexpr int BINS = 2048;                      // counters per histogram (the last pass uses 1024 of them)
constexpr int BAD = 256;                        // table entry of a NaN: (0, 0, 0)

__host__ __device__ inline int pass_shift(int p) { return p == 0 ? 21 : (p == 1 ? 10 : 0); }
__host__ __device__ inline int pass_bins(int p) { return p == 2 ? 1024 : 2048; }

// the workspace, as 32-bit words
enum { W_NOTMIN = 0, W_NAN = 1, W_STATE = 4, W_HIST = 16, W_WORDS = W_HIST + PASSES * 2 * BINS };
// state of pass p (p = 1, 2) at W_STATE + 4 (p - 1): prefix of rank lo, its rank within the prefix, the same two for rank hi

struct Sel { unsigned int prefix[2], k[2]; };

// Which bin of hist (nb counters, global memory, complete: written by the previous launch) holds the value of rank k among the
// counted ones, and k's rank inside that bin.  Called by the whole block; `out` and `wtot` are LDS.
__device__ inline void find_bin(const unsigned int* hist, int nb, unsigned int k, unsigned int* out, unsigned int* wtot) {
    const int per = nb / BLOCK, t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    unsigned int c[BINS / BLOCK], s = 0;
    for (int j = 0; j < per; ++j) { c[j] = hist[t * per + j]; s += c[j]; }
    unsigned int incl = s;
    for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == WAVE - 1) wtot[wave] = incl;
    __syncthreads();
    unsigned int excl = incl - s;
    for (int w = 0; w < wave; ++w) excl += wtot[w];
    if (k >= excl && k - excl < s) {                                  // exactly one thread: the bins partition the counted values
        unsigned int below = excl;
        for (int j = 0; j < per; ++j) {
            if (k - below < c[j]) { out[0] = (unsigned int)(t * per + j); out[1] = k - below; break; }
            below += c[j];
        }
    }
    __syncthreads();
}

// The selection state a launch starts from: pass 0 counts everything; pass p > 0 extends the state of pass p - 1 by the digit
// found in that pass's histograms.  Every block computes the same thing; block 0 stores it for the launch after this one.
__device__ inline Sel advance(unsigned int* ws, int p, unsigned int lo, unsigned int hi, unsigned int* lds) {
    Sel s;
    if (p == 0) { s.prefix[0] = s.prefix[1] = 0; s.k[0] = lo; s.k[1] = hi; return s; }
    Sel prev;
    if (p == 1) { prev.prefix[0] = prev.prefix[1] = 0; prev.k[0] = lo; prev.k[1] = hi; }
    else { const unsigned int* st = ws + W_STATE + 4 * (p - 2); prev.prefix[0] = st[0]; prev.k[0] = st[1]; prev.prefix[1] = st[2]; prev.k[1] = st[3]; }
    const bool same = prev.prefix[0] == prev.prefix[1];                // then the pass kept one histogram for both ranks
    const int nb = pass_bins(p - 1), bits = nb == 2048 ? 11 : 10;
    for (int r = 0; r < 2; ++r) {
        const unsigned int* hist = ws + W_HIST + ((p - 1) * 2 + (same ? 0 : r)) * BINS;
        find_bin(hist, nb, prev.k[r], lds + 2 * r, lds + 4);
    }
    for (int r = 0; r < 2; ++r) { s.prefix[r] = (prev.prefix[r] << bits) | lds[2 * r]; s.k[r] = lds[2 * r + 1]; }
    __syncthreads();                                                   // lds is free again
    if (p < PASSES && blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned int* st = ws + W_STATE + 4 * (p - 1);
        st[0] = s.prefix[0]; st[1] = s.k[0]; st[2] = s.prefix[1]; st[3] = s.k[1];
    }
    return s;
}

// the 4 values of chunk c (fewer at the end of the map): -> how many
__device__ inline int load_chunk(const float* depth, long long n, int vec, long long c, float v[4]) {
    const long long p = c * 4;
    const int cnt = n - p < 4 ? (int)(n - p) : 4;
    if (vec && cnt == 4) {
        const float4 q = *reinterpret_cast<const float4*>(depth + p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? depth[p + j] : 0.0f;
    }
    return cnt;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const float* depth, long long n, int vec, unsigned int* ws, int p,
                                                      unsigned int lo, unsigned int hi) {
    __shared__ unsigned int h[2][BINS];
    __shared__ unsigned int sel[8];
    __shared__ unsigned int red[2][BLOCK / WAVE];
    for (int i = threadIdx.x; i < 2 * BINS; i += BLOCK) (&h[0][0])[i] = 0;
    const Sel s = advance(ws, p, lo, hi, sel);                         // its barriers also cover the zero-fill
    if (p == 0) __syncthreads();
    const bool same = s.prefix[0] == s.prefix[1];
    const int shift = pass_shift(p), nb = pass_bins(p);
    const int nr = same ? 1 : 2;
    unsigned int cur[2] = {0xffffffffu, 0xffffffffu}, run[2] = {0, 0};
    unsigned int notmin = 0, nan = 0;
    const long long chunks = cdiv(n, 4);
    const long long c0 = (long long)blockIdx.x * (BLOCK * CHUNKS) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const long long c = c0 + (long long)k * BLOCK;                 // neighbouring lanes read neighbouring 16-byte chunks
        if (c >= chunks) break;
        float v[4];
        const int cnt = load_chunk(depth, n, vec, c, v);
        for (int j = 0; j < cnt; ++j) {
            const unsigned int key = order_key(v[j]);
            if (p == 0) {
                nan |= v[j] != v[j];
                const unsigned int inv = ~key;
                notmin = inv > notmin ? inv : notmin;
            }
            const unsigned int digit = (key >> shift) & (unsigned int)(nb - 1);
            const unsigned int top = p == 0 ? 0u : key >> (shift + (nb == 2048 ? 11 : 10));
            for (int r = 0; r < nr; ++r) {
                if (top != s.prefix[r]) continue;
                if (digit == cur[r]) { run[r] += 1; continue; }
                if (run[r]) atomicAdd(&h[r][cur[r]], run[r]);
                cur[r] = digit; run[r] = 1;
            }
        }
    }
    for (int r = 0; r < nr; ++r) if (run[r]) atomicAdd(&h[r][cur[r]], run[r]);
    if (p == 0) {
        const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const unsigned int o = __shfl_down(notmin, off), f = __shfl_down(nan, off);
            notmin = o > notmin ? o : notmin;
            nan |= f;
        }
        if (lane == 0) { red[0][wave] = notmin; red[1][wave] = nan; }
    }
    __syncthreads();
    unsigned int* g = ws + W_HIST + p * 2 * BINS;
    for (int i = threadIdx.x; i < nr * BINS; i += BLOCK) {
        const unsigned int v = (&h[0][0])[i];
        if (v) atomicAdd(g + i, v);                                    // one global add per block and non-empty bin
    }
    if (p == 0 && threadIdx.x == 0) {
        unsigned int m = 0, f = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) { m = red[0][w] > m ? red[0][w] : m; f |= red[1][w]; }
        atomicMax(ws + W_NOTMIN, m);
        if (f) atomicMax(ws + W_NAN, 1u);
    }
}

__global__ __launch_bounds__(BLOCK) void colour_kernel(const float* depth, long long n, int vec, unsigned int* ws, unsigned int lo,
                                                       unsigned int hi, float g, const unsigned char* lut, unsigned char* rgb, float* stats) {
    __shared__ unsigned int sel[8];
    __shared__ unsigned char table[(BAD + 1) * 3 + 1];
    for (int i = threadIdx.x; i < (BAD + 1) * 3; i += BLOCK) table[i] = i < BAD * 3 ? lut[i] : (unsigned char)0;
    const Sel s = advance(ws, PASSES, lo, hi, sel);                    // after the last digit the prefix IS the key
    float vmin = key_value(~ws[W_NOTMIN]);
    float vmax = lerp(key_value(s.prefix[0]), key_value(s.prefix[1]), g);
    const bool nan = ws[W_NAN] != 0;
    if (nan) vmin = vmax = bits_float(0x7fc00000u);
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = vmin; stats[1] = vmax; stats[2] = nan ? 1.0f : 0.0f; stats[3] = 0.0f; }
    const long long chunks = cdiv(n, 4);
    const long long c0 = (long long)blockIdx.x * (BLOCK * CHUNKS) + threadIdx.x;
    const bool out4 = (reinterpret_cast<uintptr_t>(rgb) & 3) == 0;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const long long c = c0 + (long long)k * BLOCK;
        if (c >= chunks) break;
        float v[4];
        const int cnt = load_chunk(depth, n, vec, c, v);
        unsigned char b[12];
        for (int j = 0; j < 4; ++j) {
            const int idx = j < cnt ? colour_index(v[j], vmin, vmax) : BAD;
            b[3 * j] = table[3 * idx]; b[3 * j + 1] = table[3 * idx + 1]; b[3 * j + 2] = table[3 * idx + 2];
        }
        unsigned char* o = rgb + c * 12;
        if (cnt == 4 && out4) {                                        // 12 bytes at a multiple of 12 from a 4-byte aligned base
            unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
            for (int q = 0; q < 3; ++q)
                o4[q] = (unsigned int)b[4 * q] | ((unsigned int)b[4 * q + 1] << 8) | ((unsigned int)b[4 * q + 2] << 16) | ((unsigned int)b[4 * q + 3] << 24);
        } else {
            for (int j = 0; j < 3 * cnt; ++j) o[j] = b[j];
        }
    }
}

}  // namespace dcm
}  // namespace rcmvs

using namespace rcmvs;

extern "C" long long rcmvs_depth_colormap_workspace_bytes(void) { return (long long)dcm::W_WORDS * 4; }

extern "C" int rcmvs_depth_colormap(const float* depth, int H, int W, double percentile, const unsigned char* lut, unsigned char* rgb,
                                    float* stats, void* workspace, void* stream) {
    RCMVS_REQUIRE(depth && lut && rgb && stats && workspace, "depth_colormap: null pointer");
    RCMVS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "depth_colormap: bad dims H=%d W=%d (each >= 1, H * W < 2^31)", H, W);
    RCMVS_REQUIRE(percentile >= 0.0 && percentile <= 100.0, "depth_colormap: percentile %g is outside [0, 100]", percentile);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(depth) & 3) == 0, "depth_colormap: depth / stats must be 4-byte and the workspace 16-byte aligned");
    const long long n = (long long)H * W;
    const dcm::Rank r = dcm::percentile_rank(n, percentile);
    const int vec = (reinterpret_cast<uintptr_t>(depth) & 15) == 0;
    const unsigned blocks = (unsigned)cdiv(cdiv(n, 4), dcm::BLOCK * dcm::CHUNKS);
    hipStream_t st = as_stream(stream);
    unsigned int* ws = static_cast<unsigned int*>(workspace);
    const hipError_t e = hipMemsetAsync(ws, 0, (size_t)dcm::W_WORDS * 4, st);
    if (e != hipSuccess) return fail((int)e, "depth_colormap: %s", hipGetErrorString(e));
    for (int p = 0; p < dcm::PASSES; ++p) {
        hipLaunchKernelGGL(dcm::count_kernel, dim3(blocks), dim3(dcm::BLOCK), 0, st, depth, n, vec, ws, p, r.lo, r.hi);
        const int rc = launch_status("depth_colormap (count)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(dcm::colour_kernel, dim3(blocks), dim3(dcm::BLOCK), 0, st, depth, n, vec, ws, r.lo, r.hi, r.g, lut, rgb, stats);
    return launch_status("depth_colormap (colour)");
}
