// Every validation statistic of one item in one launch (train_rcmvsnet.py:449-499 test_sample_depth of the reference): the
// supervised multi-stage smooth-L1 loss (models/modules.py:527-546 cas_mvsnet_loss), the mean absolute depth error and the
// 2 / 4 / 8 mm error rates, accuracies and band-wise absolute errors (utils.py:139-159 Thres_metrics, AbsDepthError_metrics)
// of the last stage.  The reference forms them with about a dozen boolean-mask indexings per item, each a nonzero with a
// blocking read-back; here they are sums and counts over the same three (estimate, ground truth, mask) triples.
//
// One grid covers the three stages (a block belongs to one stage).  A lane reads its pixels with 16-byte loads (scalar loads
// for a tail or unaligned planes), keeps counts as integers and sums in fp64: with d = est - gt one fp32 subtraction, 0.5 d^2
// and |d| - 0.5 are exact in fp64, so only the order of the additions is left to rounding.  Wave shuffle, LDS across the
// waves, one 128-byte partial per block in the workspace, each on a cache line of its own (the ticket has one too); thread 0
// releases, draws a ticket with one atomicAdd, and the block that draws the last one acquires in every wave, adds the partials
// IN BLOCK ORDER, divides in fp64 and writes the record -- the result does not
// depend on scheduling, two runs are bit-identical.  That block also puts the ticket back to 0, so back-to-back calls on one
// stream need no memset.  The two optional images of the last stage are written in the same pass.
// 5.2 MB per item at 512 x 640: a launch-latency kernel ("Validation").  gfx950 only; plain atomics,
// shuffles and __syncthreads (tests/emu compiles this file too).
#include "common.h"

namespace rcmvs {
namespace dm {

constexpr int BLOCK = 256;
constexpr int CHUNKS = 4;                  // float4 chunks per thread: 4096 pixels per block, 105 blocks at 512 x 640
constexpr int NSUM = 7;                    // fp64 sums: sl1 of the block's stage, then (last stage) sum e, band sums [0,2] [2,4] [4,8]
constexpr int NCNT = 9;                    // counts: mask pixels of the block's stage, then (last stage) e > 2, 4, 8 and the three bands
constexpr int SLOTS = 16;                  // 8-byte words per block partial
constexpr int TILE = 128;                  // block partials the last block holds in LDS at a time (16 KB)

struct Stage { const float* est; const float* gt; const float* mask; long long n; long long chunks; int first_block; int vec; };
struct Args {
    Stage s[3];
    double w[3];
    double* record;                         // row `slot` of the table
    float* masked_depth;
    float* errormap;
    unsigned int* ticket;
    unsigned long long* partials;           // (blocks, SLOTS)
    int nblocks;
};

// slots of a partial: sums first (as doubles), counts after (as 64-bit integers)
enum { S_SL1 = 0, S_E = 3, S_BAND = 4, C_N = 7, C_GT = 10, C_BAND = 13 };

struct Acc { double sl1, e, band[3]; unsigned int n, gt[3], bc[3]; };

__device__ inline void pixel(Acc& a, float est, float gt, float mask, bool last) {
    if (!(mask > 0.5f)) return;
    const float d32 = est - gt;
    const double d = (double)d32, e = fabs(d);
    a.n += 1;
    a.sl1 += e < 1.0 ? 0.5 * d * d : e - 0.5;
    if (!last) return;
    a.e += e;
    a.gt[0] += e > 2.0; a.gt[1] += e > 4.0; a.gt[2] += e > 8.0;
    if (e >= 0.0 && e <= 2.0) { a.band[0] += e; a.bc[0] += 1; }
    if (e >= 2.0 && e <= 4.0) { a.band[1] += e; a.bc[1] += 1; }
    if (e >= 4.0 && e <= 8.0) { a.band[2] += e; a.bc[2] += 1; }
}

template <class T> __device__ inline T wave_sum(T v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// The two halves of __threadfence() at agent scope, spelled as the compiler builtins so that the host compiler of tests/emu
// takes this file as written.  release = buffer_wbl2 sc1 + s_waitcnt vmcnt(0): this thread's stores reach memory before what
// follows; acquire = buffer_inv sc1: the loads that follow IN THE SAME WAVE see other XCDs' stores (a barrier carries the
// invalidate to no other wave: every wave that reads runs its own).
__device__ inline void agent_release() { __scoped_atomic_thread_fence(__ATOMIC_RELEASE, __MEMORY_SCOPE_DEVICE); }
__device__ inline void agent_acquire() { __scoped_atomic_thread_fence(__ATOMIC_ACQUIRE, __MEMORY_SCOPE_DEVICE); }
// an agent-scope load (global_load ... sc1): served by L2, never by this CU's L1
__device__ inline unsigned long long agent_load(const unsigned long long* p) {
    return __scoped_atomic_load_n(p, __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
}

__global__ __launch_bounds__(BLOCK) void depth_metrics_kernel(const Args a) {
    __shared__ double w_sum[BLOCK / WAVE][NSUM];
    __shared__ unsigned int w_cnt[BLOCK / WAVE][NCNT];
    __shared__ double total[SLOTS];
    __shared__ unsigned long long tile[TILE * SLOTS];
    __shared__ int is_last;
    const int b = blockIdx.x;
    const int si = b >= a.s[2].first_block ? 2 : (b >= a.s[1].first_block ? 1 : 0);
    const Stage st = a.s[si];
    const bool last = si == 2;
    float* img_d = last ? a.masked_depth : nullptr;
    float* img_e = last ? a.errormap : nullptr;
    Acc acc = {};
    const long long c0 = (long long)(b - st.first_block) * (BLOCK * CHUNKS) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const long long c = c0 + (long long)k * BLOCK;                 // neighbouring lanes read neighbouring 16-byte chunks
        if (c >= st.chunks) break;
        const long long p = c * 4;
        float e4[4], g4[4], m4[4];
        const int cnt = st.n - p < 4 ? (int)(st.n - p) : 4;
        const bool vec = st.vec && cnt == 4;
        if (vec) {
            const float4 e = *reinterpret_cast<const float4*>(st.est + p), g = *reinterpret_cast<const float4*>(st.gt + p),
                         m = *reinterpret_cast<const float4*>(st.mask + p);
            e4[0] = e.x; e4[1] = e.y; e4[2] = e.z; e4[3] = e.w;
            g4[0] = g.x; g4[1] = g.y; g4[2] = g.z; g4[3] = g.w;
            m4[0] = m.x; m4[1] = m.y; m4[2] = m.z; m4[3] = m.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = j < cnt;
                e4[j] = in ? st.est[p + j] : 0.0f; g4[j] = in ? st.gt[p + j] : 0.0f; m4[j] = in ? st.mask[p + j] : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) pixel(acc, e4[j], g4[j], m4[j], last);   // a pixel past the end has mask 0
        if (img_d || img_e) {
            float od[4], oe[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { od[j] = e4[j] * m4[j]; oe[j] = fabsf(e4[j] - g4[j]) * m4[j]; }
            // the images are fresh allocations of the wrapper; an unaligned caller's buffer takes the scalar stores
            if (img_d) {
                if (vec && (reinterpret_cast<uintptr_t>(img_d) & 15) == 0) *reinterpret_cast<float4*>(img_d + p) = make_float4(od[0], od[1], od[2], od[3]);
                else for (int j = 0; j < cnt; ++j) img_d[p + j] = od[j];
            }
            if (img_e) {
                if (vec && (reinterpret_cast<uintptr_t>(img_e) & 15) == 0) *reinterpret_cast<float4*>(img_e + p) = make_float4(oe[0], oe[1], oe[2], oe[3]);
                else for (int j = 0; j < cnt; ++j) img_e[p + j] = oe[j];
            }
        }
    }
    // wave, then block
    const double s[NSUM] = {si == 0 ? acc.sl1 : 0.0, si == 1 ? acc.sl1 : 0.0, si == 2 ? acc.sl1 : 0.0, acc.e, acc.band[0], acc.band[1], acc.band[2]};
    const unsigned int n[NCNT] = {si == 0 ? acc.n : 0u, si == 1 ? acc.n : 0u, si == 2 ? acc.n : 0u, acc.gt[0], acc.gt[1], acc.gt[2],
                                  acc.bc[0], acc.bc[1], acc.bc[2]};
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        const double v = wave_sum(s[k]);
        if (lane == 0) w_sum[wave][k] = v;
    }
#pragma unroll
    for (int k = 0; k < NCNT; ++k) {
        const unsigned int v = wave_sum(n[k]);
        if (lane == 0) w_cnt[wave][k] = v;
    }
    if (threadIdx.x == 0) is_last = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        // one thread writes the partial, fences and draws the ticket: program order of a single thread
        unsigned long long* mine = a.partials + (long long)b * SLOTS;
        for (int k = 0; k < NSUM; ++k) {
            double v = 0.0;
            for (int w = 0; w < BLOCK / WAVE; ++w) v += w_sum[w][k];
            reinterpret_cast<double*>(mine)[k] = v;
        }
        for (int k = 0; k < NCNT; ++k) {
            unsigned long long v = 0;
            for (int w = 0; w < BLOCK / WAVE; ++w) v += w_cnt[w][k];
            mine[NSUM + k] = v;
        }
        agent_release();                                                 // the partial is in memory before the ticket is drawn
        const unsigned int t = atomicAdd(a.ticket, 1u);
        if (t == (unsigned int)a.nblocks - 1) {
            atomicExch(a.ticket, 0u);                                    // every ticket of this launch is drawn: ready for the next one
            is_last = 1;
        }
    }
    __syncthreads();
    if (!is_last) return;
    // The last block.  Every one of its waves reads partials, so every wave acquires for itself, after the barrier that told it
    // so; the reads are agent-scope loads on top of that.  All threads fetch a tile of partials into LDS, then 16 threads add it
    // up in block order: the same additions whatever order the blocks ran in.
    agent_acquire();
    double dsum = 0.0;
    unsigned long long csum = 0;
    for (int i0 = 0; i0 < a.nblocks; i0 += TILE) {
        const int words = (a.nblocks - i0 < TILE ? a.nblocks - i0 : TILE) * SLOTS;
        unsigned long long got[TILE * SLOTS / BLOCK];                    // all of a thread's loads in flight before the first is used
#pragma unroll
        for (int u = 0; u < TILE * SLOTS / BLOCK; ++u) {
            const int j = threadIdx.x + u * BLOCK;
            got[u] = j < words ? agent_load(a.partials + (long long)i0 * SLOTS + j) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < TILE * SLOTS / BLOCK; ++u) {
            const int j = threadIdx.x + u * BLOCK;
            if (j < words) tile[j] = got[u];
        }
        __syncthreads();
        if (threadIdx.x < SLOTS) {
            const int k = threadIdx.x;
            if (k < NSUM) for (int j = k; j < words; j += SLOTS) dsum += reinterpret_cast<const double*>(tile)[j];
            else for (int j = k; j < words; j += SLOTS) csum += tile[j];
        }
        __syncthreads();
    }
    if (threadIdx.x < SLOTS) total[threadIdx.x] = threadIdx.x < NSUM ? dsum : (double)csum;   // a count is below 2^53: exact
    __syncthreads();
    if (threadIdx.x == 0) {
        double* r = a.record;
        const double* t = total;
        double loss = 0.0;
        for (int k = 0; k < 3; ++k) loss += a.w[k] * (t[S_SL1 + k] / t[C_N + k]);       // 0 / 0 = NaN: a mean over nothing
        const double n3 = t[C_N + 2];
        r[RCMVS_DM_LOSS] = loss;
        r[RCMVS_DM_DEPTH_LOSS] = t[S_SL1 + 2] / n3;
        r[RCMVS_DM_ABS_DEPTH_ERROR] = t[S_E] / n3;
        for (int k = 0; k < 3; ++k) {
            const double err = t[C_GT + k] / n3;
            r[RCMVS_DM_THRES_ERROR + k] = err;
            r[RCMVS_DM_THRES_ACCU + k] = 1.0 - err;
            r[RCMVS_DM_THRES_ABSERROR + k] = t[C_BAND + k] > 0.0 ? t[S_BAND + k] / t[C_BAND + k] : 0.0;   // an empty band is 0, as in the reference
        }
        for (int k = 0; k < SLOTS; ++k) r[RCMVS_DM_RAW + k] = t[k];
        for (int k = RCMVS_DM_RAW + SLOTS; k < RCMVS_DM_RECORD; ++k) r[k] = 0.0;
    }
}

static int blocks_of(long long chunks) { return (int)cdiv(chunks, BLOCK * CHUNKS); }

}  // namespace dm
}  // namespace rcmvs

using namespace rcmvs;

extern "C" long long rcmvs_depth_metrics_workspace_bytes(long long n1, long long n2, long long n3) {
    if (n1 <= 0 || n2 <= 0 || n3 <= 0) return -1;
    const long long blocks = dm::blocks_of(cdiv(n1, 4)) + dm::blocks_of(cdiv(n2, 4)) + dm::blocks_of(cdiv(n3, 4));
    return 128 + blocks * dm::SLOTS * 8;               // the ticket's own 128-byte line, then one line per block
}

extern "C" int rcmvs_depth_metrics_timed(const float* est1, const float* gt1, const float* mask1, long long n1,
                                         const float* est2, const float* gt2, const float* mask2, long long n2,
                                         const float* est3, const float* gt3, const float* mask3, long long n3,
                                         const double* dlossw_host, double* table, int slot, float* masked_depth, float* errormap,
                                         void* workspace, void* ev_start, void* ev_stop, void* stream) {
    RCMVS_REQUIRE(est1 && gt1 && mask1 && est2 && gt2 && mask2 && est3 && gt3 && mask3 && table && workspace, "depth_metrics: null pointer");
    RCMVS_REQUIRE(n1 > 0 && n2 > 0 && n3 > 0 && n1 < (1ll << 31) && n2 < (1ll << 31) && n3 < (1ll << 31),
                  "depth_metrics: stage sizes %lld, %lld, %lld are outside 1 .. 2^31 - 1", n1, n2, n3);
    RCMVS_REQUIRE(slot >= 0, "depth_metrics: slot %d is negative", slot);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 127) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0,
                  "depth_metrics: the workspace must be 128-byte aligned and the table 8-byte aligned");
    dm::Args a;
    const float* ptr[3][3] = {{est1, gt1, mask1}, {est2, gt2, mask2}, {est3, gt3, mask3}};
    const long long n[3] = {n1, n2, n3};
    int blocks = 0;
    for (int k = 0; k < 3; ++k) {
        dm::Stage& s = a.s[k];
        s.est = ptr[k][0]; s.gt = ptr[k][1]; s.mask = ptr[k][2];
        s.n = n[k];
        s.chunks = cdiv(n[k], 4);
        s.first_block = blocks;
        s.vec = ((reinterpret_cast<uintptr_t>(s.est) | reinterpret_cast<uintptr_t>(s.gt) | reinterpret_cast<uintptr_t>(s.mask)) & 15) == 0;
        blocks += dm::blocks_of(s.chunks);
        a.w[k] = dlossw_host ? dlossw_host[k] : 1.0;
    }
    a.record = table + (long long)slot * RCMVS_DM_RECORD;
    a.masked_depth = masked_depth;
    a.errormap = errormap;
    a.ticket = static_cast<unsigned int*>(workspace);
    a.partials = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + 128);
    a.nblocks = blocks;
    RCMVS_LAUNCH_TIMED(dm::depth_metrics_kernel, dim3((unsigned)blocks), dim3(dm::BLOCK), 0, as_stream(stream),
                       static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop), a);
    return launch_status("depth_metrics");
}

extern "C" int rcmvs_depth_metrics(const float* est1, const float* gt1, const float* mask1, long long n1,
                                   const float* est2, const float* gt2, const float* mask2, long long n2,
                                   const float* est3, const float* gt3, const float* mask3, long long n3,
                                   const double* dlossw_host, double* table, int slot, float* masked_depth, float* errormap,
                                   void* workspace, void* stream) {
    return rcmvs_depth_metrics_timed(est1, gt1, mask1, n1, est2, gt2, mask2, n2, est3, gt3, mask3, n3, dlossw_host, table, slot,
                                     masked_depth, errormap, workspace, nullptr, nullptr, stream);
}
