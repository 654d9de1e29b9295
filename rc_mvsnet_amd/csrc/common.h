// Shared helpers for librcmvs_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdarg>
#include "../../include/rcmvs.h"

namespace rcmvs {

constexpr int WAVE = 64;

// thread-local last-error text (rcmvs_last_error_string)
char* err_buf();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// check the launch that was just enqueued (no sync): >0 = hipError_t
inline int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, "%s: %s", what, hipGetErrorString(e));
    return 0;
}

// A launch whose start / stop timestamps go to two caller-owned events (hipExtLaunchKernelGGL: the dispatch's own timestamps, what rocprofv3 reports as
// the kernel's duration -- event records around a launch add the marker packets' ~2-3 us each); both events NULL = a plain launch.
#define RCMVS_LAUNCH_TIMED(kernel, grid, block, lds, st, ev0, ev1, ...) do { \
        if ((ev0) || (ev1)) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev0, ev1, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__); } while (0)

#define RCMVS_REQUIRE(cond, ...) do { if (!(cond)) return ::rcmvs::fail(-1, __VA_ARGS__); } while (0)

__host__ __device__ inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// XCD-aware remap of a 1-D block id (blocks are dispatched round-robin over the 8 XCDs,
// MI355X_MICROARCH "Workgroup dispatch"): gives each XCD a contiguous chunk of the logical
// tile order so neighbouring tiles share that XCD's L2.  Bijective for any grid size.
__device__ inline unsigned xcd_remap(unsigned bid, unsigned nblk) {
    constexpr unsigned NX = 8;
    unsigned xcd = bid % NX, idx = bid / NX;
    unsigned q = nblk / NX, r = nblk % NX;
    unsigned base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// ---- layer-output stores -----------------------------------------------------------------------------------------------------------
// Every 16-byte store of a layer's output goes through out_store16: one buffer store whose cache policy is a compile-time constant
// (the aux bits of the gfx950 buffer instructions).  A plain, sc0 or nt store leaves its line dirty in the XCD's L2, and the dirty
// lines are written back serially when the kernel ends, before the dependent launch may start; an sc1 store writes through and
// drops the line.  The next kernel never finds a predecessor's line in its own L2 anyway (visibility across XCDs needs write-back plus
// invalidate), so write-through costs the consumer nothing.
//   RCMVS_OUT_POLICY          the default of every family
//   RCMVS_OUT_POLICY_<FAMILY> one family's own choice (K1, Z8, ZS2, X3, DEEP, CONV2D, STEM, PAIR, TILE, FPN, LAYOUT)
// Narrow stores (the 4-byte logits of prob_pair / conv11_prob, the depth head's depth and confidence, the float2 plane table) and the
// activation-bound atomics stay plain: a per-lane dword sc1 store is one fabric write each, about 6x the dwordx4 time per byte.
#define RCMVS_ST_PLAIN 0
#define RCMVS_ST_NT 2
#define RCMVS_ST_SC1 16
#define RCMVS_ST_SC1_NT 18
#ifndef RCMVS_OUT_POLICY
#define RCMVS_OUT_POLICY RCMVS_ST_SC1
#endif
// (K1 keeps nt: its three launches took 124 us per scene with nt, 138 with sc1 and 138 with sc1 | nt -- profiles/store_policy.txt)
#ifndef RCMVS_OUT_POLICY_K1
#define RCMVS_OUT_POLICY_K1 RCMVS_ST_NT
#endif
#ifndef RCMVS_OUT_POLICY_Z8
#define RCMVS_OUT_POLICY_Z8 RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_ZS2
#define RCMVS_OUT_POLICY_ZS2 RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_X3
#define RCMVS_OUT_POLICY_X3 RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_DEEP
#define RCMVS_OUT_POLICY_DEEP RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_CONV2D
#define RCMVS_OUT_POLICY_CONV2D RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_STEM
#define RCMVS_OUT_POLICY_STEM RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_PAIR
#define RCMVS_OUT_POLICY_PAIR RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_TILE
#define RCMVS_OUT_POLICY_TILE RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_FPN
#define RCMVS_OUT_POLICY_FPN RCMVS_OUT_POLICY
#endif
#ifndef RCMVS_OUT_POLICY_LAYOUT
#define RCMVS_OUT_POLICY_LAYOUT RCMVS_OUT_POLICY
#endif

constexpr int OUT_OOB = 0x7ffffff0;                    // the offset of a masked lane: outside every span, the store is dropped
constexpr long long OUT_SPAN_MAX = 0x7ffffff0LL;       // a descriptor's span stays below this (launchers: out_span_ok)

// descriptor of an output span: `base` must be wave-uniform (anything 64-bit of the address goes here), `bytes` < 2^31
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(float* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
}

// v: any 16-byte value (float4, a 4-vector of float or unsigned); off: byte offset inside the span, OUT_OOB for a masked lane
template <int POLICY, class T>
__device__ __forceinline__ void out_store16(const T& v, __amdgpu_buffer_rsrc_t rs, int off) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    static_assert(sizeof(T) == 16, "out_store16 stores 16 bytes per lane");
    static_assert(POLICY == RCMVS_ST_PLAIN || POLICY == RCMVS_ST_NT || POLICY == RCMVS_ST_SC1 || POLICY == RCMVS_ST_SC1_NT, "unknown store policy");
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, off, 0, POLICY);
}

// a value the compiler cannot prove wave-uniform, made so (it is uniform: the caller's claim)
__device__ __forceinline__ long long uniform_ll(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// launcher side: a span of `bytes` fits one descriptor
inline bool out_span_ok(long long bytes) { return bytes > 0 && bytes < OUT_SPAN_MAX; }

}  // namespace rcmvs
