// Simplification of a triangle mesh by quadric edge collapse, one independent set of edges a round (rc_mvsnet_amd/mesh_simplify.py;
// contract in mesh_simplify.h, the per-element rules in mesh_simplify_math.h, the rule and its proof in DESIGN.md).
//
//   init       the corners of every vertex by a stable sort of (vertex, corner) pairs (scan_sort.hip's radix pass), then one lane per
//              vertex adds its corners' plane quadrics in fp64 in ascending corner order; members, colour sums, the live faces.
//   round      topology    mesh_clean.hip's sorted 1-ring with multiplicities, the corner sort again, the locked vertices;
//              candidates  one lane per CSR entry u -> v, u < v: target, cost, the three rejections, the key at the entry and at
//                          its mirror v -> u (found by bisection in v's sorted ring), so that every entry has exactly one writer;
//              selection   one lane per vertex takes the smallest key of its segment, then the smallest over its closed ring; an
//                          edge is selected when it is that minimum at both ends; scan3 of the flags cuts the set at the budget;
//              apply       one lane per applied edge writes the survivor in place (no two applied edges share a vertex or a
//                          neighbour), one thread per face takes its indices through remap and counts the live faces.
//   finish     flags and ranks of the valid faces and the vertices they use, for mesh_clean's gather; colours from the sums.
// No thread waits for another workgroup and there are no floating-point atomics.  gfx950 only; __syncthreads, plain loads and
// stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_clean.h"                                           // rcmvs_mc_adjacency_timed
#include "mesh_simplify.h"
#include "mesh_simplify_math.h"
#include "scan_sort.h"                                            // gid, blocks, scan3, radix_sort, segments_kernel, zero_kernel
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MS_BLOCK = TM_BLOCK;
static_assert(MS_BLOCK == RCMVS_MS_SORT_BLOCK && MS_BLOCK == SS_BLOCK, "a sort block is one workgroup's threads");
static_assert(RCMVS_MS_SCAN_TILE == SS_TILE && RCMVS_MS_SCAN_WORK == SS_WORK, "mesh_simplify.h describes scan_sort.h's work area");
static_assert(ms::QUADRIC_DOUBLES == RCMVS_MS_QUADRIC_DOUBLES && ms::PATH_END_V == RCMVS_MS_PATH_END_V && ms::EDGE_FLIP == RCMVS_MS_EDGE_FLIP &&
              ms::EDGE_NONE == RCMVS_MS_EDGE_NONE && RCMVS_MS_COUNT_PATH + ms::PATHS == RCMVS_MS_COUNT_SELECTED, "the constants of mesh_simplify.h");

using u64 = unsigned long long;

struct MsFrame {
    double ctr[3];
    double side;
};

// every lane adds one to at most one of the counters first .. first + count - 1 (what; anything else: none)
__device__ inline void ms_count(int what, int first, int count, u64* counts, unsigned* sh) {
    for (int k = first; k < first + count; ++k) {
        const unsigned s = tm_block_sum(what == k ? 1u : 0u, sh);
        if (threadIdx.x == 0 && s) atomicAdd(&counts[k], (u64)s);
    }
}

__device__ inline void ms_local(const float* verts, int v, const MsFrame& F, double* p) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = md::local(verts[3 * (size_t)v + a], F.ctr[a], F.side);
}

__device__ inline bool ms_finite(const float* verts, int v) { return md::finite3(verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]); }

__device__ inline ms::Quadric ms_load(const double* quad, int v) {
    ms::Quadric Q;
    const double* q = quad + (size_t)ms::QUADRIC_DOUBLES * v;
#pragma unroll
    for (int j = 0; j < 6; ++j) Q.a[j] = q[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) Q.b[j] = q[6 + j];
    Q.c = q[9];
    return Q;
}

__device__ inline void ms_store(double* quad, int v, const ms::Quadric& Q) {
    double* q = quad + (size_t)ms::QUADRIC_DOUBLES * v;
#pragma unroll
    for (int j = 0; j < 6; ++j) q[j] = Q.a[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[6 + j] = Q.b[j];
    q[9] = Q.c;
}

// ---- incidence ------------------------------------------------------------------------------------------------------------------
// the keys of a face's three corners: the vertex, or the sentinel nv for an invalid face; the faces by kind
__global__ __launch_bounds__(MS_BLOCK) void ms_corner_key_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf,
                                                                 unsigned* __restrict__ key, int* __restrict__ idx, u64* stats) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long f = gid();
    int what = -1;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const bool ok = mc::face_valid(a, b, c, nv);
        key[3 * f] = ok ? (unsigned)a : (unsigned)nv;
        key[3 * f + 1] = ok ? (unsigned)b : (unsigned)nv;
        key[3 * f + 2] = ok ? (unsigned)c : (unsigned)nv;
        idx[3 * f] = (int)(3 * f);
        idx[3 * f + 1] = (int)(3 * f + 1);
        idx[3 * f + 2] = (int)(3 * f + 2);
        if (ok && stats) what = (ms_finite(verts, a) && ms_finite(verts, b) && ms_finite(verts, c)) ? 2 : 0;
    }
    if (stats) {                                                  // uniform over the launch
        const unsigned bad = tm_block_sum(what == 0 ? 1u : 0u, sh), valid = tm_block_sum(what >= 0 ? 1u : 0u, sh);
        if (threadIdx.x == 0 && bad) atomicAdd(&stats[0], (u64)bad);
        if (threadIdx.x == 0 && valid) atomicAdd(&stats[2], (u64)valid);
    }
}

// seg[2 v], seg[2 v + 1] and *idx (one of the two index buffers) describe every vertex's corners, ascending
static void ms_incidence(const float* verts, const int* faces, int nv, int nf, unsigned* key_a, int** idx_a, unsigned* key_b, int* idx_b, int* hist,
                         int* hist_start, int* scan_work, int* seg, u64* stats, hipStream_t st, hipEvent_t e1) {
    const long long n = 3ll * nf;
    hipEvent_t none = nullptr;
    hipLaunchKernelGGL(zero_kernel<int>, dim3(blocks(2ll * nv)), dim3(MS_BLOCK), 0, st, seg, 2ll * nv);
    hipLaunchKernelGGL(ms_corner_key_kernel, dim3(blocks(nf)), dim3(MS_BLOCK), 0, st, verts, faces, nv, nf, key_a, *idx_a, stats);
    radix_sort<unsigned>(&key_a, idx_a, &key_b, &idx_b, n, radix_passes((u64)nv), hist, hist_start, scan_work, st);      // the sentinel nv is the largest key
    RCMVS_LAUNCH_TIMED(segments_kernel, dim3(blocks(n)), dim3(MS_BLOCK), 0, st, none, e1, key_a, n, nv, seg);
}

// ---- init -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_init_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const unsigned char* __restrict__ rgb,
                                                           int nv, long long n, MsFrame F, const int* __restrict__ idx, const int* __restrict__ seg,
                                                           double* __restrict__ quad, int* __restrict__ members, u64* __restrict__ csum, u64* live, u64* stats) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long v = gid();
    unsigned bad = 0;
    if (v == 0) live[0] = stats[2];
    if (v < nv) {
        bad = ms_finite(verts, (int)v) ? 0u : 1u;
        long long i0 = seg[2 * v], i1 = seg[2 * v + 1];
        if (i0 < 0) i0 = 0;
        if (i1 > n) i1 = n;
        ms::Quadric Q = ms::zero();
        for (long long i = i0; i < i1; ++i) {
            const int e = idx[i];
            if ((unsigned)e >= (unsigned)n) continue;
            const int f = e / 3, k = e - 3 * f;
            const int w[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
            if (!mc::face_valid(w[0], w[1], w[2], nv) || (k == 0 ? w[0] : (k == 1 ? w[1] : w[2])) != (int)v) continue;
            if (!(ms_finite(verts, w[0]) && ms_finite(verts, w[1]) && ms_finite(verts, w[2]))) continue;
            double q0[3], q1[3], q2[3];
            ms_local(verts, w[0], F, q0);
            ms_local(verts, w[1], F, q1);
            ms_local(verts, w[2], F, q2);
            ms::add_corner(Q, q0, q1, q2);
        }
        ms_store(quad, (int)v, Q);
        members[v] = 1;
        if (csum) {
#pragma unroll
            for (int a = 0; a < 3; ++a) csum[3 * v + a] = rgb[3 * v + a];
        }
    }
    const unsigned s = tm_block_sum(bad, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&stats[1], (u64)s);
}

// ---- topology ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_begin_kernel(int* __restrict__ remap, int nv, const u64* __restrict__ live, u64* __restrict__ counts) {
    const long long v = gid();
    if (v < nv) remap[v] = (int)v;
    if (v < RCMVS_MS_COUNTS) counts[v] = v == RCMVS_MS_COUNT_LIVE_BEFORE ? live[0] : 0;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_lock_kernel(const float* __restrict__ verts, int nv, long long entries, const int* __restrict__ row_start,
                                                           const int* __restrict__ row_len, const int* __restrict__ mult, unsigned char* __restrict__ locked,
                                                           u64* counts) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long v = gid();
    unsigned lock = 0;
    if (v < nv) {
        lock = ms_finite(verts, (int)v) ? 0u : 1u;
        const long long i0 = row_start[v], i1 = i0 + row_len[v];
        for (long long i = i0 < 0 ? 0 : i0; i < i1 && i < entries; ++i)
            if (mult[i] != 2) lock = 1;
        locked[v] = (unsigned char)lock;
    }
    const unsigned s = tm_block_sum(lock, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&counts[RCMVS_MS_COUNT_LOCKED], (u64)s);
}

// ---- candidates -------------------------------------------------------------------------------------------------------------------
// the row of entry i: the largest u with row_start[u] <= i, for 0 <= i < row_start[nv] (bisection; empty rows are passed over)
__device__ inline int ms_owner(const int* __restrict__ row_start, int nv, long long i) {
    int lo = 0, hi = nv;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (row_start[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the ring of w as a pointer and a length inside nbr, or a length of 0
__device__ inline const int* ms_ring(const int* __restrict__ row_start, const int* __restrict__ row_len, const int* __restrict__ nbr, long long entries, int w,
                                     int* len) {
    const long long i0 = row_start[w], l = row_len[w];
    *len = (i0 >= 0 && l >= 0 && i0 + l <= entries) ? (int)l : 0;
    return nbr + (*len ? i0 : 0);
}

struct MsEdge {
    int path, from;
    unsigned t[3];                                                // the target's fp32 bits
    double xt[3];                                                 // the target in the frame
    double cost;
    ms::Quadric Q;
};

// the target, the summed quadric and the cost of the edge {u < v}: ms::place, one rounding to fp32 or an endpoint's bits
__device__ inline void ms_edge(const float* verts, const double* quad, const MsFrame& F, int u, int v, bool locked_u, bool locked_v, MsEdge* E) {
    double pu[3], pv[3], x[3] = {0.0, 0.0, 0.0};
    ms_local(verts, u, F, pu);
    ms_local(verts, v, F, pv);
    E->Q = ms::add(ms_load(quad, u), ms_load(quad, v));
    E->path = ms::place(E->Q, pu, pv, locked_u, locked_v, x, &E->from);
    if (E->from == ms::FROM_X) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float w = md::world(F.ctr[a], F.side, x[a]);
            E->t[a] = __builtin_bit_cast(unsigned, w);
            E->xt[a] = md::local(w, F.ctr[a], F.side);
        }
    } else {
        const int src = E->from == ms::FROM_U ? u : v;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            E->t[a] = reinterpret_cast<const unsigned*>(verts)[3 * (size_t)src + a];
            E->xt[a] = E->from == ms::FROM_U ? pu[a] : pv[a];
        }
    }
    E->cost = ms::cost(E->Q, E->xt);
}

// every face at w that does not hold `other` keeps its side when w moves to xt
__device__ inline bool ms_keeps_sides(const float* verts, const int* __restrict__ faces, int nv, long long n, const int* __restrict__ idx,
                                      const int* __restrict__ seg, const MsFrame& F, int w, int other, const double* xt) {
    long long i0 = seg[2 * (size_t)w], i1 = seg[2 * (size_t)w + 1];
    if (i0 < 0) i0 = 0;
    if (i1 > n) i1 = n;
    for (long long i = i0; i < i1; ++i) {
        const int e = idx[i];
        if ((unsigned)e >= (unsigned)n) continue;
        const int f = e / 3, k = e - 3 * f;
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (!mc::face_valid(a, b, c, nv) || (k == 0 ? a : (k == 1 ? b : c)) != w) continue;
        if (a == other || b == other || c == other) continue;
        double q0[3], q1[3], q2[3];
        ms_local(verts, a, F, q0);
        ms_local(verts, b, F, q1);
        ms_local(verts, c, F, q2);
        if (!ms::keeps_side(q0, q1, q2, k, xt)) return false;
    }
    return true;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_candidate_kernel(const float* verts, const int* __restrict__ faces, int nv, long long n, long long entries,
                                                                MsFrame F, const double* quad, double max_error, const int* __restrict__ row_start,
                                                                const int* __restrict__ row_len, const int* __restrict__ nbr, const int* __restrict__ mult,
                                                                const int* __restrict__ idx, const int* __restrict__ seg, const unsigned char* __restrict__ locked,
                                                                unsigned char* __restrict__ edge, u64* key, u64* counts) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long i = gid();
    int state = ms::EDGE_NONE, path = -1;
    if (i < entries) {
        bool mine = true;                                         // this lane writes key[i]: not the entry of an edge v -> u, u < v
        long long mirror = -1;
        u64 k = ms::NO_KEY;
        const long long used = nv > 0 ? row_start[nv] : 0;
        if (i < used) {
            const int u = ms_owner(row_start, nv, i);
            const long long j = i - row_start[u];
            const int v = j < row_len[u] ? nbr[i] : -1;
            if ((unsigned)v < (unsigned)nv && v != u) {
                int lu, lv;
                const int* ru = ms_ring(row_start, row_len, nbr, entries, u, &lu);
                const int* rv = ms_ring(row_start, row_len, nbr, entries, v, &lv);
                int lo = 0, hi = lv;                              // where u stands in v's ring: the entry v -> u
                while (lo < hi) {
                    const int mid = lo + (hi - lo) / 2;
                    if (rv[mid] < u) lo = mid + 1;
                    else hi = mid;
                }
                const bool found = lo < lv && rv[lo] == u;
                if (u > v) mine = !found;                         // the lane of v -> u writes here
                else if (found) mirror = (long long)row_start[v] + lo;
                if (u < v && mult[i] == 2 && !(locked[u] && locked[v])) {
                    MsEdge E;
                    ms_edge(verts, quad, F, u, v, locked[u] != 0, locked[v] != 0, &E);
                    path = E.path;
                    if (!ms::cost_ok(E.cost, max_error)) state = ms::EDGE_COST;
                    else if (!ms::link_ok(ms::common(ru, lu, rv, lv), lu, lv)) state = ms::EDGE_LINK;
                    else if (!ms_keeps_sides(verts, faces, nv, n, idx, seg, F, u, v, E.xt) || !ms_keeps_sides(verts, faces, nv, n, idx, seg, F, v, u, E.xt))
                        state = ms::EDGE_FLIP;
                    else {
                        state = ms::EDGE_OK;
                        k = ms::key(E.cost, i);
                    }
                }
            }
        }
        edge[i] = (unsigned char)state;
        if (mine) key[i] = k;
        if (mirror >= 0 && mirror < entries) key[mirror] = k;
    }
    ms_count(state != ms::EDGE_NONE ? RCMVS_MS_COUNT_CANDIDATES : -1, RCMVS_MS_COUNT_CANDIDATES, 1, counts, sh);
    ms_count(state >= ms::EDGE_COST && state <= ms::EDGE_FLIP ? RCMVS_MS_COUNT_REJECT_COST + state - ms::EDGE_COST : -1, RCMVS_MS_COUNT_REJECT_COST, 3, counts, sh);
    ms_count(path >= 0 ? RCMVS_MS_COUNT_PATH + path : -1, RCMVS_MS_COUNT_PATH, ms::PATHS, counts, sh);
}

// ---- selection --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_best1_kernel(int nv, long long entries, const int* __restrict__ row_start, const int* __restrict__ row_len,
                                                            const u64* __restrict__ key, u64* __restrict__ best1) {
    const long long w = gid();
    if (w >= nv) return;
    u64 best = ms::NO_KEY;
    const long long i0 = row_start[w], i1 = i0 + row_len[w];
    for (long long i = i0 < 0 ? 0 : i0; i < i1 && i < entries; ++i) best = key[i] < best ? key[i] : best;
    best1[w] = best;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_best2_kernel(int nv, long long entries, const int* __restrict__ row_start, const int* __restrict__ row_len,
                                                            const int* __restrict__ nbr, const u64* __restrict__ best1, u64* __restrict__ best2) {
    const long long w = gid();
    if (w >= nv) return;
    u64 best = best1[w];
    const long long i0 = row_start[w], i1 = i0 + row_len[w];
    for (long long i = i0 < 0 ? 0 : i0; i < i1 && i < entries; ++i) {
        const int x = nbr[i];
        if ((unsigned)x < (unsigned)nv) best = best1[x] < best ? best1[x] : best;
    }
    best2[w] = best;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_select_kernel(int nv, long long entries, const int* __restrict__ row_start, const int* __restrict__ nbr,
                                                             const unsigned char* __restrict__ edge, const u64* __restrict__ key, const u64* __restrict__ best2,
                                                             unsigned char* __restrict__ selected) {
    const long long i = gid();
    if (i >= entries) return;
    unsigned char s = 0;
    if (edge[i] == ms::EDGE_OK) {                                 // an entry u -> v inside row_start[nv], v in [0, nv)
        const int u = ms_owner(row_start, nv, i), v = nbr[i];
        s = (key[i] == best2[u] && key[i] == best2[v]) ? 1 : 0;
    }
    selected[i] = s;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_apply_kernel(float* verts, int nv, long long entries, MsFrame F, double* quad, int* members, u64* csum,
                                                            long long target, const int* __restrict__ row_start, const int* __restrict__ nbr,
                                                            const unsigned char* __restrict__ locked, const unsigned char* __restrict__ selected,
                                                            const int* __restrict__ rank, unsigned char* __restrict__ applied, int* remap, u64* counts) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long i = gid();
    unsigned did = 0, worst = 0;
    if (i < entries) {
        const long long allowed = ms::budget((long long)counts[RCMVS_MS_COUNT_LIVE_BEFORE], target);
        did = (selected[i] && rank[i] < allowed) ? 1u : 0u;
        applied[i] = (unsigned char)did;
        if (did) {
            const int u = ms_owner(row_start, nv, i), v = nbr[i];
            MsEdge E;
            ms_edge(verts, quad, F, u, v, locked[u] != 0, locked[v] != 0, &E);
            const int s = locked[v] ? v : u, g = locked[v] ? u : v;
            unsigned* dst = reinterpret_cast<unsigned*>(verts) + 3 * (size_t)s;
#pragma unroll
            for (int a = 0; a < 3; ++a) dst[a] = E.t[a];
            ms_store(quad, s, E.Q);
            members[s] = members[u] + members[v];
            members[g] = 0;
            if (csum) {
#pragma unroll
                for (int a = 0; a < 3; ++a) csum[3 * (size_t)s + a] = csum[3 * (size_t)u + a] + csum[3 * (size_t)v + a];
            }
            remap[g] = s;
            worst = md::ordered((float)E.cost);
        }
    }
    const unsigned n = tm_block_sum(did, sh);
    if (threadIdx.x == 0 && n) atomicAdd(&counts[RCMVS_MS_COUNT_APPLIED], (u64)n);
    sh[threadIdx.x] = worst;
    __syncthreads();
    for (int o = MS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && sh[threadIdx.x + o] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) atomicMax(&counts[RCMVS_MS_COUNT_MAX_COST], (u64)sh[0]);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_rewrite_kernel(const int* __restrict__ faces_in, int* __restrict__ faces_out, int nv, int nf,
                                                              const int* __restrict__ remap, u64* counts) {
    __shared__ unsigned sh[MS_BLOCK];
    const long long f = gid();
    unsigned ok = 0;
    if (f < nf) {
        int w[3] = {faces_in[3 * f], faces_in[3 * f + 1], faces_in[3 * f + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if ((unsigned)w[k] < (unsigned)nv) w[k] = remap[w[k]];
        faces_out[3 * f] = w[0];
        faces_out[3 * f + 1] = w[1];
        faces_out[3 * f + 2] = w[2];
        ok = mc::face_valid(w[0], w[1], w[2], nv) ? 1u : 0u;
    }
    const unsigned s = tm_block_sum(ok, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&counts[RCMVS_MS_COUNT_LIVE], (u64)s);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_end_kernel(u64* __restrict__ live, const u64* __restrict__ counts) {
    if (gid() == 0) live[0] = counts[RCMVS_MS_COUNT_LIVE];
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_vert_init_kernel(const int* __restrict__ members, const u64* __restrict__ csum, int nv, int drop,
                                                                unsigned char* __restrict__ vert_keep, unsigned char* __restrict__ out_rgb) {
    const long long v = gid();
    if (v >= nv) return;
    const int m = members[v];
    vert_keep[v] = (!drop && m > 0) ? 1 : 0;
    if (out_rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out_rgb[3 * v + a] = m > 0 ? md::colour(csum[3 * v + a], (u64)m) : (unsigned char)0;
    }
}

__global__ __launch_bounds__(MS_BLOCK) void ms_face_keep_kernel(const int* __restrict__ faces, int nv, int nf, int drop, unsigned char* __restrict__ face_keep,
                                                                unsigned char* vert_keep) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool keep = mc::face_valid(a, b, c, nv);
    face_keep[f] = keep ? 1 : 0;
    if (keep && drop) { vert_keep[a] = 1; vert_keep[b] = 1; vert_keep[c] = 1; }      // every writer stores the same value
}

static int ms_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0, "%s: nv = %d vertices (0 .. 2^31-1)", what, nv);
    RCMVS_REQUIRE(nf >= 0 && 6ll * nf <= RCMVS_MC_MAX_ENTRIES && 3ll * nf <= RCMVS_MS_MAX_CORNERS, "%s: nf = %d faces (0 .. (2^31-1) / 6)", what, nf);
    return 0;
}

static int ms_frame_args(const char* what, const double* frame_host, MsFrame* F) {
    RCMVS_REQUIRE(frame_host, "%s: null pointer (frame_host)", what);
    for (int a = 0; a < 3; ++a) F->ctr[a] = frame_host[a];
    F->side = frame_host[3];
    RCMVS_REQUIRE(std::isfinite(F->ctr[0]) && std::isfinite(F->ctr[1]) && std::isfinite(F->ctr[2]), "%s: the frame's centre is not finite", what);
    RCMVS_REQUIRE(F->side > 0.0 && std::isfinite(F->side), "%s: side = %g (finite, > 0)", what, F->side);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_ms_init_timed(const float* verts, const int* faces, const unsigned char* rgb, int nv, int nf, const double* frame_host, unsigned* key_a,
                                   int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, double* quad, int* members,
                                   u64* csum, u64* live, u64* stats, void* ev0, void* ev1, void* stream) {
    if (int rc = ms_sizes("ms_init", nv, nf)) return rc;
    MsFrame F;
    if (int rc = ms_frame_args("ms_init", frame_host, &F)) return rc;
    RCMVS_REQUIRE(live && stats, "ms_init: null pointer (live, stats)");
    RCMVS_REQUIRE(nv == 0 || (verts && seg && quad && members), "ms_init: null pointer (verts, seg, quad and members hold nv rows)");
    RCMVS_REQUIRE(nf == 0 || (faces && key_a && idx_a && key_b && idx_b && hist && hist_start),
                  "ms_init: null pointer (faces, key_a, idx_a, key_b, idx_b, hist and hist_start serve 3 nf corners)");
    RCMVS_REQUIRE((rgb == nullptr) == (csum == nullptr) || nv == 0, "ms_init: null pointer (csum goes with rgb)");
    RCMVS_REQUIRE(scan_work, "ms_init: null pointer (scan_work)");
    if (int rc = scan_work_check("ms_init", scan_work)) return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MS_BLOCK), 0, st, e0, none, stats, 4ll);
    ms_incidence(verts, faces, nv, nf, key_a, &idx_a, key_b, idx_b, hist, hist_start, scan_work, seg, stats, st, none);
    RCMVS_LAUNCH_TIMED(ms_init_kernel, dim3(blocks(nv)), dim3(MS_BLOCK), 0, st, none, e1, verts, faces, rgb, nv, 3ll * nf, F, idx_a, seg, quad, members,
                       nv ? csum : nullptr, live, stats);
    return launch_status("ms_init");
}

extern "C" int rcmvs_ms_init(const float* verts, const int* faces, const unsigned char* rgb, int nv, int nf, const double* frame_host, unsigned* key_a, int* idx_a,
                             unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, double* quad, int* members, u64* csum, u64* live,
                             u64* stats, void* stream) {
    return rcmvs_ms_init_timed(verts, faces, rgb, nv, nf, frame_host, key_a, idx_a, key_b, idx_b, hist, hist_start, scan_work, seg, quad, members, csum, live,
                               stats, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ms_round_timed(float* verts, const int* faces_in, int* faces_out, int nv, int nf, const double* frame_host, double* quad, int* members,
                                    u64* csum, long long target_faces, double max_error, int* row_start, int* row_len, int* nbr, int* mult,
                                    unsigned char* on_boundary, int* cursor, int* heavy, int heavy_capacity, u64* adj_stats, unsigned* key_a, int* idx_a,
                                    unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, unsigned char* locked, unsigned char* edge,
                                    u64* key, u64* best1, u64* best2, unsigned char* selected, int* rank, unsigned char* applied, int* remap, u64* live,
                                    u64* counts, int phase, void* ev0, void* ev1, void* stream) {
    if (int rc = ms_sizes("ms_round", nv, nf)) return rc;
    MsFrame F;
    if (int rc = ms_frame_args("ms_round", frame_host, &F)) return rc;
    RCMVS_REQUIRE(target_faces >= 0, "ms_round: target_faces = %lld (>= 0)", target_faces);
    RCMVS_REQUIRE(max_error >= 0.0, "ms_round: max_error = %g (>= 0, +inf allowed)", max_error);
    RCMVS_REQUIRE(phase >= RCMVS_MS_PHASE_ALL && phase <= RCMVS_MS_PHASE_APPLY, "ms_round: phase = %d (0 .. 4)", phase);
    RCMVS_REQUIRE(heavy_capacity >= 6ll * nf / (RCMVS_MC_SORT_LIMIT + 1) + 1, "ms_round: heavy_capacity = %d (at least 6 nf / %d + 1)", heavy_capacity,
                  RCMVS_MC_SORT_LIMIT + 1);
    RCMVS_REQUIRE(row_start && rank && live && counts && adj_stats && heavy, "ms_round: null pointer (row_start, rank, live, counts, adj_stats, heavy)");
    RCMVS_REQUIRE(nv == 0 || (verts && quad && members && row_len && on_boundary && cursor && seg && locked && best1 && best2 && remap),
                  "ms_round: null pointer (verts, quad, members, row_len, on_boundary, cursor, seg, locked, best1, best2 and remap hold nv rows)");
    RCMVS_REQUIRE(nf == 0 || (faces_in && faces_out && nbr && mult && key_a && idx_a && key_b && idx_b && hist && hist_start && edge && key && selected && applied),
                  "ms_round: null pointer (faces_in, faces_out, nbr, mult, key_a, idx_a, key_b, idx_b, hist, hist_start, edge, key, selected and applied serve nf faces)");
    RCMVS_REQUIRE(scan_work, "ms_round: null pointer (scan_work)");
    if (int rc = scan_work_check("ms_round", scan_work)) return rc;
    RCMVS_REQUIRE(!ranges_overlap(faces_in, (size_t)nf * 12, faces_out, (size_t)nf * 12), "ms_round: faces_out overlaps faces_in");
    const long long n = 3ll * nf, entries = 6ll * nf;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    const bool all = phase == RCMVS_MS_PHASE_ALL, topo = phase == RCMVS_MS_PHASE_TOPOLOGY, cand = phase == RCMVS_MS_PHASE_CANDIDATES,
               sel = phase == RCMVS_MS_PHASE_SELECTION, app = phase == RCMVS_MS_PHASE_APPLY;
    // topology
    if (int rc = rcmvs_mc_adjacency_timed(faces_in, nv, nf, row_start, row_len, nbr, mult, on_boundary, cursor, heavy, heavy_capacity, scan_work, adj_stats,
                                          (all || topo) ? ev0 : nullptr, nullptr, stream))
        return rc;
    hipLaunchKernelGGL(ms_begin_kernel, dim3(blocks(nv > RCMVS_MS_COUNTS ? nv : RCMVS_MS_COUNTS)), dim3(MS_BLOCK), 0, st, remap, nv, live, counts);
    ms_incidence(verts, faces_in, nv, nf, key_a, &idx_a, key_b, idx_b, hist, hist_start, scan_work, seg, nullptr, st, none);
    RCMVS_LAUNCH_TIMED(ms_lock_kernel, dim3(blocks(nv)), dim3(MS_BLOCK), 0, st, none, topo ? e1 : none, verts, nv, entries, row_start, row_len, mult, locked, counts);
    // candidates
    RCMVS_LAUNCH_TIMED(ms_candidate_kernel, dim3(blocks(entries)), dim3(MS_BLOCK), 0, st, cand ? e0 : none, cand ? e1 : none, verts, faces_in, nv, n, entries, F, quad,
                       max_error, row_start, row_len, nbr, mult, idx_a, seg, locked, edge, key, counts);
    // selection
    RCMVS_LAUNCH_TIMED(ms_best1_kernel, dim3(blocks(nv)), dim3(MS_BLOCK), 0, st, sel ? e0 : none, none, nv, entries, row_start, row_len, key, best1);
    hipLaunchKernelGGL(ms_best2_kernel, dim3(blocks(nv)), dim3(MS_BLOCK), 0, st, nv, entries, row_start, row_len, nbr, best1, best2);
    hipLaunchKernelGGL(ms_select_kernel, dim3(blocks(entries)), dim3(MS_BLOCK), 0, st, nv, entries, row_start, nbr, edge, key, best2, selected);
    scan3<unsigned char>(selected, entries, rank, scan_work, counts + RCMVS_MS_COUNT_SELECTED, st, none, sel ? e1 : none);
    // apply
    RCMVS_LAUNCH_TIMED(ms_apply_kernel, dim3(blocks(entries)), dim3(MS_BLOCK), 0, st, app ? e0 : none, none, verts, nv, entries, F, quad, members, csum, target_faces,
                       row_start, nbr, locked, selected, rank, applied, remap, counts);
    hipLaunchKernelGGL(ms_rewrite_kernel, dim3(blocks(nf)), dim3(MS_BLOCK), 0, st, faces_in, faces_out, nv, nf, remap, counts);
    RCMVS_LAUNCH_TIMED(ms_end_kernel, dim3(1), dim3(MS_BLOCK), 0, st, none, (all || app) ? e1 : none, live, counts);
    return launch_status("ms_round");
}

extern "C" int rcmvs_ms_round(float* verts, const int* faces_in, int* faces_out, int nv, int nf, const double* frame_host, double* quad, int* members, u64* csum,
                              long long target_faces, double max_error, int* row_start, int* row_len, int* nbr, int* mult, unsigned char* on_boundary, int* cursor,
                              int* heavy, int heavy_capacity, u64* adj_stats, unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start,
                              int* scan_work, int* seg, unsigned char* locked, unsigned char* edge, u64* key, u64* best1, u64* best2, unsigned char* selected,
                              int* rank, unsigned char* applied, int* remap, u64* live, u64* counts, void* stream) {
    return rcmvs_ms_round_timed(verts, faces_in, faces_out, nv, nf, frame_host, quad, members, csum, target_faces, max_error, row_start, row_len, nbr, mult,
                                on_boundary, cursor, heavy, heavy_capacity, adj_stats, key_a, idx_a, key_b, idx_b, hist, hist_start, scan_work, seg, locked, edge, key,
                                best1, best2, selected, rank, applied, remap, live, counts, RCMVS_MS_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ms_finish_timed(const int* faces, int nv, int nf, const int* members, const u64* csum, int drop_unreferenced, unsigned char* face_keep,
                                     unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, unsigned char* out_rgb, u64* totals, void* ev0,
                                     void* ev1, void* stream) {
    if (int rc = ms_sizes("ms_finish", nv, nf)) return rc;
    RCMVS_REQUIRE(face_rank && vert_rank && totals, "ms_finish: null pointer (face_rank, vert_rank, totals)");
    RCMVS_REQUIRE(nf == 0 || (faces && face_keep), "ms_finish: null pointer (faces and face_keep hold nf rows)");
    RCMVS_REQUIRE(nv == 0 || (members && vert_keep), "ms_finish: null pointer (members and vert_keep hold nv rows)");
    RCMVS_REQUIRE((csum == nullptr) == (out_rgb == nullptr) || nv == 0, "ms_finish: null pointer (out_rgb goes with csum)");
    RCMVS_REQUIRE(scan_work, "ms_finish: null pointer (scan_work)");
    if (int rc = scan_work_check("ms_finish", scan_work)) return rc;
    const int drop = drop_unreferenced != 0;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(ms_vert_init_kernel, dim3(blocks(nv)), dim3(MS_BLOCK), 0, st, e0, none, members, csum, nv, drop, vert_keep, nv ? out_rgb : nullptr);
    hipLaunchKernelGGL(ms_face_keep_kernel, dim3(blocks(nf)), dim3(MS_BLOCK), 0, st, faces, nv, nf, drop, face_keep, vert_keep);
    scan3<unsigned char>(face_keep, nf, face_rank, scan_work, totals, st, none, none);
    scan3<unsigned char>(vert_keep, nv, vert_rank, scan_work, totals + 1, st, none, e1);
    return launch_status("ms_finish");
}

extern "C" int rcmvs_ms_finish(const int* faces, int nv, int nf, const int* members, const u64* csum, int drop_unreferenced, unsigned char* face_keep,
                               unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, unsigned char* out_rgb, u64* totals, void* stream) {
    return rcmvs_ms_finish_timed(faces, nv, nf, members, csum, drop_unreferenced, face_keep, vert_keep, face_rank, vert_rank, scan_work, out_rgb, totals, nullptr,
                                 nullptr, stream);
}
