// Clean-up of an extracted triangle mesh: connected components, selection, stable compaction, the 1-ring and Taubin smoothing
// (rc_mvsnet_amd/mesh_clean.py; contract in mesh_clean.h, the per-element rules in mesh_clean_math.h).
//
//   components  Union-find over the vertices on label[] (ECL-CC): one thread per face hooks a-b and b-c, always the larger root
//               under the smaller by atomicCAS, halving the paths it walks; a flatten pass then writes every vertex's root, which
//               is the smallest vertex of its component whatever the order of the hooks was (DESIGN.md has the argument).  No
//               thread waits for another: a failed CAS means another hook succeeded, and the retry starts strictly lower.
//   scan        Flags or counts -> exclusive prefix sums in three levels: scan_sort.hip's scan3, which mesh_decimate.hip and
//               mesh_holes.hip call too.  Used for the component table, the kept faces, the kept vertices and the 1-ring's
//               row starts.
//   select      Per face the keep rule of its first index's component; kept faces mark their vertices with plain byte stores of 1.
//   gather      Kept vertices and faces to their ranks: stable, bit copies, indices rewritten through the vertex rank.
//   adjacency   Entry counts by atomicAdd, scan, fill through the same counters counting down (arbitrary order inside a segment),
//               then every segment sorted and collapsed to (neighbour, multiplicity): up to 48 entries by one lane in LDS, longer
//               ones listed and sorted by a workgroup in place.  The edge statistics are integer sums.
//   taubin      One thread per vertex: fp64 sum of the neighbours in ascending order, one rounding to fp32 per step.
// gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_clean.h"
#include "mesh_clean_math.h"
#include "scan_sort.h"                                            // gid, blocks, scan3, zero_kernel
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MC_BLOCK = TM_BLOCK;
constexpr int MC_LIMIT = RCMVS_MC_SORT_LIMIT;
constexpr int MC_HEAVY_GRID = 64;
static_assert(MC_BLOCK == SS_BLOCK, "gid, blocks and zero_kernel count in this family's block");
static_assert(RCMVS_MC_SCAN_TILE == SS_TILE && RCMVS_MC_SCAN_WORK == SS_WORK, "mesh_clean.h describes scan_sort.h's work area");
static_assert(MC_LIMIT * MC_BLOCK * 4 <= 64 * 1024, "the lanes' segments share one block's static LDS");

using u64 = unsigned long long;

// ---- components ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_init_kernel(int* __restrict__ label, int* __restrict__ comp_faces, int nv, u64* __restrict__ counts) {
    const long long v = gid();
    if (v < nv) { label[v] = (int)v; comp_faces[v] = 0; }
    if (v < 4) counts[v] = 0;
}

// The representative of v's tree, halving the path.  parent[x] <= x always and a vertex that is no root never becomes one again,
// so every value that memory ever held is an ancestor of v, and the plain stores only ever touch vertices that are no roots.
// The loads are volatile (they bypass the caches that are not coherent across the chip): with ordinary cached loads the labels
// came out wrong on the MI355X, so nothing here relies on what such a cache would return.
__device__ inline int mc_find(int* parent, int v) {
    volatile int* p = parent;
    int cur = p[v];
    if (cur != v) {
        int prev = v, next;
        while (cur > (next = p[cur])) {
            p[prev] = next;
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

__device__ inline void mc_unite(int* parent, int a, int b) {
    int ra = mc_find(parent, a), rb = mc_find(parent, b);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) break;                                     // hi was a root and hangs under lo now
        ra = old;                                                 // hi had been hooked already: go on from its parent, old < hi
        rb = lo;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_hook_kernel(const int* __restrict__ faces, int nv, int nf, int* parent, unsigned char* __restrict__ face_ok,
                                                           u64* counts) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool ok = mc::face_valid(a, b, c, nv);
    face_ok[f] = ok ? 1 : 0;
    if (!ok) { atomicAdd(&counts[0], (u64)1); return; }
    mc_unite(parent, a, b);
    mc_unite(parent, b, c);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_flatten_kernel(int* parent, int nv) {
    const long long v = gid();
    if (v >= nv) return;
    volatile int* p = parent;
    int r = (int)v, n;
    while ((n = p[r]) != r) r = n;                                // the roots are fixed by now; other lanes only shorten paths
    p[v] = r;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_face_count_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ face_ok, int nf,
                                                                 const int* __restrict__ label, int* comp_faces) {
    const long long f = gid();
    if (f >= nf || !face_ok[f]) return;
    atomicAdd(&comp_faces[label[faces[3 * f]]], 1);
}

// ---- component table ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_root_flag_kernel(const int* __restrict__ label, const int* __restrict__ comp_faces, int nv,
                                                                unsigned char* __restrict__ flags, u64* totals) {
    __shared__ unsigned sh[MC_BLOCK];
    const long long v = gid();
    unsigned most = 0;
    if (v < nv) {
        const bool row = label[v] == (int)v && comp_faces[v] > 0;
        flags[v] = row ? 1 : 0;
        if (row) most = (unsigned)comp_faces[v];
    }
    sh[threadIdx.x] = most;
    __syncthreads();
    for (int o = MC_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && sh[threadIdx.x + o] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] > 0) atomicMax(&totals[1], (u64)sh[0]);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_table_kernel(const int* __restrict__ comp_faces, int nv, const unsigned char* __restrict__ flags,
                                                            const int* __restrict__ rank, int* __restrict__ table, int capacity) {
    const long long v = gid();
    if (v >= nv || !flags[v]) return;
    const int r = rank[v];
    if (r < 0 || r >= capacity) return;
    table[2 * (size_t)r] = (int)v;
    table[2 * (size_t)r + 1] = comp_faces[v];
}

// ---- select -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_vert_init_kernel(const int* __restrict__ label, const int* __restrict__ comp_faces, int nv, mc::Select sel,
                                                                int drop, unsigned char* __restrict__ vert_keep, u64* totals) {
    __shared__ unsigned sh[MC_BLOCK];
    const long long v = gid();
    unsigned kept = 0;
    if (v < nv) {
        vert_keep[v] = drop ? 0 : 1;
        kept = label[v] == (int)v && comp_faces[v] > 0 && mc::keep(comp_faces[v], (int)v, sel);
    }
    const unsigned s = tm_block_sum(kept, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&totals[2], (u64)s);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_face_keep_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ face_ok,
                                                                const int* __restrict__ label, const int* __restrict__ comp_faces, int nv, int nf,
                                                                mc::Select sel, int drop, unsigned char* __restrict__ face_keep, unsigned char* vert_keep) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bool keep = face_ok[f] && mc::face_valid(a, b, c, nv);
    if (keep) {
        const int l = label[a];
        keep = (unsigned)l < (unsigned)nv && mc::keep(comp_faces[l], l, sel);
    }
    face_keep[f] = keep ? 1 : 0;
    if (keep && drop) { vert_keep[a] = 1; vert_keep[b] = 1; vert_keep[c] = 1; }      // every writer stores the same value
}

// ---- gather -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_gather_verts_kernel(const unsigned* __restrict__ verts, const unsigned char* __restrict__ rgb,
                                                                   const unsigned char* __restrict__ vert_keep, const int* __restrict__ vert_rank, int nv,
                                                                   int nv_out, unsigned* __restrict__ out_verts, unsigned char* __restrict__ out_rgb) {
    const long long v = gid();
    if (v >= nv || !vert_keep[v]) return;
    const int r = vert_rank[v];
    if (r < 0 || r >= nv_out) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) out_verts[3 * (size_t)r + e] = verts[3 * v + e];
    if (out_rgb) {
#pragma unroll
        for (int e = 0; e < 3; ++e) out_rgb[3 * (size_t)r + e] = rgb[3 * v + e];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_gather_faces_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ face_keep,
                                                                   const int* __restrict__ face_rank, const int* __restrict__ vert_rank, int nv, int nf,
                                                                   int nf_out, int* __restrict__ out_faces) {
    const long long f = gid();
    if (f >= nf || !face_keep[f]) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const int r = face_rank[f];
    if (r < 0 || r >= nf_out || !mc::face_valid(a, b, c, nv)) return;
    out_faces[3 * (size_t)r] = vert_rank[a];
    out_faces[3 * (size_t)r + 1] = vert_rank[b];
    out_faces[3 * (size_t)r + 2] = vert_rank[c];
}

// ---- adjacency ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_zero_int_kernel(int* __restrict__ p, int n, u64* __restrict__ stats) {
    const long long i = gid();
    if (i < n) p[i] = 0;
    if (i < 6) stats[i] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_degree_kernel(const int* __restrict__ faces, int nv, int nf, int* cursor) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!mc::face_valid(a, b, c, nv)) return;
    atomicAdd(&cursor[a], 2);
    atomicAdd(&cursor[b], 2);
    atomicAdd(&cursor[c], 2);
}

// cursor[v] counts down from the segment's length: the slot order inside a segment is arbitrary, the sort removes it
__global__ __launch_bounds__(MC_BLOCK) void mc_fill_kernel(const int* __restrict__ faces, int nv, int nf, const int* __restrict__ row_start, int* cursor,
                                                           int* __restrict__ nbr) {
    const long long f = gid();
    if (f >= nf) return;
    const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (!mc::face_valid(idx[0], idx[1], idx[2], nv)) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int v = idx[e], lo = row_start[v], hi = row_start[v + 1];
#pragma unroll
        for (int o = 1; o < 3; ++o) {
            const int at = lo + atomicAdd(&cursor[v], -1) - 1;
            if (at >= lo && at < hi) nbr[at] = idx[(e + o) % 3];
        }
    }
}

struct McEdgeStats {
    unsigned edges, boundary, nonmanifold;
};

// A sorted run of d entries read through get(k) -> (neighbour, multiplicity) pairs at nbr / mult[s0 ..], padded with -1 / 0; the
// writes trail the reads, so get may read nbr itself.  Every undirected edge is counted at its smaller end.
template <class Get>
__device__ inline int mc_collapse(int v, int s0, int d, Get get, int* __restrict__ nbr, int* __restrict__ mult, McEdgeStats* st, int* on_boundary) {
    int u = 0, k = 0, bnd = 0;
    while (k < d) {
        const int w = get(k);
        int c = 1;
        while (k + c < d && get(k + c) == w) ++c;
        nbr[s0 + u] = w;
        mult[s0 + u] = c;
        ++u;
        k += c;
        if (c == 1) bnd = 1;
        if (w > v) {
            st->edges += 1;
            st->boundary += c == 1;
            st->nonmanifold += c > 2;
        }
    }
    for (int q = u; q < d; ++q) { nbr[s0 + q] = -1; mult[s0 + q] = 0; }
    *on_boundary = bnd;
    return u;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_sort_kernel(int nv, const int* __restrict__ row_start, int* __restrict__ row_len, int* __restrict__ nbr,
                                                           int* __restrict__ mult, unsigned char* __restrict__ on_boundary, int* __restrict__ heavy,
                                                           int heavy_capacity, u64* stats) {
    __shared__ int seg[MC_LIMIT * MC_BLOCK];                      // entry k of lane t at seg[k * MC_BLOCK + t]: no bank conflicts
    __shared__ unsigned sh[MC_BLOCK];
    const long long v = gid();
    const int t = threadIdx.x;
    McEdgeStats st = {0u, 0u, 0u};
    unsigned referenced = 0;
    if (v < nv) {
        const int s0 = row_start[v], d = row_start[v + 1] - s0;
        if (d <= 0) {
            row_len[v] = 0;
            on_boundary[v] = 0;
        } else if (d > MC_LIMIT) {
            const u64 slot = atomicAdd(&stats[4], (u64)1);
            if (slot < (u64)heavy_capacity) heavy[slot] = (int)v;
        } else {
            for (int k = 0; k < d; ++k) seg[k * MC_BLOCK + t] = nbr[s0 + k];
            for (int k = 1; k < d; ++k) {                         // insertion sort, ascending
                const int x = seg[k * MC_BLOCK + t];
                int j = k - 1;
                while (j >= 0 && seg[j * MC_BLOCK + t] > x) { seg[(j + 1) * MC_BLOCK + t] = seg[j * MC_BLOCK + t]; --j; }
                seg[(j + 1) * MC_BLOCK + t] = x;
            }
            int bnd;
            row_len[v] = mc_collapse((int)v, s0, d, [&](int k) { return seg[k * MC_BLOCK + t]; }, nbr, mult, &st, &bnd);
            on_boundary[v] = (unsigned char)bnd;
            referenced = 1;
        }
    }
    const unsigned e = tm_block_sum(st.edges, sh), b = tm_block_sum(st.boundary, sh), m = tm_block_sum(st.nonmanifold, sh);
    const unsigned r = tm_block_sum(referenced, sh);
    if (threadIdx.x == 0) {
        if (e) atomicAdd(&stats[0], (u64)e);
        if (b) atomicAdd(&stats[1], (u64)b);
        if (m) atomicAdd(&stats[2], (u64)m);
        if (r) atomicAdd(&stats[3], (u64)r);
    }
}

// Segments longer than MC_LIMIT: a workgroup per listed vertex, odd-even transposition in place (d phases of d / 2 independent
// compare-exchanges), then one lane collapses the run.  Any length; the order of the list does not matter.
__global__ __launch_bounds__(MC_BLOCK) void mc_sort_heavy_kernel(int nv, const int* __restrict__ row_start, int* __restrict__ row_len, int* nbr,
                                                                 int* __restrict__ mult, unsigned char* __restrict__ on_boundary,
                                                                 const int* __restrict__ heavy, int heavy_capacity, u64* stats) {
    const u64 listed = stats[4];
    const int n = listed < (u64)heavy_capacity ? (int)listed : heavy_capacity;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int v = heavy[i];
        if ((unsigned)v >= (unsigned)nv) continue;                // uniform over the block
        const int s0 = row_start[v], d = row_start[v + 1] - s0;
        for (int phase = 0; phase < d; ++phase) {
            for (long long j = (phase & 1) + 2ll * threadIdx.x; j + 1 < d; j += 2ll * MC_BLOCK) {
                const int x = nbr[s0 + j], y = nbr[s0 + j + 1];
                if (x > y) { nbr[s0 + j] = y; nbr[s0 + j + 1] = x; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            McEdgeStats st = {0u, 0u, 0u};
            int bnd;
            row_len[v] = mc_collapse(v, s0, d, [&](int k) { return nbr[s0 + k]; }, nbr, mult, &st, &bnd);
            on_boundary[v] = (unsigned char)bnd;
            if (st.edges) atomicAdd(&stats[0], (u64)st.edges);
            if (st.boundary) atomicAdd(&stats[1], (u64)st.boundary);
            if (st.nonmanifold) atomicAdd(&stats[2], (u64)st.nonmanifold);
            atomicAdd(&stats[3], (u64)1);
        }
        __syncthreads();
    }
}

// ---- Taubin -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_taubin_kernel(const float* __restrict__ src, float* __restrict__ dst, int nv, const int* __restrict__ row_start,
                                                             const int* __restrict__ row_len, const int* __restrict__ nbr, long long entries,
                                                             const unsigned char* __restrict__ pinned, double f) {
    const long long v = gid();
    if (v >= nv) return;
    const unsigned* sb = reinterpret_cast<const unsigned*>(src);
    unsigned* db = reinterpret_cast<unsigned*>(dst);
    const int s0 = row_start[v], len = row_len[v];
    bool move = len >= 1 && !(pinned && pinned[v]) && s0 >= 0 && (long long)s0 + len <= entries;
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = 0; move && k < len; ++k) {
        const int w = nbr[s0 + k];
        if ((unsigned)w >= (unsigned)nv) { move = false; break; }
#pragma unroll
        for (int e = 0; e < 3; ++e) s[e] += (double)src[3 * (size_t)w + e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (move) dst[3 * v + e] = mc::taubin(src[3 * v + e], s[e], len, f);
        else db[3 * v + e] = sb[3 * v + e];
    }
}

static int mc_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0 && nf >= 0, "%s: %d vertices, %d faces (0 .. 2^31-1 each)", what, nv, nf);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_mc_components_timed(const int* faces, int nv, int nf, int* label, unsigned char* face_ok, int* comp_faces, u64* counts, void* ev0,
                                         void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_components", nv, nf)) return rc;
    RCMVS_REQUIRE(counts && (nf == 0 || (faces && face_ok)) && (nv == 0 || (label && comp_faces)), "mc_components: null pointer");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(mc_init_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, e0, none, label, comp_faces, nv, counts);
    hipLaunchKernelGGL(mc_hook_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, faces, nv, nf, label, face_ok, counts);
    hipLaunchKernelGGL(mc_flatten_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, label, nv);
    RCMVS_LAUNCH_TIMED(mc_face_count_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, none, e1, faces, face_ok, nf, label, comp_faces);
    return launch_status("mc_components");
}

extern "C" int rcmvs_mc_components(const int* faces, int nv, int nf, int* label, unsigned char* face_ok, int* comp_faces, u64* counts, void* stream) {
    return rcmvs_mc_components_timed(faces, nv, nf, label, face_ok, comp_faces, counts, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mc_component_table_timed(const int* label, const int* comp_faces, int nv, unsigned char* flags, int* rank, int* scan_work, int* table,
                                              int capacity, u64* totals, void* ev0, void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_component_table", nv, 0)) return rc;
    RCMVS_REQUIRE(rank && totals && (nv == 0 || (label && comp_faces && flags)), "mc_component_table: null pointer");
    RCMVS_REQUIRE(capacity >= 0 && (table || capacity == 0), "mc_component_table: capacity = %d (>= 0, with a table)", capacity);
    if (int rc = scan_work_check("mc_component_table", scan_work)) return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MC_BLOCK), 0, st, e0, none, totals, 2ll);
    hipLaunchKernelGGL(mc_root_flag_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, label, comp_faces, nv, flags, totals);
    scan3<unsigned char>(flags, nv, rank, scan_work, totals, st, none, none);
    RCMVS_LAUNCH_TIMED(mc_table_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, none, e1, comp_faces, nv, flags, rank, table, capacity);
    return launch_status("mc_component_table");
}

extern "C" int rcmvs_mc_component_table(const int* label, const int* comp_faces, int nv, unsigned char* flags, int* rank, int* scan_work, int* table,
                                        int capacity, u64* totals, void* stream) {
    return rcmvs_mc_component_table_timed(label, comp_faces, nv, flags, rank, scan_work, table, capacity, totals, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mc_select_timed(const int* faces, const unsigned char* face_ok, const int* label, const int* comp_faces, int nv, int nf, int min_faces,
                                     double min_fraction, int max_faces, int keep_largest, int k_faces, int k_label, int drop_unreferenced,
                                     unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, u64* totals,
                                     void* ev0, void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_select", nv, nf)) return rc;
    RCMVS_REQUIRE(face_rank && vert_rank && totals && (nf == 0 || (faces && face_ok && face_keep)) && (nv == 0 || (label && comp_faces && vert_keep)),
                  "mc_select: null pointer");
    RCMVS_REQUIRE(min_faces >= 0 && keep_largest >= 0, "mc_select: min_faces = %d, keep_largest = %d (>= 0 each)", min_faces, keep_largest);
    RCMVS_REQUIRE(std::isfinite(min_fraction), "mc_select: min_fraction = %g (finite)", min_fraction);
    if (int rc = scan_work_check("mc_select", scan_work)) return rc;
    const mc::Select sel = {min_faces, min_fraction, max_faces, keep_largest, k_faces, k_label};
    const int drop = drop_unreferenced != 0;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MC_BLOCK), 0, st, e0, none, totals, 3ll);
    hipLaunchKernelGGL(mc_vert_init_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, label, comp_faces, nv, sel, drop, vert_keep, totals);
    hipLaunchKernelGGL(mc_face_keep_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, faces, face_ok, label, comp_faces, nv, nf, sel, drop, face_keep,
                       vert_keep);
    scan3<unsigned char>(face_keep, nf, face_rank, scan_work, totals, st, none, none);
    scan3<unsigned char>(vert_keep, nv, vert_rank, scan_work, totals + 1, st, none, e1);
    return launch_status("mc_select");
}

extern "C" int rcmvs_mc_select(const int* faces, const unsigned char* face_ok, const int* label, const int* comp_faces, int nv, int nf, int min_faces,
                               double min_fraction, int max_faces, int keep_largest, int k_faces, int k_label, int drop_unreferenced,
                               unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, u64* totals,
                               void* stream) {
    return rcmvs_mc_select_timed(faces, face_ok, label, comp_faces, nv, nf, min_faces, min_fraction, max_faces, keep_largest, k_faces, k_label,
                                 drop_unreferenced, face_keep, vert_keep, face_rank, vert_rank, scan_work, totals, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mc_gather_timed(const float* verts, const unsigned char* rgb, const int* faces, const unsigned char* face_keep, const int* face_rank,
                                     const unsigned char* vert_keep, const int* vert_rank, int nv, int nf, int nv_out, int nf_out, float* out_verts,
                                     unsigned char* out_rgb, int* out_faces, void* ev0, void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_gather", nv, nf)) return rc;
    RCMVS_REQUIRE(nv_out >= 0 && nv_out <= nv && nf_out >= 0 && nf_out <= nf, "mc_gather: %d of %d vertices, %d of %d faces out", nv_out, nv, nf_out, nf);
    RCMVS_REQUIRE(face_rank && vert_rank && (nf == 0 || (faces && face_keep)) && (nv == 0 || (verts && vert_keep)) && (nv_out == 0 || out_verts) &&
                  (nf_out == 0 || out_faces), "mc_gather: null pointer");
    RCMVS_REQUIRE(!out_rgb || rgb, "mc_gather: null pointer (out_rgb needs rgb)");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(mc_gather_verts_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, e0, none, reinterpret_cast<const unsigned*>(verts), rgb, vert_keep,
                       vert_rank, nv, nv_out, reinterpret_cast<unsigned*>(out_verts), out_rgb);
    RCMVS_LAUNCH_TIMED(mc_gather_faces_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, none, e1, faces, face_keep, face_rank, vert_rank, nv, nf, nf_out,
                       out_faces);
    return launch_status("mc_gather");
}

extern "C" int rcmvs_mc_gather(const float* verts, const unsigned char* rgb, const int* faces, const unsigned char* face_keep, const int* face_rank,
                               const unsigned char* vert_keep, const int* vert_rank, int nv, int nf, int nv_out, int nf_out, float* out_verts,
                               unsigned char* out_rgb, int* out_faces, void* stream) {
    return rcmvs_mc_gather_timed(verts, rgb, faces, face_keep, face_rank, vert_keep, vert_rank, nv, nf, nv_out, nf_out, out_verts, out_rgb, out_faces, nullptr,
                                 nullptr, stream);
}

extern "C" int rcmvs_mc_adjacency_timed(const int* faces, int nv, int nf, int* row_start, int* row_len, int* nbr, int* mult, unsigned char* on_boundary,
                                        int* cursor, int* heavy, int heavy_capacity, int* scan_work, u64* stats, void* ev0, void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_adjacency", nv, nf)) return rc;
    RCMVS_REQUIRE(6ll * nf <= RCMVS_MC_MAX_ENTRIES, "mc_adjacency: %d faces (6 entries each, at most 2^31-1 entries)", nf);
    RCMVS_REQUIRE(row_start && stats && heavy && (nf == 0 || (faces && nbr && mult)) && (nv == 0 || (row_len && on_boundary && cursor)),
                  "mc_adjacency: null pointer");
    RCMVS_REQUIRE(heavy_capacity >= 6ll * nf / (MC_LIMIT + 1) + 1, "mc_adjacency: heavy_capacity = %d (at least 6 nf / %d + 1)", heavy_capacity,
                  MC_LIMIT + 1);
    if (int rc = scan_work_check("mc_adjacency", scan_work)) return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(mc_zero_int_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, e0, none, cursor, nv, stats);
    hipLaunchKernelGGL(mc_degree_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, faces, nv, nf, cursor);
    scan3<int>(cursor, nv, row_start, scan_work, stats + 5, st, none, none);
    hipLaunchKernelGGL(mc_fill_kernel, dim3(blocks(nf)), dim3(MC_BLOCK), 0, st, faces, nv, nf, row_start, cursor, nbr);
    hipLaunchKernelGGL(mc_sort_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, st, nv, row_start, row_len, nbr, mult, on_boundary, heavy, heavy_capacity,
                       stats);
    const int grid = heavy_capacity < MC_HEAVY_GRID ? heavy_capacity : MC_HEAVY_GRID;
    RCMVS_LAUNCH_TIMED(mc_sort_heavy_kernel, dim3(grid), dim3(MC_BLOCK), 0, st, none, e1, nv, row_start, row_len, nbr, mult, on_boundary, heavy,
                       heavy_capacity, stats);
    return launch_status("mc_adjacency");
}

extern "C" int rcmvs_mc_adjacency(const int* faces, int nv, int nf, int* row_start, int* row_len, int* nbr, int* mult, unsigned char* on_boundary,
                                  int* cursor, int* heavy, int heavy_capacity, int* scan_work, u64* stats, void* stream) {
    return rcmvs_mc_adjacency_timed(faces, nv, nf, row_start, row_len, nbr, mult, on_boundary, cursor, heavy, heavy_capacity, scan_work, stats, nullptr,
                                    nullptr, stream);
}

extern "C" int rcmvs_mc_taubin_step_timed(const float* src, float* dst, int nv, const int* row_start, const int* row_len, const int* nbr, long long entries,
                                          const unsigned char* pinned, double f, void* ev0, void* ev1, void* stream) {
    if (int rc = mc_sizes("mc_taubin_step", nv, 0)) return rc;
    RCMVS_REQUIRE(entries >= 0 && entries <= RCMVS_MC_MAX_ENTRIES, "mc_taubin_step: %lld entries (0 .. 2^31-1)", entries);
    RCMVS_REQUIRE((nv == 0 || (src && dst && row_start && row_len)) && (entries == 0 || nbr), "mc_taubin_step: null pointer");
    RCMVS_REQUIRE(std::isfinite(f), "mc_taubin_step: factor = %g (finite)", f);
    if (nv > 0) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst), bytes = (uintptr_t)nv * 12;
        RCMVS_REQUIRE(a + bytes <= b || b + bytes <= a, "mc_taubin_step: src and dst overlap (a Jacobi step reads the old positions)");
    }
    RCMVS_LAUNCH_TIMED(mc_taubin_kernel, dim3(blocks(nv)), dim3(MC_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1),
                       src, dst, nv, row_start, row_len, nbr, entries, pinned, f);
    return launch_status("mc_taubin_step");
}

extern "C" int rcmvs_mc_taubin_step(const float* src, float* dst, int nv, const int* row_start, const int* row_len, const int* nbr, long long entries,
                                    const unsigned char* pinned, double f, void* stream) {
    return rcmvs_mc_taubin_step_timed(src, dst, nv, row_start, row_len, nbr, entries, pinned, f, nullptr, nullptr, stream);
}
