// Decimation of a triangle mesh by vertex clustering on a regular lattice with quadric-error placement (Lindstrom's out-of-core
// simplification; rc_mvsnet_amd/mesh_decimate.py; contract in mesh_decimate.h, the per-element rules in mesh_decimate_math.h).
//
//   bounds     the box of the finite vertices as integer-ordered keys: block minima / maxima in LDS, then atomicMin / atomicMax.
//   cluster    63-bit cell keys, an LSD radix sort of (key, vertex) pairs, 8 bits a pass (scan_sort.hip's kernels: per-block
//              digit histograms, one scan over the digit-major (digit, block) table, a stable scatter whose in-block rank comes
//              from wave ballots), only as many passes as the lattice needs, ending in either buffer.  Segment heads + scan
//              number the clusters; stable passes from vertex order leave every cluster's members ascending.
//   classify   per face its three clusters and the first rule that drops it; duplicates (up to rotation) through an
//              open-addressing hash table of face numbers: a triple always settles in the first slot of its probe sequence that
//              no other triple holds, and atomicMin leaves the smallest face number there, whatever the insertion order.
//   quadrics   a second stable sort, of the 3 nf (cluster, corner) pairs on 32-bit keys; one thread per cluster then walks its
//              segment and adds the corners' plane quadrics in fp64 in ascending (face, corner) order.
//   place      one thread per cluster: the members' mean in ascending vertex order, the regularised quadric minimiser by Cramer's
//              rule or the mean, integer colour sums.
//   select     flags and ranks of the kept faces and the clusters they use, for mesh_clean's gather.
//   scan       flags or counts -> exclusive prefix sums in three levels: scan_sort.hip's scan3, which the radix passes use too.
// No thread waits for another workgroup and there are no floating-point atomics.  gfx950 only; __syncthreads, ballots, plain
// loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_decimate.h"
#include "mesh_decimate_math.h"
#include "scan_sort.h"                                            // gid, blocks, scan3, radix_sort, segments_kernel, zero_kernel
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MD_BLOCK = TM_BLOCK;
constexpr int MD_BOUNDS_GRID = 1024;
static_assert(MD_BLOCK == RCMVS_MD_SORT_BLOCK && MD_BLOCK == SS_BLOCK, "a sort block is one workgroup's threads");
static_assert(RCMVS_MD_SCAN_TILE == SS_TILE && RCMVS_MD_SCAN_WORK == SS_WORK, "mesh_decimate.h describes scan_sort.h's work area");

using u64 = unsigned long long;

struct MdLattice {
    double org[3];
    double cell;
    long long g[3];
};

// ---- bounds -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_BLOCK) void md_bounds_init_kernel(unsigned* __restrict__ bounds) {
    if (blockIdx.x == 0 && threadIdx.x < 8) bounds[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(MD_BLOCK) void md_bounds_kernel(const float* __restrict__ verts, int nv, unsigned* bounds) {
    __shared__ unsigned sh[7][MD_BLOCK];
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, cnt = 0;
    for (long long v = gid(); v < nv; v += (long long)gridDim.x * MD_BLOCK) {
        const float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
        if (!md::finite3(p[0], p[1], p[2])) continue;
        ++cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned k = md::ordered(p[a]);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
    const int t = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) { sh[a][t] = lo[a]; sh[3 + a][t] = hi[a]; }
    sh[6][t] = cnt;
    __syncthreads();
    for (int o = MD_BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (sh[a][t + o] < sh[a][t]) sh[a][t] = sh[a][t + o];
                if (sh[3 + a][t + o] > sh[3 + a][t]) sh[3 + a][t] = sh[3 + a][t + o];
            }
            sh[6][t] += sh[6][t + o];
        }
        __syncthreads();
    }
    if (t == 0 && sh[6][0]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&bounds[a], sh[a][0]); atomicMax(&bounds[3 + a], sh[3 + a][0]); }
        atomicAdd(&bounds[6], sh[6][0]);
    }
}

// ---- clusters -----------------------------------------------------------------------------------------------------------------
// the vertex's cell on the lattice -> true and its three coordinates, false for a vertex that is not clustered
__device__ inline bool md_cell(const float* __restrict__ verts, long long v, const MdLattice& L, long long* k) {
    const float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    if (!md::finite3(p[0], p[1], p[2])) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = md::cell_coord(p[a], L.org[a], L.cell);
        if (!(c >= 0.0 && c < (double)L.g[a])) return false;
        k[a] = (long long)c;
    }
    return true;
}

__global__ __launch_bounds__(MD_BLOCK) void md_vertex_key_kernel(const float* __restrict__ verts, int nv, MdLattice L, u64 behind, u64* __restrict__ key,
                                                                 int* __restrict__ idx, u64* totals) {
    __shared__ unsigned sh[MD_BLOCK];
    const long long v = gid();
    unsigned in = 0;
    if (v < nv) {
        long long k[3];
        in = md_cell(verts, v, L, k) ? 1u : 0u;
        key[v] = in ? (u64)((k[2] * L.g[1] + k[1]) * L.g[0] + k[0]) : behind;
        idx[v] = (int)v;
    }
    const unsigned s = tm_block_sum(in, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&totals[1], (u64)s);
}

__global__ __launch_bounds__(MD_BLOCK) void md_head_kernel(const u64* __restrict__ key, int n, u64 behind, unsigned char* __restrict__ head) {
    const long long i = gid();
    if (i < n) head[i] = (key[i] != behind && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
}

__global__ __launch_bounds__(MD_BLOCK) void md_emit_kernel(const u64* __restrict__ key, const int* __restrict__ idx, const unsigned char* __restrict__ head,
                                                           const int* __restrict__ head_rank, int n, u64 behind, const u64* __restrict__ totals,
                                                           int* __restrict__ cluster, int* __restrict__ order, int* __restrict__ cluster_start,
                                                           u64* __restrict__ cluster_key) {
    const long long i = gid();
    if (i == 0) {
        const u64 m = totals[0];
        if (m <= (u64)n) cluster_start[m] = (int)totals[1];
    }
    if (i >= n) return;
    const int v = idx[i];
    const u64 k = key[i];
    order[i] = v;
    if ((unsigned)v >= (unsigned)n) return;
    if (k == behind) { cluster[v] = -1; return; }
    const int r = head_rank[i] + (int)head[i] - 1;                // the heads up to and including i, less one
    cluster[v] = r;
    if (head[i] && r >= 0 && r < n) { cluster_start[r] = (int)i; cluster_key[r] = k; }
}

// ---- faces --------------------------------------------------------------------------------------------------------------------
constexpr int MD_EMPTY = -1;

__global__ __launch_bounds__(MD_BLOCK) void md_table_init_kernel(int* __restrict__ table, long long capacity, u64* __restrict__ counts) {
    for (long long i = gid(); i < capacity; i += (long long)gridDim.x * MD_BLOCK) table[i] = MD_EMPTY;
    if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0;
}

__device__ inline u64 md_hash(const int* r) {
    u64 h = (u64)(unsigned)r[0] * 0x9E3779B97F4A7C15ull;
    h ^= (u64)(unsigned)r[1] * 0xC2B2AE3D27D4EB4Full;
    h ^= (u64)(unsigned)r[2] * 0x165667B19E3779F9ull;
    return h ^ (h >> 29);
}

__global__ __launch_bounds__(MD_BLOCK) void md_face_map_kernel(const int* __restrict__ faces, int nv, int nf, const int* __restrict__ cluster,
                                                               int* __restrict__ cface, unsigned char* __restrict__ face_class, u64* counts) {
    __shared__ unsigned sh[MD_BLOCK];
    const long long f = gid();
    int cls = -1;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        int ca = -1, cb = -1, cc = -1;
        if (!mc::face_valid(a, b, c, nv)) {
            cls = RCMVS_MD_FACE_INVALID;
        } else {
            ca = cluster[a]; cb = cluster[b]; cc = cluster[c];
            if (ca < 0 || cb < 0 || cc < 0) cls = RCMVS_MD_FACE_UNCLUSTERED;
            else if (ca == cb || cb == cc || ca == cc) cls = RCMVS_MD_FACE_COLLAPSED;
            else cls = RCMVS_MD_FACE_KEPT;
        }
        cface[3 * f] = ca; cface[3 * f + 1] = cb; cface[3 * f + 2] = cc;
        face_class[f] = (unsigned char)cls;
    }
    for (int which = RCMVS_MD_FACE_INVALID; which <= RCMVS_MD_FACE_COLLAPSED; ++which) {
        const unsigned s = tm_block_sum(cls == which ? 1u : 0u, sh);
        if (threadIdx.x == 0 && s) atomicAdd(&counts[which - 1], (u64)s);
    }
}

__device__ inline bool md_same_triple(const int* __restrict__ cface, long long g, const int* r) {
    int o[3];
    md::rotate_min_first(cface[3 * g], cface[3 * g + 1], cface[3 * g + 2], o);
    return o[0] == r[0] && o[1] == r[1] && o[2] == r[2];
}

// Every candidate face walks its triple's probe sequence to the first slot that is empty (claimed by atomicCAS) or holds a face
// of the same triple (atomicMin).  A slot never changes its triple and is never emptied, so the walk of a triple passes the same
// slots in every order of execution; no thread waits: a failed CAS is another thread's success.
__global__ __launch_bounds__(MD_BLOCK) void md_face_insert_kernel(const int* __restrict__ cface, const unsigned char* __restrict__ face_class, int nf,
                                                                  int* table, long long capacity) {
    const long long f = gid();
    if (f >= nf || face_class[f] != RCMVS_MD_FACE_KEPT) return;
    int r[3];
    md::rotate_min_first(cface[3 * f], cface[3 * f + 1], cface[3 * f + 2], r);
    u64 slot = md_hash(r) & (u64)(capacity - 1);
    for (long long probe = 0; probe < capacity; ++probe, slot = (slot + 1) & (u64)(capacity - 1)) {
        const int old = atomicCAS(&table[slot], MD_EMPTY, (int)f);
        if (old == MD_EMPTY) return;
        if ((unsigned)old < (unsigned)nf && md_same_triple(cface, old, r)) {
            atomicMin(&table[slot], (int)f);
            return;
        }
    }
}

__global__ __launch_bounds__(MD_BLOCK) void md_face_resolve_kernel(const int* __restrict__ cface, unsigned char* __restrict__ face_class, int nf,
                                                                   const int* __restrict__ table, long long capacity, u64* counts) {
    __shared__ unsigned sh[MD_BLOCK];
    const long long f = gid();
    unsigned dup = 0;
    if (f < nf && face_class[f] == RCMVS_MD_FACE_KEPT) {
        int r[3];
        md::rotate_min_first(cface[3 * f], cface[3 * f + 1], cface[3 * f + 2], r);
        u64 slot = md_hash(r) & (u64)(capacity - 1);
        for (long long probe = 0; probe < capacity; ++probe, slot = (slot + 1) & (u64)(capacity - 1)) {
            const int first = table[slot];
            if (first == MD_EMPTY) break;
            if ((unsigned)first < (unsigned)nf && md_same_triple(cface, first, r)) {
                dup = first != (int)f;
                break;
            }
        }
        if (dup) face_class[f] = RCMVS_MD_FACE_DUPLICATE;
    }
    const unsigned s = tm_block_sum(dup, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&counts[3], (u64)s);
}

// ---- quadrics -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_BLOCK) void md_corner_key_kernel(const int* __restrict__ faces, int nv, long long n, const int* __restrict__ cluster, int m,
                                                                 unsigned* __restrict__ key, int* __restrict__ idx) {
    const long long e = gid();
    if (e >= n) return;
    const long long f = e / 3;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    unsigned k = (unsigned)m;
    if (mc::face_valid(a, b, c, nv)) {
        const int ca = cluster[a], cb = cluster[b], cc = cluster[c];
        const int mine = e - 3 * f == 0 ? ca : (e - 3 * f == 1 ? cb : cc);
        if ((unsigned)ca < (unsigned)m && (unsigned)cb < (unsigned)m && (unsigned)cc < (unsigned)m) k = (unsigned)mine;
    }
    key[e] = k;
    idx[e] = (int)e;
}

__device__ inline void md_key_cell(u64 key, const MdLattice& L, long long* k) {
    const u64 gx = (u64)L.g[0], gy = (u64)L.g[1];
    k[0] = (long long)(key % gx);
    k[1] = (long long)((key / gx) % gy);
    k[2] = (long long)(key / gx / gy);
}

__global__ __launch_bounds__(MD_BLOCK) void md_quadric_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, long long n,
                                                              const u64* __restrict__ cluster_key, int m, MdLattice L, const int* __restrict__ idx,
                                                              const int* __restrict__ seg, double* __restrict__ quad) {
    const long long r = gid();
    if (r >= m) return;
    long long k[3];
    md_key_cell(cluster_key[r], L, k);
    double ctr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ctr[a] = md::centre(L.org[a], k[a], L.cell);
    md::Quadric Q = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const long long s0 = seg[2 * r], s1 = seg[2 * r + 1];
    for (long long i = s0; i < s1 && i < n; ++i) {
        const long long e = idx[i];
        if (e < 0 || e >= n) continue;
        const long long f = e / 3;
        const int w[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        if (!mc::face_valid(w[0], w[1], w[2], nv)) continue;
        double q[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int a = 0; a < 3; ++a) q[c][a] = md::local(verts[3 * (size_t)w[c] + a], ctr[a], L.cell);
        }
        md::add_corner(Q, q[0], q[1], q[2]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) quad[9 * r + j] = Q.a[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) quad[9 * r + 6 + j] = Q.b[j];
}

// ---- placement ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_BLOCK) void md_place_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ rgb, int nv,
                                                            const int* __restrict__ order, const int* __restrict__ cluster_start,
                                                            const u64* __restrict__ cluster_key, int m, MdLattice L, const double* __restrict__ quad,
                                                            int placement, double reg, float* __restrict__ out_verts, unsigned char* __restrict__ out_rgb,
                                                            unsigned char* __restrict__ via_out, u64* counts) {
    __shared__ unsigned sh[MD_BLOCK];
    const long long r = gid();
    int via = -1;
    if (r < m) {
        const long long s0 = cluster_start[r], s1 = cluster_start[r + 1];
        bool ok = s0 >= 0 && s1 > s0 && s1 <= nv;
        long long k[3];
        md_key_cell(cluster_key[r], L, k);
        double ctr[3], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 3; ++a) ctr[a] = md::centre(L.org[a], k[a], L.cell);
        u64 col[3] = {0, 0, 0};
        for (long long i = s0; ok && i < s1; ++i) {
            const int v = order[i];
            if ((unsigned)v >= (unsigned)nv) { ok = false; break; }
#pragma unroll
            for (int a = 0; a < 3; ++a) sum[a] = sum[a] + md::local(verts[3 * (size_t)v + a], ctr[a], L.cell);
            if (out_rgb) {
#pragma unroll
                for (int a = 0; a < 3; ++a) col[a] += rgb[3 * (size_t)v + a];
            }
        }
        if (ok) {
            const double count = (double)(s1 - s0);
            double mean[3], x[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) mean[a] = sum[a] / count;
            via = md::VIA_MEAN;
            if (placement == RCMVS_MD_PLACE_QUADRIC) {
                md::Quadric Q;
#pragma unroll
                for (int j = 0; j < 6; ++j) Q.a[j] = quad[9 * r + j];
#pragma unroll
                for (int j = 0; j < 3; ++j) Q.b[j] = quad[9 * r + 6 + j];
                via = md::solve(Q, mean, reg, x);
            }
            if (via == md::VIA_QUADRIC) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_verts[3 * r + a] = md::world(ctr[a], L.cell, x[a]);
            } else if (s1 - s0 == 1) {                            // the mean of one member is that member, in every bit
                const unsigned* src = reinterpret_cast<const unsigned*>(verts) + 3 * (size_t)order[s0];
                unsigned* dst = reinterpret_cast<unsigned*>(out_verts) + 3 * r;
#pragma unroll
                for (int a = 0; a < 3; ++a) dst[a] = src[a];
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_verts[3 * r + a] = md::world(ctr[a], L.cell, mean[a]);
            }
            if (out_rgb) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_rgb[3 * r + a] = md::colour(col[a], (u64)(s1 - s0));
            }
            via_out[r] = (unsigned char)via;
        }
    }
    for (int which = md::VIA_NO_FACES; which <= md::VIA_OUTSIDE; ++which) {
        const unsigned s = tm_block_sum(via == which ? 1u : 0u, sh);
        if (threadIdx.x == 0 && s) atomicAdd(&counts[which - 1], (u64)s);
    }
}

// ---- select -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_BLOCK) void md_vert_init_kernel(unsigned char* __restrict__ vert_keep, int m, int drop) {
    const long long r = gid();
    if (r < m) vert_keep[r] = drop ? 0 : 1;
}

__global__ __launch_bounds__(MD_BLOCK) void md_face_keep_kernel(const int* __restrict__ cface, const unsigned char* __restrict__ face_class, int m, int nf,
                                                                int drop, unsigned char* __restrict__ face_keep, unsigned char* vert_keep) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = cface[3 * f], b = cface[3 * f + 1], c = cface[3 * f + 2];
    const bool keep = face_class[f] == RCMVS_MD_FACE_KEPT && mc::face_valid(a, b, c, m);
    face_keep[f] = keep ? 1 : 0;
    if (keep && drop) { vert_keep[a] = 1; vert_keep[b] = 1; vert_keep[c] = 1; }      // every writer stores the same value
}

static int md_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0 && nv <= RCMVS_MD_MAX_ELEMENTS, "%s: %d vertices (0 .. 2^31-256)", what, nv);
    RCMVS_REQUIRE(nf >= 0 && 3ll * nf <= RCMVS_MD_MAX_ELEMENTS, "%s: %d faces (0 .. (2^31-256) / 3)", what, nf);
    return 0;
}

static int md_lattice_args(const char* what, const double* lattice_host, const long long* dims_host, MdLattice* L) {
    RCMVS_REQUIRE(lattice_host && dims_host, "%s: null pointer", what);
    for (int a = 0; a < 3; ++a) { L->org[a] = lattice_host[a]; L->g[a] = dims_host[a]; }
    L->cell = lattice_host[3];
    RCMVS_REQUIRE(L->cell > 0.0 && std::isfinite(L->cell), "%s: cell = %g (finite, > 0)", what, L->cell);
    RCMVS_REQUIRE(std::isfinite(L->org[0]) && std::isfinite(L->org[1]) && std::isfinite(L->org[2]), "%s: lattice origin is not finite", what);
    for (int a = 0; a < 3; ++a)
        RCMVS_REQUIRE(L->g[a] >= 1 && L->g[a] <= RCMVS_MD_MAX_CELLS_PER_AXIS, "%s: %lld cells on axis %c (1 .. 2^21)", what, L->g[a], "xyz"[a]);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_md_bounds_timed(const float* verts, int nv, unsigned* bounds, void* ev0, void* ev1, void* stream) {
    if (int rc = md_sizes("md_bounds", nv, 0)) return rc;
    RCMVS_REQUIRE(bounds && (nv == 0 || verts), "md_bounds: null pointer");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    const unsigned grid = blocks(nv) < (unsigned)MD_BOUNDS_GRID ? blocks(nv) : (unsigned)MD_BOUNDS_GRID;
    RCMVS_LAUNCH_TIMED(md_bounds_init_kernel, dim3(1), dim3(MD_BLOCK), 0, st, e0, none, bounds);
    RCMVS_LAUNCH_TIMED(md_bounds_kernel, dim3(grid), dim3(MD_BLOCK), 0, st, none, e1, verts, nv, bounds);
    return launch_status("md_bounds");
}

extern "C" int rcmvs_md_bounds(const float* verts, int nv, unsigned* bounds, void* stream) {
    return rcmvs_md_bounds_timed(verts, nv, bounds, nullptr, nullptr, stream);
}

extern "C" int rcmvs_md_lattice(const float* lohi_host, double cell, double* lattice_host, long long* dims_host) {
    RCMVS_REQUIRE(lohi_host && lattice_host && dims_host, "md_lattice: null pointer");
    RCMVS_REQUIRE(cell > 0.0 && std::isfinite(cell), "md_lattice: cell = %g (finite, > 0)", cell);
    double org[3], g[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = lohi_host[a], hi = lohi_host[3 + a];
        RCMVS_REQUIRE(md::finite(lo) && md::finite(hi) && lo <= hi, "md_lattice: box %g .. %g on axis %c (finite, min <= max)", (double)lo, (double)hi,
                      "xyz"[a]);
        org[a] = md::origin(lo, cell);
        g[a] = md::cells(hi, org[a], cell);
        RCMVS_REQUIRE(std::isfinite(org[a]) && g[a] >= 1.0 && g[a] <= (double)RCMVS_MD_MAX_CELLS_PER_AXIS,
                      "md_lattice: %.0f cells on axis %c (1 .. 2^21): cell = %g does not fit the mesh's extent", g[a], "xyz"[a], cell);
    }
    for (int a = 0; a < 3; ++a) { lattice_host[a] = org[a]; dims_host[a] = (long long)g[a]; }
    lattice_host[3] = cell;
    return 0;
}

extern "C" int rcmvs_md_cluster_timed(const float* verts, int nv, const double* lattice_host, const long long* dims_host, u64* key_a, int* idx_a, u64* key_b,
                                      int* idx_b, int* hist, int* hist_start, int* scan_work, unsigned char* head, int* head_rank, int* cluster, int* order,
                                      int* cluster_start, u64* cluster_key, u64* totals, void* ev0, void* ev1, void* stream) {
    if (int rc = md_sizes("md_cluster", nv, 0)) return rc;
    MdLattice L;
    if (int rc = md_lattice_args("md_cluster", lattice_host, dims_host, &L)) return rc;
    RCMVS_REQUIRE(head_rank && cluster_start && totals &&
                  (nv == 0 || (verts && key_a && idx_a && key_b && idx_b && hist && hist_start && head && cluster && order && cluster_key)),
                  "md_cluster: null pointer");
    if (int rc = scan_work_check("md_cluster", scan_work)) return rc;
    const u64 behind = (u64)L.g[0] * (u64)L.g[1] * (u64)L.g[2];   // <= 2^63: the key of the vertices that are not clustered
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MD_BLOCK), 0, st, e0, none, totals, 2ll);
    hipLaunchKernelGGL(md_vertex_key_kernel, dim3(blocks(nv)), dim3(MD_BLOCK), 0, st, verts, nv, L, behind, key_a, idx_a, totals);
    radix_sort<u64>(&key_a, &idx_a, &key_b, &idx_b, nv, radix_passes(behind), hist, hist_start, scan_work, st);
    hipLaunchKernelGGL(md_head_kernel, dim3(blocks(nv)), dim3(MD_BLOCK), 0, st, key_a, nv, behind, head);
    scan3<unsigned char>(head, nv, head_rank, scan_work, totals, st, none, none);
    RCMVS_LAUNCH_TIMED(md_emit_kernel, dim3(blocks(nv)), dim3(MD_BLOCK), 0, st, none, e1, key_a, idx_a, head, head_rank, nv, behind, totals, cluster, order,
                       cluster_start, cluster_key);
    return launch_status("md_cluster");
}

extern "C" int rcmvs_md_cluster(const float* verts, int nv, const double* lattice_host, const long long* dims_host, u64* key_a, int* idx_a, u64* key_b,
                                int* idx_b, int* hist, int* hist_start, int* scan_work, unsigned char* head, int* head_rank, int* cluster, int* order,
                                int* cluster_start, u64* cluster_key, u64* totals, void* stream) {
    return rcmvs_md_cluster_timed(verts, nv, lattice_host, dims_host, key_a, idx_a, key_b, idx_b, hist, hist_start, scan_work, head, head_rank, cluster, order,
                                  cluster_start, cluster_key, totals, nullptr, nullptr, stream);
}

extern "C" int rcmvs_md_classify_faces_timed(const int* faces, int nv, int nf, const int* cluster, int* cface, unsigned char* face_class, int* table,
                                             long long table_capacity, u64* counts, void* ev0, void* ev1, void* stream) {
    if (int rc = md_sizes("md_classify_faces", nv, nf)) return rc;
    RCMVS_REQUIRE(counts && table && (nf == 0 || (faces && cface && face_class)) && (nv == 0 || cluster), "md_classify_faces: null pointer");
    RCMVS_REQUIRE(table_capacity > nf && table_capacity <= (1ll << 32) && (table_capacity & (table_capacity - 1)) == 0,
                  "md_classify_faces: table_capacity = %lld (a power of two above the %d faces)", table_capacity, nf);
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(md_table_init_kernel, dim3(capped_blocks(table_capacity)), dim3(MD_BLOCK), 0, st, e0, none, table, table_capacity, counts);
    hipLaunchKernelGGL(md_face_map_kernel, dim3(blocks(nf)), dim3(MD_BLOCK), 0, st, faces, nv, nf, cluster, cface, face_class, counts);
    hipLaunchKernelGGL(md_face_insert_kernel, dim3(blocks(nf)), dim3(MD_BLOCK), 0, st, cface, face_class, nf, table, table_capacity);
    RCMVS_LAUNCH_TIMED(md_face_resolve_kernel, dim3(blocks(nf)), dim3(MD_BLOCK), 0, st, none, e1, cface, face_class, nf, table, table_capacity, counts);
    return launch_status("md_classify_faces");
}

extern "C" int rcmvs_md_classify_faces(const int* faces, int nv, int nf, const int* cluster, int* cface, unsigned char* face_class, int* table,
                                       long long table_capacity, u64* counts, void* stream) {
    return rcmvs_md_classify_faces_timed(faces, nv, nf, cluster, cface, face_class, table, table_capacity, counts, nullptr, nullptr, stream);
}

extern "C" int rcmvs_md_quadrics_timed(const float* verts, const int* faces, int nv, int nf, const int* cluster, const u64* cluster_key, int m,
                                       const double* lattice_host, const long long* dims_host, unsigned* ckey_a, int* cidx_a, unsigned* ckey_b, int* cidx_b,
                                       int* hist, int* hist_start, int* scan_work, int* seg, double* quad, void* ev0, void* ev1, void* stream) {
    if (int rc = md_sizes("md_quadrics", nv, nf)) return rc;
    RCMVS_REQUIRE(m >= 1 && m <= nv, "md_quadrics: m = %d clusters (1 .. the %d vertices)", m, nv);
    MdLattice L;
    if (int rc = md_lattice_args("md_quadrics", lattice_host, dims_host, &L)) return rc;
    RCMVS_REQUIRE(verts && cluster && cluster_key && seg && quad && (nf == 0 || (faces && ckey_a && cidx_a && ckey_b && cidx_b && hist && hist_start)),
                  "md_quadrics: null pointer");
    if (int rc = scan_work_check("md_quadrics", scan_work)) return rc;
    const long long n = 3ll * nf;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<int>, dim3(blocks(2ll * m)), dim3(MD_BLOCK), 0, st, e0, none, seg, 2ll * m);
    hipLaunchKernelGGL(md_corner_key_kernel, dim3(blocks(n)), dim3(MD_BLOCK), 0, st, faces, nv, n, cluster, m, ckey_a, cidx_a);
    radix_sort<unsigned>(&ckey_a, &cidx_a, &ckey_b, &cidx_b, n, radix_passes((u64)m), hist, hist_start, scan_work, st);
    hipLaunchKernelGGL(segments_kernel, dim3(blocks(n)), dim3(MD_BLOCK), 0, st, ckey_a, n, m, seg);
    RCMVS_LAUNCH_TIMED(md_quadric_kernel, dim3(blocks(m)), dim3(MD_BLOCK), 0, st, none, e1, verts, faces, nv, n, cluster_key, m, L, cidx_a, seg, quad);
    return launch_status("md_quadrics");
}

extern "C" int rcmvs_md_quadrics(const float* verts, const int* faces, int nv, int nf, const int* cluster, const u64* cluster_key, int m,
                                 const double* lattice_host, const long long* dims_host, unsigned* ckey_a, int* cidx_a, unsigned* ckey_b, int* cidx_b, int* hist,
                                 int* hist_start, int* scan_work, int* seg, double* quad, void* stream) {
    return rcmvs_md_quadrics_timed(verts, faces, nv, nf, cluster, cluster_key, m, lattice_host, dims_host, ckey_a, cidx_a, ckey_b, cidx_b, hist, hist_start,
                                   scan_work, seg, quad, nullptr, nullptr, stream);
}

extern "C" int rcmvs_md_place_timed(const float* verts, const unsigned char* rgb, int nv, const int* order, const int* cluster_start, const u64* cluster_key,
                                    int m, const double* lattice_host, const long long* dims_host, const double* quad, int placement, double reg,
                                    float* out_verts, unsigned char* out_rgb, unsigned char* via, u64* counts, void* ev0, void* ev1, void* stream) {
    if (int rc = md_sizes("md_place", nv, 0)) return rc;
    RCMVS_REQUIRE(m >= 0 && m <= nv, "md_place: m = %d clusters (0 .. the %d vertices)", m, nv);
    MdLattice L;
    if (int rc = md_lattice_args("md_place", lattice_host, dims_host, &L)) return rc;
    RCMVS_REQUIRE(placement == RCMVS_MD_PLACE_QUADRIC || placement == RCMVS_MD_PLACE_MEAN, "md_place: placement = %d (0 quadric, 1 mean)", placement);
    RCMVS_REQUIRE(reg >= 0.0 && std::isfinite(reg), "md_place: reg = %g (finite, >= 0)", reg);
    RCMVS_REQUIRE(counts && cluster_start && (m == 0 || (verts && order && cluster_key && out_verts && via)), "md_place: null pointer");
    RCMVS_REQUIRE(placement == RCMVS_MD_PLACE_MEAN || m == 0 || quad, "md_place: null pointer (quadric placement needs quad)");
    RCMVS_REQUIRE(!out_rgb || rgb, "md_place: null pointer (out_rgb needs rgb)");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MD_BLOCK), 0, st, e0, none, counts, 3ll);
    RCMVS_LAUNCH_TIMED(md_place_kernel, dim3(blocks(m)), dim3(MD_BLOCK), 0, st, none, e1, verts, rgb, nv, order, cluster_start, cluster_key, m, L, quad,
                       placement, reg, out_verts, out_rgb, via, counts);
    return launch_status("md_place");
}

extern "C" int rcmvs_md_place(const float* verts, const unsigned char* rgb, int nv, const int* order, const int* cluster_start, const u64* cluster_key, int m,
                              const double* lattice_host, const long long* dims_host, const double* quad, int placement, double reg, float* out_verts,
                              unsigned char* out_rgb, unsigned char* via, u64* counts, void* stream) {
    return rcmvs_md_place_timed(verts, rgb, nv, order, cluster_start, cluster_key, m, lattice_host, dims_host, quad, placement, reg, out_verts, out_rgb, via,
                                counts, nullptr, nullptr, stream);
}

extern "C" int rcmvs_md_select_timed(const int* cface, const unsigned char* face_class, int m, int nf, int drop_unreferenced, unsigned char* face_keep,
                                     unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, u64* totals, void* ev0, void* ev1,
                                     void* stream) {
    if (int rc = md_sizes("md_select", m, nf)) return rc;
    RCMVS_REQUIRE(face_rank && vert_rank && totals && (nf == 0 || (cface && face_class && face_keep)) && (m == 0 || vert_keep), "md_select: null pointer");
    if (int rc = scan_work_check("md_select", scan_work)) return rc;
    const int drop = drop_unreferenced != 0;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(md_vert_init_kernel, dim3(blocks(m)), dim3(MD_BLOCK), 0, st, e0, none, vert_keep, m, drop);
    hipLaunchKernelGGL(md_face_keep_kernel, dim3(blocks(nf)), dim3(MD_BLOCK), 0, st, cface, face_class, m, nf, drop, face_keep, vert_keep);
    scan3<unsigned char>(face_keep, nf, face_rank, scan_work, totals, st, none, none);
    scan3<unsigned char>(vert_keep, m, vert_rank, scan_work, totals + 1, st, none, e1);
    return launch_status("md_select");
}

extern "C" int rcmvs_md_select(const int* cface, const unsigned char* face_class, int m, int nf, int drop_unreferenced, unsigned char* face_keep,
                               unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, u64* totals, void* stream) {
    return rcmvs_md_select_timed(cface, face_class, m, nf, drop_unreferenced, face_keep, vert_keep, face_rank, vert_rank, scan_work, totals, nullptr, nullptr,
                                 stream);
}
