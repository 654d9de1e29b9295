// Hole filling of a triangle mesh: the boundary half-edges, the closed loops they form, a fan over every loop of at most max_edges
// edges (rc_mvsnet_amd/mesh_holes.py; contract in mesh_holes.h, the per-element rules in mesh_holes_math.h).
//
//   boundary   one thread per face corner: the multiplicity of its edge by bisection in the tail's sorted 1-ring segment
//              (mesh_clean's CSR); a boundary half-edge adds 1 to out[tail] and in[head] and stores succ[tail] / pred[head] with
//              plain stores.  A second launch classifies every vertex and writes -1 where it is not simple, so a store that raced
//              at a complex vertex never shows.
//   leaders    one thread per vertex; a simple vertex smaller than its successor and its predecessor walks the finished succ
//              array until it meets a smaller vertex, a -1, itself, or has made max_edges steps.  Nothing is written that the
//              launch reads.  Then block sums of the loop statistics, one integer atomic each per block.
//   scan       counts -> exclusive prefix sums in three levels: scan_sort.hip's scan3.
//   emit       bit copies of the input, then one lane per leader walks its loop once more: fp64 sum in loop order, integer colour
//              sums, the faces at the ranks the scans gave.
// No kernel reads a cell that another workgroup of the same launch writes, none waits for another workgroup, and there are no
// floating-point atomics.  gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_holes.h"
#include "mesh_holes_math.h"
#include "scan_sort.h"                                            // gid, blocks, ranges_overlap, scan3, zero_kernel
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MH_BLOCK = TM_BLOCK;
static_assert(MH_BLOCK == SS_BLOCK, "gid, blocks and zero_kernel count in this family's block");
static_assert(RCMVS_MH_SCAN_TILE == SS_TILE && RCMVS_MH_SCAN_WORK == SS_WORK, "mesh_holes.h describes scan_sort.h's work area");
static_assert(mh::NONE == RCMVS_MH_NONE && mh::SIMPLE == RCMVS_MH_SIMPLE && mh::COMPLEX == RCMVS_MH_COMPLEX, "the flags of mesh_holes.h");

using u64 = unsigned long long;

// ---- boundary -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MH_BLOCK) void mh_init_kernel(int nv, int* __restrict__ out_count, int* __restrict__ in_count, int* __restrict__ succ,
                                                           int* __restrict__ pred, u64* __restrict__ counts) {
    const long long v = gid();
    if (v < nv) { out_count[v] = 0; in_count[v] = 0; succ[v] = -1; pred[v] = -1; }
    if (v < 2) counts[v] = 0;
}

// the multiplicity of the edge {v, w} in v's segment (distinct neighbours ascending), 0 when the segment does not hold w
__device__ inline int mh_multiplicity(int v, int w, const int* __restrict__ row_start, const int* __restrict__ row_len, const int* __restrict__ nbr,
                                      const int* __restrict__ mult, long long entries) {
    const long long s0 = row_start[v];
    const int len = row_len[v];
    if (s0 < 0 || len <= 0 || s0 + len > entries) return 0;
    int lo = 0, hi = len;                                         // the first entry >= w
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (nbr[s0 + mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && nbr[s0 + lo] == w ? mult[s0 + lo] : 0;
}

// One thread per face corner e = 3 f + k: the half-edge from the face's k-th index to its next.  An edge of multiplicity 1 lies in
// one valid face, so exactly one corner finds it: succ[v] has one writer when out[v] == 1 and pred[w] one when in[w] == 1.
__global__ __launch_bounds__(MH_BLOCK) void mh_half_edge_kernel(const int* __restrict__ faces, int nv, long long corners, const int* __restrict__ row_start,
                                                                const int* __restrict__ row_len, const int* __restrict__ nbr, const int* __restrict__ mult,
                                                                long long entries, int* out_count, int* in_count, int* succ, int* pred) {
    const long long e = gid();
    if (e >= corners) return;
    const long long f = e / 3;
    const int k = (int)(e - 3 * f);
    const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (!mc::face_valid(idx[0], idx[1], idx[2], nv)) return;
    const int v = idx[k], w = idx[(k + 1) % 3];
    if (mh_multiplicity(v, w, row_start, row_len, nbr, mult, entries) != 1) return;
    atomicAdd(&out_count[v], 1);
    atomicAdd(&in_count[w], 1);
    succ[v] = w;
    pred[w] = v;
}

__global__ __launch_bounds__(MH_BLOCK) void mh_classify_kernel(int nv, const int* __restrict__ out_count, const int* __restrict__ in_count,
                                                               int* __restrict__ succ, int* __restrict__ pred, unsigned char* __restrict__ flags, u64* counts) {
    __shared__ unsigned sh[MH_BLOCK];
    const long long v = gid();
    unsigned leaving = 0, complex_here = 0;
    if (v < nv) {
        const int o = out_count[v], cls = mh::classify(o, in_count[v]);
        flags[v] = (unsigned char)cls;
        if (cls != mh::SIMPLE) { succ[v] = -1; pred[v] = -1; }
        leaving = (unsigned)o;
        complex_here = cls == mh::COMPLEX;
    }
    const unsigned b = tm_block_sum(leaving, sh), c = tm_block_sum(complex_here, sh);
    if (threadIdx.x == 0) {
        if (b) atomicAdd(&counts[0], (u64)b);
        if (c) atomicAdd(&counts[1], (u64)c);
    }
}

// ---- leaders ------------------------------------------------------------------------------------------------------------------
// The length of the loop that v leads, 0 when v leads none of at most max_edges edges.  succ and pred are only read.  A vertex
// that is not simple has succ == pred == -1 and fails the first test; the walk leaves a loop's vertices only through a -1.
__device__ inline int mh_loop_length(const int* __restrict__ succ, const int* __restrict__ pred, int nv, int v, int max_edges) {
    int cur = succ[v];
    if (cur <= v || pred[v] <= v) return 0;
    for (int steps = 1; steps <= max_edges; ++steps) {
        if (cur == v) return steps >= 3 ? steps : 0;
        if (cur < v || cur >= nv) return 0;                       // a smaller vertex leads this loop, if it is one; -1 ends a chain
        cur = succ[cur];
    }
    return 0;
}

__global__ __launch_bounds__(MH_BLOCK) void mh_leader_kernel(const int* __restrict__ succ, const int* __restrict__ pred, int nv, int max_edges,
                                                             int* __restrict__ loop_len, unsigned char* __restrict__ vert_count, int* __restrict__ face_count,
                                                             u64* totals) {
    __shared__ unsigned sh[MH_BLOCK];
    const long long v = gid();
    int L = 0;
    if (v < nv) {
        L = mh_loop_length(succ, pred, nv, (int)v, max_edges);
        loop_len[v] = L;
        vert_count[v] = (unsigned char)(L ? mh::verts_added(L) : 0);
        face_count[v] = L ? mh::faces_added(L) : 0;
    }
    const unsigned loops = tm_block_sum(L > 0, sh), single = tm_block_sum(L == 3, sh);
    sh[threadIdx.x] = (unsigned)L;
    __syncthreads();
    for (int o = MH_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && sh[threadIdx.x + o] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (loops) atomicAdd(&totals[2], (u64)loops);
        if (single) atomicAdd(&totals[3], (u64)single);
        if (sh[0]) atomicMax(&totals[4], (u64)sh[0]);
    }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(MH_BLOCK) void mh_copy_kernel(const T* __restrict__ src, long long n, T* __restrict__ dst) {
    for (long long i = gid(); i < n; i += (long long)gridDim.x * MH_BLOCK) dst[i] = src[i];
}

// One lane per leader.  The chain of succ is a chain of dependent loads whatever walks it, and the fp64 sum is in loop order, so
// a wave per loop would only share out the stores of the L faces.
__global__ __launch_bounds__(MH_BLOCK) void mh_fan_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ rgb, int nv, int nf,
                                                          const int* __restrict__ succ, const int* __restrict__ loop_len, const int* __restrict__ vert_rank,
                                                          const int* __restrict__ face_rank, int nv_out, int nf_out, float* __restrict__ out_verts,
                                                          unsigned char* __restrict__ out_rgb, int* __restrict__ out_faces) {
    const long long v = gid();
    if (v >= nv) return;
    const int L = loop_len[v];
    if (L < 3 || L > RCMVS_MH_MAX_EDGES) return;
    const long long f0 = (long long)nf + face_rank[v];
    if (f0 < nf || f0 + mh::faces_added(L) > nf_out) return;
    if (L == 3) {
        const int u1 = succ[v];
        if ((unsigned)u1 >= (unsigned)nv) return;
        const int u2 = succ[u1];
        if ((unsigned)u2 >= (unsigned)nv) return;
        out_faces[3 * f0] = (int)v;
        out_faces[3 * f0 + 1] = u2;
        out_faces[3 * f0 + 2] = u1;
        return;
    }
    const long long c = (long long)nv + vert_rank[v];
    if (c < nv || c >= nv_out) return;
    double s[3] = {0.0, 0.0, 0.0};
    u64 col[3] = {0, 0, 0};
    int cur = (int)v;
    for (int i = 0; i < L; ++i) {
        const int nxt = succ[cur];
        if ((unsigned)nxt >= (unsigned)nv) return;                // not a loop of this mesh: its vertex is not written
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = mh::add_member(s[a], verts[3 * (size_t)cur + a]);
        if (out_rgb) {
#pragma unroll
            for (int a = 0; a < 3; ++a) col[a] += rgb[3 * (size_t)cur + a];
        }
        out_faces[3 * (f0 + i)] = nxt;
        out_faces[3 * (f0 + i) + 1] = cur;
        out_faces[3 * (f0 + i) + 2] = (int)c;
        cur = nxt;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out_verts[3 * c + a] = mh::centroid(s[a], L);
    if (out_rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out_rgb[3 * c + a] = md::colour(col[a], (u64)L);
    }
}

static int mh_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0 && nf >= 0, "%s: %d vertices, %d faces (0 .. 2^31-1 each)", what, nv, nf);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_mh_boundary_timed(const int* faces, int nv, int nf, const int* row_start, const int* row_len, const int* nbr, const int* mult,
                                       long long entries, int* out_count, int* in_count, int* succ, int* pred, unsigned char* flags, u64* counts, void* ev0,
                                       void* ev1, void* stream) {
    if (int rc = mh_sizes("mh_boundary", nv, nf)) return rc;
    RCMVS_REQUIRE(entries >= 0 && entries <= 2147483647ll, "mh_boundary: %lld entries (0 .. 2^31-1)", entries);
    RCMVS_REQUIRE(counts && (nf == 0 || faces) && (nv == 0 || (row_start && row_len && out_count && in_count && succ && pred && flags)) &&
                  (entries == 0 || (nbr && mult)), "mh_boundary: null pointer");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(mh_init_kernel, dim3(blocks(nv)), dim3(MH_BLOCK), 0, st, e0, none, nv, out_count, in_count, succ, pred, counts);
    hipLaunchKernelGGL(mh_half_edge_kernel, dim3(blocks(3ll * nf)), dim3(MH_BLOCK), 0, st, faces, nv, 3ll * nf, row_start, row_len, nbr, mult, entries,
                       out_count, in_count, succ, pred);
    RCMVS_LAUNCH_TIMED(mh_classify_kernel, dim3(blocks(nv)), dim3(MH_BLOCK), 0, st, none, e1, nv, out_count, in_count, succ, pred, flags, counts);
    return launch_status("mh_boundary");
}

extern "C" int rcmvs_mh_boundary(const int* faces, int nv, int nf, const int* row_start, const int* row_len, const int* nbr, const int* mult, long long entries,
                                 int* out_count, int* in_count, int* succ, int* pred, unsigned char* flags, u64* counts, void* stream) {
    return rcmvs_mh_boundary_timed(faces, nv, nf, row_start, row_len, nbr, mult, entries, out_count, in_count, succ, pred, flags, counts, nullptr, nullptr,
                                   stream);
}

extern "C" int rcmvs_mh_leaders_timed(const int* succ, const int* pred, int nv, int max_edges, int* loop_len, unsigned char* vert_count, int* face_count,
                                      int* vert_rank, int* face_rank, int* scan_work, u64* totals, void* ev0, void* ev1, void* stream) {
    if (int rc = mh_sizes("mh_leaders", nv, 0)) return rc;
    RCMVS_REQUIRE(max_edges >= 3 && max_edges <= RCMVS_MH_MAX_EDGES, "mh_leaders: max_edges = %d (3 .. %d)", max_edges, RCMVS_MH_MAX_EDGES);
    RCMVS_REQUIRE(vert_rank && face_rank && totals && scan_work && (nv == 0 || (succ && pred && loop_len && vert_count && face_count)),
                  "mh_leaders: null pointer");
    if (int rc = scan_work_check("mh_leaders", scan_work)) return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MH_BLOCK), 0, st, e0, none, totals, 5ll);
    hipLaunchKernelGGL(mh_leader_kernel, dim3(blocks(nv)), dim3(MH_BLOCK), 0, st, succ, pred, nv, max_edges, loop_len, vert_count, face_count, totals);
    scan3<unsigned char>(vert_count, nv, vert_rank, scan_work, totals, st, none, none);
    scan3<int>(face_count, nv, face_rank, scan_work, totals + 1, st, none, e1);
    return launch_status("mh_leaders");
}

extern "C" int rcmvs_mh_leaders(const int* succ, const int* pred, int nv, int max_edges, int* loop_len, unsigned char* vert_count, int* face_count,
                                int* vert_rank, int* face_rank, int* scan_work, u64* totals, void* stream) {
    return rcmvs_mh_leaders_timed(succ, pred, nv, max_edges, loop_len, vert_count, face_count, vert_rank, face_rank, scan_work, totals, nullptr, nullptr,
                                  stream);
}

extern "C" int rcmvs_mh_emit_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, const int* succ, const int* loop_len,
                                   const int* vert_rank, const int* face_rank, int nv_out, int nf_out, float* out_verts, unsigned char* out_rgb,
                                   int* out_faces, void* ev0, void* ev1, void* stream) {
    if (int rc = mh_sizes("mh_emit", nv, nf)) return rc;
    RCMVS_REQUIRE(nv_out >= nv && nf_out >= nf, "mh_emit: %d of %d vertices, %d of %d faces out (no fewer than the input's)", nv_out, nv, nf_out, nf);
    RCMVS_REQUIRE((nv == 0 || (verts && succ && loop_len && vert_rank && face_rank)) && (nf == 0 || faces) && (nv_out == 0 || out_verts) &&
                  (nf_out == 0 || out_faces), "mh_emit: null pointer");
    RCMVS_REQUIRE(!out_rgb || rgb || nv == 0, "mh_emit: null pointer (out_rgb needs rgb)");
    RCMVS_REQUIRE(!ranges_overlap(verts, (size_t)nv * 12, out_verts, (size_t)nv_out * 12) && !ranges_overlap(faces, (size_t)nf * 12, out_faces, (size_t)nf_out * 12) &&
                  !ranges_overlap(rgb, (size_t)nv * 3, out_rgb, (size_t)nv_out * 3), "mh_emit: an output overlaps its input");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    const long long wv = 3ll * nv, wf = 3ll * nf;
    RCMVS_LAUNCH_TIMED(mh_copy_kernel<unsigned>, dim3(capped_blocks(wv)), dim3(MH_BLOCK), 0, st, e0, none, reinterpret_cast<const unsigned*>(verts), wv,
                       reinterpret_cast<unsigned*>(out_verts));
    hipLaunchKernelGGL(mh_copy_kernel<int>, dim3(capped_blocks(wf)), dim3(MH_BLOCK), 0, st, faces, wf, out_faces);
    if (out_rgb) hipLaunchKernelGGL(mh_copy_kernel<unsigned char>, dim3(capped_blocks(wv)), dim3(MH_BLOCK), 0, st, rgb, wv, out_rgb);
    RCMVS_LAUNCH_TIMED(mh_fan_kernel, dim3(blocks(nv)), dim3(MH_BLOCK), 0, st, none, e1, verts, rgb, nv, nf, succ, loop_len, vert_rank, face_rank, nv_out,
                       nf_out, out_verts, out_rgb, out_faces);
    return launch_status("mh_emit");
}

extern "C" int rcmvs_mh_emit(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, const int* succ, const int* loop_len,
                             const int* vert_rank, const int* face_rank, int nv_out, int nf_out, float* out_verts, unsigned char* out_rgb, int* out_faces,
                             void* stream) {
    return rcmvs_mh_emit_timed(verts, rgb, faces, nv, nf, succ, loop_len, vert_rank, face_rank, nv_out, nf_out, out_verts, out_rgb, out_faces, nullptr, nullptr,
                               stream);
}
