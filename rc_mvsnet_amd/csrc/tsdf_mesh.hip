// TSDF fusion of depth maps into a dense voxel grid and marching-tetrahedra extraction of its zero surface
// (rc_mvsnet_amd/tsdf_mesh.py; contract in tsdf_mesh.h, arithmetic and the 16-case table in tsdf_mesh_math.h).
//
//   integrate  One thread per voxel.  It reads its state (dsum, wsum, three colour sums) once, walks the chunk's views in order
//              with the state in registers -- per view some thirty fp64 operations, one depth gather, one fp32 add -- and
//              writes the state once: the planes cross HBM once per chunk of up to 16 views, not once per view.  The cameras
//              travel as one kernel argument (uniform loads).  No atomics: a voxel has one owner.
//   count      A block owns a tile of RCMVS_TSDF_SCAN_TILE voxels, a thread eight of them, 256 apart.  Per voxel the 7-bit mask of
//              its edges that carry a vertex and the number of triangles of its cube, both as bytes, and the tile's two sums.
//   scan       Three levels, because 2^28 voxels are 2^17 tiles: tile sums (32 bit, a tile holds at most 2048 * 12), sums of
//              2048 tile sums and their scan in 64 bits by one thread per array (at most 64 of them), then the two levels back down.
//              The totals are exact in 64 bits; the 32-bit starts wrap when a total passes 2^32 and the caller refuses those.
//   emit       One thread per voxel: its vertices at vert_start + rank, its cube's triangles at tri_start, a triangle's vertex
//              looked up through the owner's start and the popcount of the owner's lower mask bits.
// gfx950 only; __syncthreads and plain loads and stores (tests/emu compiles this file too).
#include <cstdint>

#include "common.h"
#include "tsdf_mesh.h"
#include "tsdf_mesh_math.h"
#include "tsdf_mesh_cells.h"

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int TM_TOP = 64;                                        // at most ceil(2^28 / 2048 / 2048) sums at the top level

// ---- integrate --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_integrate_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ rgb, int n, int H,
                                                                  int W, tsdf::Cams cams, double trunc, tsdf::Grid g, int voxels,
                                                                  float* __restrict__ dsum, float* __restrict__ wsum, float* __restrict__ cr,
                                                                  float* __restrict__ cg, float* __restrict__ cb) {
    const long long id = (long long)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (id >= voxels) return;
    const int v = (int)id;
    const int i = v % g.gx, j = (v / g.gx) % g.gy, k = v / (g.gx * g.gy);
    const double px = tsdf::centre(g.ox, i, g.h), py = tsdf::centre(g.oy, j, g.h), pz = tsdf::centre(g.oz, k, g.h);
    const bool colour = rgb != nullptr && cr != nullptr;
    float d = dsum[v], w = wsum[v], r = 0.0f, gr = 0.0f, b = 0.0f;
    if (colour) { r = cr[v]; gr = cg[v]; b = cb[v]; }
    const TmState s = tm_integrate_voxel(depth, rgb, n, H, W, cams, trunc, px, py, pz, colour, TmState{d, w, r, gr, b});
    dsum[v] = s.d;
    wsum[v] = s.w;
    if (colour) { cr[v] = s.r; cg[v] = s.g; cb[v] = s.b; }
}

// ---- the field as the extraction sees it ------------------------------------------------------------------------------------
struct TmDims {
    int gx, gy, gz;
};

// the flags of the eight voxels at codes 0..7 from (i, j, k); a neighbour beyond the grid is unobserved
__device__ inline void tm_corner_flags(const float* __restrict__ dsum, const float* __restrict__ wsum, TmDims g, int i, int j, int k, float min_weight,
                                       int* f) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ii = i + (c & 1), jj = j + ((c >> 1) & 1), kk = k + (c >> 2);
        f[c] = (ii < g.gx && jj < g.gy && kk < g.gz) ? tm_flags(dsum, wsum, ii + g.gx * (jj + g.gy * kk), min_weight) : 0;
    }
}

// ---- count ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_count_kernel(const float* __restrict__ dsum, const float* __restrict__ wsum, TmDims g, int voxels,
                                                              float min_weight, unsigned char* __restrict__ edge_mask,
                                                              unsigned char* __restrict__ tri_count, unsigned* __restrict__ tile_v,
                                                              unsigned* __restrict__ tile_t) {
    __shared__ unsigned sh[TM_BLOCK];
    const long long base = (long long)blockIdx.x * TM_TILE + threadIdx.x;           // only the tile's sums are needed here, so a thread
    unsigned nv = 0, nt = 0;                                                        // takes every 256th voxel: neighbouring lanes, neighbouring voxels
    for (int q = 0; q < TM_PER; ++q) {
        if (base + (long long)q * TM_BLOCK >= voxels) break;
        const int v = (int)(base + (long long)q * TM_BLOCK);
        const int i = v % g.gx, j = (v / g.gx) % g.gy, k = v / (g.gx * g.gy);
        int f[8];
        tm_corner_flags(dsum, wsum, g, i, j, k, min_weight, f);
        const unsigned m = tm_edge_mask(f);
        unsigned t = 0;
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) t += tsdf::tet_case(tm_tet_case(f, tet)).n;   // a cube beyond the grid has an unobserved corner
        edge_mask[v] = (unsigned char)m;
        tri_count[v] = (unsigned char)t;
        nv += (unsigned)tsdf::popcount7(m);
        nt += t;
    }
    const unsigned sv = tm_block_sum(nv, sh), st = tm_block_sum(nt, sh);
    if (threadIdx.x == 0) { tile_v[blockIdx.x] = sv; tile_t[blockIdx.x] = st; }
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_scan_down_kernel(const unsigned char* __restrict__ edge_mask, const unsigned char* __restrict__ tri_count,
                                                                  int voxels, const unsigned* __restrict__ tile_v, const unsigned* __restrict__ tile_t,
                                                                  const unsigned long long* __restrict__ totals, int* __restrict__ vert_start,
                                                                  int* __restrict__ tri_start) {
    __shared__ unsigned sh[TM_BLOCK];
    const long long base = (long long)blockIdx.x * TM_TILE + (long long)threadIdx.x * TM_PER;
    unsigned cv[TM_PER], ct[TM_PER], sv = 0, st = 0;
#pragma unroll
    for (int q = 0; q < TM_PER; ++q) {
        const bool in = base + q < voxels;
        cv[q] = in ? (unsigned)tsdf::popcount7(edge_mask[base + q]) : 0u;
        ct[q] = in ? (unsigned)tri_count[base + q] : 0u;
        sv += cv[q];
        st += ct[q];
    }
    unsigned rv = tm_block_exclusive(sv, sh) + tile_v[blockIdx.x];
    unsigned rt = tm_block_exclusive(st, sh) + tile_t[blockIdx.x];
#pragma unroll
    for (int q = 0; q < TM_PER; ++q) {
        if (base + q < voxels) { vert_start[base + q] = (int)rv; tri_start[base + q] = (int)rt; }
        rv += cv[q];
        rt += ct[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { vert_start[voxels] = (int)(unsigned)totals[0]; tri_start[voxels] = (int)(unsigned)totals[1]; }
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_emit_kernel(const float* __restrict__ dsum, const float* __restrict__ wsum, const float* __restrict__ cr,
                                                             const float* __restrict__ cg, const float* __restrict__ cb, tsdf::Grid g, int voxels,
                                                             float min_weight, const unsigned char* __restrict__ edge_mask,
                                                             const unsigned char* __restrict__ tri_count, const int* __restrict__ vert_start,
                                                             const int* __restrict__ tri_start, int nv, int nf, float* __restrict__ verts,
                                                             unsigned char* __restrict__ vert_rgb, int* __restrict__ faces) {
    const long long id = (long long)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (id >= voxels) return;
    const int v = (int)id;
    const unsigned mask = edge_mask[v];
    const int ntri = tri_count[v];
    if (mask == 0 && ntri == 0) return;
    const int i = v % g.gx, j = (v / g.gx) % g.gy, k = v / (g.gx * g.gy);
    if (mask) {
        const double wa = (double)wsum[v], da = (double)dsum[v] / wa;
        const double pa[3] = {tsdf::centre(g.ox, i, g.h), tsdf::centre(g.oy, j, g.h), tsdf::centre(g.oz, k, g.h)};
        int at = vert_start[v];
        for (int c = 1; c < 8; ++c) {
            if (!((mask >> (c - 1)) & 1)) continue;
            const int ii = i + (c & 1), jj = j + ((c >> 1) & 1), kk = k + (c >> 2);
            if (ii >= g.gx || jj >= g.gy || kk >= g.gz) continue;                        // never with the count kernel's masks
            const int u = ii + g.gx * (jj + g.gy * kk);
            const double wb = (double)wsum[u], db = (double)dsum[u] / wb;
            const double t = tsdf::crossing(da, db);
            const double pb[3] = {tsdf::centre(g.ox, ii, g.h), tsdf::centre(g.oy, jj, g.h), tsdf::centre(g.oz, kk, g.h)};
            if (at >= 0 && at < nv) {
#pragma unroll
                for (int a = 0; a < 3; ++a) verts[(size_t)at * 3 + a] = (float)tsdf::lerp(pa[a], pb[a], t);
                if (vert_rgb) {
                    vert_rgb[(size_t)at * 3 + 0] = tsdf::colour_byte((double)cr[v] / wa, (double)cr[u] / wb, t);
                    vert_rgb[(size_t)at * 3 + 1] = tsdf::colour_byte((double)cg[v] / wa, (double)cg[u] / wb, t);
                    vert_rgb[(size_t)at * 3 + 2] = tsdf::colour_byte((double)cb[v] / wa, (double)cb[u] / wb, t);
                }
            }
            ++at;
        }
    }
    if (ntri) {                                                     // the cube at (i, j, k) lies inside the grid: its eight corners are observed voxels
        const TmDims d = {g.gx, g.gy, g.gz};
        int f[8];
        tm_corner_flags(dsum, wsum, d, i, j, k, min_weight, f);
        int at = tri_start[v];
        for (int tet = 0; tet < 6; ++tet) {
            const int m = tm_tet_case(f, tet);
            const tsdf::TetCase tc = tsdf::tet_case(m);
            const bool swap = tsdf::tet_sign(tet) < 0;
            for (int q = 0; q < tc.n; ++q) {
                int idx[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int code = tc.e[3 * q + (e == 0 ? 0 : (swap ? 3 - e : e))];
                    const int ca = tsdf::tet_corner(tet, code >> 2), cb2 = tsdf::tet_corner(tet, code & 3);
                    const int owner = (i + (ca & 1)) + g.gx * ((j + ((ca >> 1) & 1)) + g.gy * (k + (ca >> 2)));
                    const unsigned lower = (1u << ((cb2 ^ ca) - 1)) - 1u;
                    idx[e] = vert_start[owner] + tsdf::popcount7(edge_mask[owner] & lower);
                }
                if (at >= 0 && at < nf) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) faces[(size_t)at * 3 + e] = idx[e];
                }
                ++at;
            }
        }
    }
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
static int tm_dims(const int* dims_host, const char* what, long long* voxels) {
    RCMVS_REQUIRE(dims_host, "%s: null pointer", what);
    const long long gx = dims_host[0], gy = dims_host[1], gz = dims_host[2];
    RCMVS_REQUIRE(gx >= 1 && gy >= 1 && gz >= 1 && gx <= RCMVS_TSDF_MAX_VOXELS && gy <= RCMVS_TSDF_MAX_VOXELS && gz <= RCMVS_TSDF_MAX_VOXELS &&
                  gx * gy <= RCMVS_TSDF_MAX_VOXELS && gx * gy * gz <= RCMVS_TSDF_MAX_VOXELS,
                  "%s: bad dims %lld x %lld x %lld (each >= 1, at most 2^28 voxels)", what, gx, gy, gz);
    *voxels = gx * gy * gz;
    return 0;
}

static int tm_grid(const double* grid_host, const int* dims_host, const char* what, tsdf::Grid* g) {
    RCMVS_REQUIRE(grid_host, "%s: null pointer", what);
    for (int a = 0; a < 4; ++a) RCMVS_REQUIRE(std::isfinite(grid_host[a]), "%s: grid value %d is %g (finite; the order is ox oy oz h)", what, a, grid_host[a]);
    RCMVS_REQUIRE(grid_host[3] > 0.0, "%s: voxel edge h = %g (finite, positive)", what, grid_host[3]);
    *g = tsdf::Grid{grid_host[0], grid_host[1], grid_host[2], grid_host[3], dims_host[0], dims_host[1], dims_host[2]};
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_tsdf_integrate_timed(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                                          const double* grid_host, const int* dims_host, float* dsum, float* wsum, float* csum_r, float* csum_g,
                                          float* csum_b, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(depth && cams_host && grid_host && dims_host && dsum && wsum, "tsdf_integrate: null pointer");
    RCMVS_REQUIRE((csum_r && csum_g && csum_b) || (!csum_r && !csum_g && !csum_b), "tsdf_integrate: null pointer (three colour planes or none)");
    long long voxels;
    if (int rc = tm_dims(dims_host, "tsdf_integrate", &voxels)) return rc;
    RCMVS_REQUIRE(n >= 1 && n <= RCMVS_TSDF_MAX_VIEWS, "tsdf_integrate: %d views (1 .. %d per call)", n, RCMVS_TSDF_MAX_VIEWS);
    RCMVS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "tsdf_integrate: bad image size H=%d W=%d (each >= 1, H * W < 2^31)", H, W);
    RCMVS_REQUIRE(std::isfinite(trunc) && trunc > 0.0, "tsdf_integrate: trunc = %g (finite, positive)", trunc);
    tsdf::Grid g;
    if (int rc = tm_grid(grid_host, dims_host, "tsdf_integrate", &g)) return rc;
    tsdf::Cams cams = {};
    for (int s = 0; s < n; ++s) {
        const double* c = cams_host + 16 * s;
        for (int a = 0; a < 16; ++a) {
            RCMVS_REQUIRE(std::isfinite(c[a]), "tsdf_integrate: camera %d value %d is %g (finite; the order is R 9, t 3, fx fy cx cy)", s, a, c[a]);
            cams.c[s][a] = c[a];
        }
        RCMVS_REQUIRE(c[12] > 0.0 && c[13] > 0.0, "tsdf_integrate: camera %d focal lengths %g, %g (finite, positive)", s, c[12], c[13]);
    }
    const unsigned blocks = (unsigned)cdiv(voxels, TM_BLOCK);
    RCMVS_LAUNCH_TIMED(tsdf_integrate_kernel, dim3(blocks), dim3(TM_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1),
                       depth, rgb, n, H, W, cams, trunc, g, (int)voxels, dsum, wsum, csum_r, csum_g, csum_b);
    return launch_status("tsdf_integrate");
}

extern "C" int rcmvs_tsdf_integrate(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                                    const double* grid_host, const int* dims_host, float* dsum, float* wsum, float* csum_r, float* csum_g,
                                    float* csum_b, void* stream) {
    return rcmvs_tsdf_integrate_timed(depth, rgb, n, H, W, cams_host, trunc, grid_host, dims_host, dsum, wsum, csum_r, csum_g, csum_b, nullptr, nullptr,
                                      stream);
}

extern "C" int rcmvs_tsdf_mesh_count_timed(const float* dsum, const float* wsum, const int* dims_host, int min_weight, unsigned char* edge_mask,
                                           unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                                           void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(dsum && wsum && dims_host && edge_mask && tri_count && scan_work && vert_start && tri_start && totals, "tsdf_mesh_count: null pointer");
    long long voxels;
    if (int rc = tm_dims(dims_host, "tsdf_mesh_count", &voxels)) return rc;
    RCMVS_REQUIRE(min_weight >= 1, "tsdf_mesh_count: min_weight = %d (>= 1)", min_weight);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(scan_work) & 7) == 0, "tsdf_mesh_count: scan_work must be 8-byte aligned");
    const TmDims g = {dims_host[0], dims_host[1], dims_host[2]};
    const int nb1 = (int)cdiv(voxels, TM_TILE), nb2 = (int)cdiv(nb1, TM_TILE);      // nb2 <= TM_TOP by the voxel cap
    unsigned long long* top = reinterpret_cast<unsigned long long*>(scan_work);       // 2 * TM_TOP uint64 = 256 ints
    unsigned* tile_v = reinterpret_cast<unsigned*>(scan_work) + 4 * TM_TOP;
    unsigned* tile_t = tile_v + nb1;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(tsdf_count_kernel, dim3(nb1), dim3(TM_BLOCK), 0, st, e0, none, dsum, wsum, g, (int)voxels, (float)min_weight, edge_mask, tri_count,
                       tile_v, tile_t);
    hipLaunchKernelGGL(tsdf_scan_up_kernel<TM_TOP>, dim3(nb2), dim3(TM_BLOCK), 0, st, tile_v, tile_t, nb1, top);
    hipLaunchKernelGGL(tsdf_scan_top_kernel<TM_TOP>, dim3(1), dim3(64), 0, st, top, nb2, totals);
    hipLaunchKernelGGL(tsdf_scan_mid_kernel<TM_TOP>, dim3(nb2), dim3(TM_BLOCK), 0, st, tile_v, tile_t, nb1, top);
    RCMVS_LAUNCH_TIMED(tsdf_scan_down_kernel, dim3(nb1), dim3(TM_BLOCK), 0, st, none, e1, edge_mask, tri_count, (int)voxels, tile_v, tile_t, totals,
                       vert_start, tri_start);
    return launch_status("tsdf_mesh_count");
}

extern "C" int rcmvs_tsdf_mesh_count(const float* dsum, const float* wsum, const int* dims_host, int min_weight, unsigned char* edge_mask,
                                     unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                                     void* stream) {
    return rcmvs_tsdf_mesh_count_timed(dsum, wsum, dims_host, min_weight, edge_mask, tri_count, scan_work, vert_start, tri_start, totals, nullptr, nullptr,
                                       stream);
}

extern "C" int rcmvs_tsdf_mesh_emit_timed(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                                          const double* grid_host, const int* dims_host, int min_weight, const unsigned char* edge_mask,
                                          const unsigned char* tri_count, const int* vert_start, const int* tri_start, long long nv, long long nf,
                                          float* verts, unsigned char* vert_rgb, int* faces, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(dsum && wsum && grid_host && dims_host && edge_mask && tri_count && vert_start && tri_start, "tsdf_mesh_emit: null pointer");
    RCMVS_REQUIRE(nv >= 0 && nf >= 0 && nv < (1ll << 31) && nf < (1ll << 31), "tsdf_mesh_emit: %lld vertices, %lld faces (0 .. 2^31-1 each)", nv, nf);
    RCMVS_REQUIRE((verts || nv == 0) && (faces || nf == 0), "tsdf_mesh_emit: null pointer (verts / faces)");
    RCMVS_REQUIRE(!vert_rgb || (csum_r && csum_g && csum_b), "tsdf_mesh_emit: null pointer (vert_rgb needs the three colour planes)");
    long long voxels;
    if (int rc = tm_dims(dims_host, "tsdf_mesh_emit", &voxels)) return rc;
    RCMVS_REQUIRE(min_weight >= 1, "tsdf_mesh_emit: min_weight = %d (>= 1)", min_weight);
    tsdf::Grid g;
    if (int rc = tm_grid(grid_host, dims_host, "tsdf_mesh_emit", &g)) return rc;
    const unsigned blocks = (unsigned)cdiv(voxels, TM_BLOCK);
    RCMVS_LAUNCH_TIMED(tsdf_emit_kernel, dim3(blocks), dim3(TM_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1),
                       dsum, wsum, csum_r, csum_g, csum_b, g, (int)voxels, (float)min_weight, edge_mask, tri_count, vert_start, tri_start, (int)nv,
                       (int)nf, verts, vert_rgb, faces);
    return launch_status("tsdf_mesh_emit");
}

extern "C" int rcmvs_tsdf_mesh_emit(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                                    const double* grid_host, const int* dims_host, int min_weight, const unsigned char* edge_mask,
                                    const unsigned char* tri_count, const int* vert_start, const int* tri_start, long long nv, long long nf,
                                    float* verts, unsigned char* vert_rgb, int* faces, void* stream) {
    return rcmvs_tsdf_mesh_emit_timed(dsum, wsum, csum_r, csum_g, csum_b, grid_host, dims_host, min_weight, edge_mask, tri_count, vert_start, tri_start, nv,
                                      nf, verts, vert_rgb, faces, nullptr, nullptr, stream);
}
