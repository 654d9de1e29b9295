// The block-sparse TSDF volume: 8 x 8 x 8-voxel blocks allocated in a band around the depth samples, integrated and meshed by
// marching tetrahedra (rc_mvsnet_amd/tsdf_mesh.py SparseTsdfVolume; contract in tsdf_sparse.h, the marking rule in
// tsdf_sparse_math.h, everything per voxel in tsdf_mesh_math.h and tsdf_mesh_cells.h, shared with the dense volume).
//
//   mark       One thread per pixel, the views on the grid's y.  The rule bounds a thread's stores at 4 x 4 x 4 flag bytes.
//   build      flags -> 32-bit mask words and their popcounts (a block owns 2048 words), one block scans the at most 2048 tile
//              sums, then every word gets its rank and writes its set bits' block numbers to `active`.
//   integrate  One workgroup per active block, a thread per voxel: the block's coordinates come from active[slot], the walk
//              through the views is the dense kernel's own (tm_integrate_voxel).
//   count      One workgroup per active block.  It fills a 9 x 9 x 9 tile of (allocated number, flags) in LDS -- its own voxels
//              and the halo from up to seven neighbour blocks, found by rank -- and every cube and edge then reads LDS only.
//              The blocks' sums are scanned by the dense volume's upper levels (top level: 256 sums), then one workgroup per
//              block writes its voxels' starts.
//   emit       The same tile; a vertex reads its two voxels, a face its owners' starts and masks, through the allocated numbers.
// gfx950 only; __syncthreads and plain loads and stores, one atomicAdd per workgroup for the skipped count (tests/emu compiles this).
#include <cstdint>

#include "common.h"
#include "tsdf_mesh_cells.h"
#include "tsdf_sparse.h"
#include "tsdf_sparse_math.h"

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int SP_VOX = tsdf_sp::BLOCK_VOXELS;                     // 512 voxels per block
constexpr int SP_TILE = RCMVS_TSDF_SP_SCAN_TILE;
constexpr int SP_PER = SP_TILE / TM_BLOCK;
constexpr int SP_TOP = RCMVS_TSDF_SP_MAX_ACTIVE / RCMVS_TSDF_SP_SCAN_TILE;        // 256 sums at the top level of the count scan
constexpr int SP_HALO = 9 * 9 * 9;
static_assert(SP_TILE == TM_TILE, "the count scan's upper levels are the dense volume's");

// ---- mark -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_mark_kernel(const float* __restrict__ depth, int H, int W, tsdf::Cams cams, double trunc,
                                                                tsdf_sp::BlockGrid g, unsigned char* __restrict__ flags,
                                                                unsigned long long* __restrict__ skipped) {
    const int s = (int)blockIdx.y;
    const size_t plane = (size_t)H * (size_t)W;
    const long long p = (long long)blockIdx.x * TM_BLOCK + threadIdx.x;
    int skip = 0;
    if (p < (long long)plane) {
        int bl[3], bh[3];
        const tsdf_sp::MarkResult r = tsdf_sp::mark_range(cams.c[s], (int)(p % W), (int)(p / W), depth[(size_t)s * plane + (size_t)p], trunc, g, bl, bh);
        skip = r == tsdf_sp::MARK_SKIPPED;
        if (r == tsdf_sp::MARK_RANGE)
            for (int Z = bl[2]; Z <= bh[2]; ++Z)
                for (int Y = bl[1]; Y <= bh[1]; ++Y)
                    for (int X = bl[0]; X <= bh[0]; ++X) flags[(size_t)X + (size_t)g.bx * ((size_t)Y + (size_t)g.by * (size_t)Z)] = 1;
    }
    const int count = __syncthreads_count(skip);
    if (threadIdx.x == 0 && count) atomicAdd(skipped, (unsigned long long)count);
}

// ---- build ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_words_kernel(const unsigned char* __restrict__ flags, int blocks, int words,
                                                                 unsigned* __restrict__ mask_words, unsigned* __restrict__ tile_sum) {
    __shared__ unsigned sh[TM_BLOCK];
    unsigned n = 0;
    for (int q = 0; q < SP_PER; ++q) {
        const long long w = (long long)blockIdx.x * SP_TILE + (long long)q * TM_BLOCK + threadIdx.x;
        if (w >= words) break;
        unsigned m = 0;
        const long long base = w * 32;
        for (int b = 0; b < 32; ++b)
            if (base + b < blocks && flags[base + b]) m |= 1u << b;
        mask_words[w] = m;
        n += (unsigned)__builtin_popcount(m);
    }
    const unsigned sum = tm_block_sum(n, sh);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;
}

// the at most SP_TILE tile sums -> their exclusive prefixes in place; the total goes to word_rank[words]
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_tiles_kernel(unsigned* __restrict__ tile_sum, int tiles, unsigned* __restrict__ total) {
    __shared__ unsigned sh[TM_BLOCK];
    const int base = (int)threadIdx.x * SP_PER;
    unsigned c[SP_PER], s = 0;
#pragma unroll
    for (int q = 0; q < SP_PER; ++q) { c[q] = base + q < tiles ? tile_sum[base + q] : 0u; s += c[q]; }
    unsigned run = tm_block_exclusive(s, sh);
#pragma unroll
    for (int q = 0; q < SP_PER; ++q) { if (base + q < tiles) tile_sum[base + q] = run; run += c[q]; }
    if (threadIdx.x == TM_BLOCK - 1) *total = run;
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_rank_kernel(const unsigned* __restrict__ mask_words, int words, const unsigned* __restrict__ tile_sum,
                                                                unsigned* __restrict__ word_rank, int* __restrict__ active, int capacity) {
    __shared__ unsigned sh[TM_BLOCK];
    const long long base = (long long)blockIdx.x * SP_TILE + (long long)threadIdx.x * SP_PER;
    unsigned m[SP_PER], s = 0;
#pragma unroll
    for (int q = 0; q < SP_PER; ++q) { m[q] = base + q < words ? mask_words[base + q] : 0u; s += (unsigned)__builtin_popcount(m[q]); }
    unsigned run = tm_block_exclusive(s, sh) + tile_sum[blockIdx.x];
#pragma unroll
    for (int q = 0; q < SP_PER; ++q) {
        if (base + q >= words) break;
        word_rank[base + q] = run;
        for (unsigned rest = m[q]; rest; rest &= rest - 1u) {
            if (run < (unsigned)capacity) active[run] = (int)((base + q) * 32 + __builtin_ctz(rest));
            ++run;
        }
    }
}

// ---- the block table --------------------------------------------------------------------------------------------------------
struct SpTable {
    const unsigned* mask_words;
    const unsigned* word_rank;
    const int* active;
    int n_active, bx, by, bz;
};

// the slot of block (X, Y, Z), or -1 when it lies beyond the grid or is not active
__device__ inline int sp_slot(const SpTable& t, int X, int Y, int Z) {
    if (X >= t.bx || Y >= t.by || Z >= t.bz) return -1;
    const unsigned B = (unsigned)(X + t.bx * (Y + t.by * Z));
    const unsigned word = t.mask_words[B >> 5];
    if (!((word >> (B & 31u)) & 1u)) return -1;
    const unsigned s = t.word_rank[B >> 5] + (unsigned)__builtin_popcount(tsdf_sp::bits_below(word, B & 31u));
    return s < (unsigned)t.n_active ? (int)s : -1;
}

__device__ inline int sp_halo_index(int x, int y, int z) { return x + 9 * (y + 9 * z); }

// The 9 x 9 x 9 tile of the block in `slot`: alloc[e] = the allocated number of voxel (x, y, z) of the tile (8 = the first voxel of
// the next block along that axis) or -1 where there is no active block, fl[e] = its flags.  False (for the whole workgroup) when
// active[slot] is no block of the grid.  nslot: 8 ints of LDS.
__device__ inline bool sp_fill_tile(const SpTable& t, int slot, const float* __restrict__ dsum, const float* __restrict__ wsum, float min_weight,
                                    int* nslot, int* alloc, unsigned char* fl, int* X, int* Y, int* Z) {
    const int B = t.active[slot];
    if (B < 0 || B >= t.bx * t.by * t.bz) return false;
    *X = B % t.bx; *Y = (B / t.bx) % t.by; *Z = B / (t.bx * t.by);
    if (threadIdx.x < 8) {
        const int c = (int)threadIdx.x;
        nslot[c] = c == 0 ? slot : sp_slot(t, *X + (c & 1), *Y + ((c >> 1) & 1), *Z + (c >> 2));
    }
    __syncthreads();
    for (int e = (int)threadIdx.x; e < SP_HALO; e += TM_BLOCK) {
        const int x = e % 9, y = (e / 9) % 9, z = e / 81;
        const int s = nslot[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
        const int a = s < 0 ? -1 : s * SP_VOX + (x & 7) + 8 * ((y & 7) + 8 * (z & 7));
        alloc[e] = a;
        fl[e] = (unsigned char)(a < 0 ? 0 : tm_flags(dsum, wsum, a, min_weight));
    }
    __syncthreads();
    return true;
}

__device__ inline void sp_corner_flags(const unsigned char* fl, int lx, int ly, int lz, int* f) {
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = fl[sp_halo_index(lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2))];
}

// ---- integrate --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_VOX) void tsdf_sp_integrate_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ rgb, int n, int H,
                                                                   int W, tsdf::Cams cams, double trunc, tsdf_sp::BlockGrid g,
                                                                   const int* __restrict__ active, float* __restrict__ dsum, float* __restrict__ wsum,
                                                                   float* __restrict__ cr, float* __restrict__ cg, float* __restrict__ cb) {
    const int B = active[blockIdx.x];
    if (B < 0 || B >= g.bx * g.by * g.bz) return;
    const int l = (int)threadIdx.x;
    const int i = 8 * (B % g.bx) + (l & 7), j = 8 * ((B / g.bx) % g.by) + ((l >> 3) & 7), k = 8 * (B / (g.bx * g.by)) + (l >> 6);
    const double px = tsdf::centre(g.ox, i, g.h), py = tsdf::centre(g.oy, j, g.h), pz = tsdf::centre(g.oz, k, g.h);
    const int v = (int)blockIdx.x * SP_VOX + l;
    const bool colour = rgb != nullptr && cr != nullptr;
    float d = dsum[v], w = wsum[v], r = 0.0f, gr = 0.0f, b = 0.0f;
    if (colour) { r = cr[v]; gr = cg[v]; b = cb[v]; }
    const TmState s = tm_integrate_voxel(depth, rgb, n, H, W, cams, trunc, px, py, pz, colour, TmState{d, w, r, gr, b});
    dsum[v] = s.d;
    wsum[v] = s.w;
    if (colour) { cr[v] = s.r; cg[v] = s.g; cb[v] = s.b; }
}

// ---- count ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_count_kernel(const float* __restrict__ dsum, const float* __restrict__ wsum, SpTable t, float min_weight,
                                                                 unsigned char* __restrict__ edge_mask, unsigned char* __restrict__ tri_count,
                                                                 unsigned* __restrict__ blk_v, unsigned* __restrict__ blk_t) {
    __shared__ unsigned sh[TM_BLOCK];
    __shared__ int nslot[8], alloc[SP_HALO];
    __shared__ unsigned char fl[SP_HALO];
    const int slot = (int)blockIdx.x;
    int X, Y, Z;
    const bool ok = sp_fill_tile(t, slot, dsum, wsum, min_weight, nslot, alloc, fl, &X, &Y, &Z);
    unsigned nv = 0, nt = 0;
    for (int l = (int)threadIdx.x; l < SP_VOX; l += TM_BLOCK) {
        unsigned m = 0, tr = 0;
        if (ok) {
            int f[8];
            sp_corner_flags(fl, l & 7, (l >> 3) & 7, l >> 6, f);
            m = tm_edge_mask(f);
#pragma unroll
            for (int tet = 0; tet < 6; ++tet) tr += tsdf::tet_case(tm_tet_case(f, tet)).n;
        }
        edge_mask[(size_t)slot * SP_VOX + l] = (unsigned char)m;
        tri_count[(size_t)slot * SP_VOX + l] = (unsigned char)tr;
        nv += (unsigned)tsdf::popcount7(m);
        nt += tr;
    }
    const unsigned sv = tm_block_sum(nv, sh), st = tm_block_sum(nt, sh);
    if (threadIdx.x == 0) { blk_v[slot] = sv; blk_t[slot] = st; }
}

// a block's voxels' starts from the scanned block sums; a thread owns two neighbouring voxels
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_starts_kernel(const unsigned char* __restrict__ edge_mask, const unsigned char* __restrict__ tri_count,
                                                                  int n_active, const unsigned* __restrict__ blk_v, const unsigned* __restrict__ blk_t,
                                                                  const unsigned long long* __restrict__ totals, int* __restrict__ vert_start,
                                                                  int* __restrict__ tri_start) {
    __shared__ unsigned sh[TM_BLOCK];
    const size_t base = (size_t)blockIdx.x * SP_VOX + 2 * threadIdx.x;
    const unsigned v0 = (unsigned)tsdf::popcount7(edge_mask[base]), v1 = (unsigned)tsdf::popcount7(edge_mask[base + 1]);
    const unsigned t0 = tri_count[base], t1 = tri_count[base + 1];
    const unsigned rv = tm_block_exclusive(v0 + v1, sh) + blk_v[blockIdx.x];
    const unsigned rt = tm_block_exclusive(t0 + t1, sh) + blk_t[blockIdx.x];
    vert_start[base] = (int)rv;
    vert_start[base + 1] = (int)(rv + v0);
    tri_start[base] = (int)rt;
    tri_start[base + 1] = (int)(rt + t0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        vert_start[(size_t)n_active * SP_VOX] = (int)(unsigned)totals[0];
        tri_start[(size_t)n_active * SP_VOX] = (int)(unsigned)totals[1];
    }
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tsdf_sp_emit_kernel(const float* __restrict__ dsum, const float* __restrict__ wsum, const float* __restrict__ cr,
                                                                const float* __restrict__ cg, const float* __restrict__ cb, tsdf_sp::BlockGrid g, SpTable t,
                                                                float min_weight, const unsigned char* __restrict__ edge_mask,
                                                                const unsigned char* __restrict__ tri_count, const int* __restrict__ vert_start,
                                                                const int* __restrict__ tri_start, int nv, int nf, float* __restrict__ verts,
                                                                unsigned char* __restrict__ vert_rgb, int* __restrict__ faces) {
    __shared__ int nslot[8], alloc[SP_HALO];
    __shared__ unsigned char fl[SP_HALO];
    const int slot = (int)blockIdx.x;
    int X, Y, Z;
    if (!sp_fill_tile(t, slot, dsum, wsum, min_weight, nslot, alloc, fl, &X, &Y, &Z)) return;
    for (int l = (int)threadIdx.x; l < SP_VOX; l += TM_BLOCK) {
        const int v = slot * SP_VOX + l;
        const unsigned mask = edge_mask[v];
        const int ntri = tri_count[v];
        if (mask == 0 && ntri == 0) continue;
        const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
        const int i = 8 * X + lx, j = 8 * Y + ly, k = 8 * Z + lz;
        if (mask) {
            const double wa = (double)wsum[v], da = (double)dsum[v] / wa;
            const double pa[3] = {tsdf::centre(g.ox, i, g.h), tsdf::centre(g.oy, j, g.h), tsdf::centre(g.oz, k, g.h)};
            int at = vert_start[v];
            for (int c = 1; c < 8; ++c) {
                if (!((mask >> (c - 1)) & 1)) continue;
                const int u = alloc[sp_halo_index(lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2))];
                if (u < 0) continue;                                                          // never with the count kernel's masks
                const double wb = (double)wsum[u], db = (double)dsum[u] / wb;
                const double tt = tsdf::crossing(da, db);
                const double pb[3] = {tsdf::centre(g.ox, i + (c & 1), g.h), tsdf::centre(g.oy, j + ((c >> 1) & 1), g.h),
                                      tsdf::centre(g.oz, k + (c >> 2), g.h)};
                if (at >= 0 && at < nv) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) verts[(size_t)at * 3 + a] = (float)tsdf::lerp(pa[a], pb[a], tt);
                    if (vert_rgb) {
                        vert_rgb[(size_t)at * 3 + 0] = tsdf::colour_byte((double)cr[v] / wa, (double)cr[u] / wb, tt);
                        vert_rgb[(size_t)at * 3 + 1] = tsdf::colour_byte((double)cg[v] / wa, (double)cg[u] / wb, tt);
                        vert_rgb[(size_t)at * 3 + 2] = tsdf::colour_byte((double)cb[v] / wa, (double)cb[u] / wb, tt);
                    }
                }
                ++at;
            }
        }
        if (ntri) {                                                 // the cube's eight corners are observed voxels of active blocks
            int f[8];
            sp_corner_flags(fl, lx, ly, lz, f);
            int at = tri_start[v];
            for (int tet = 0; tet < 6; ++tet) {
                const tsdf::TetCase tc = tsdf::tet_case(tm_tet_case(f, tet));
                const bool swap = tsdf::tet_sign(tet) < 0;
                for (int q = 0; q < tc.n; ++q) {
                    int idx[3];
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const int code = tc.e[3 * q + (e == 0 ? 0 : (swap ? 3 - e : e))];
                        const int ca = tsdf::tet_corner(tet, code >> 2), cb2 = tsdf::tet_corner(tet, code & 3);
                        const int owner = alloc[sp_halo_index(lx + (ca & 1), ly + ((ca >> 1) & 1), lz + (ca >> 2))];
                        const unsigned lower = (1u << ((cb2 ^ ca) - 1)) - 1u;
                        idx[e] = owner < 0 ? 0 : vert_start[owner] + tsdf::popcount7(edge_mask[owner] & lower);
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
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
static int sp_bdims(const int* bdims_host, const char* what, long long* blocks) {
    RCMVS_REQUIRE(bdims_host, "%s: null pointer", what);
    const long long bx = bdims_host[0], by = bdims_host[1], bz = bdims_host[2];
    RCMVS_REQUIRE(bx >= 1 && by >= 1 && bz >= 1 && bx <= RCMVS_TSDF_SP_MAX_BLOCKS && by <= RCMVS_TSDF_SP_MAX_BLOCKS && bz <= RCMVS_TSDF_SP_MAX_BLOCKS &&
                  bx * by <= RCMVS_TSDF_SP_MAX_BLOCKS && bx * by * bz <= RCMVS_TSDF_SP_MAX_BLOCKS,
                  "%s: bad bdims %lld x %lld x %lld (each >= 1, at most 2^27 blocks)", what, bx, by, bz);
    *blocks = bx * by * bz;
    return 0;
}

static int sp_grid(const double* grid_host, const int* bdims_host, const char* what, tsdf_sp::BlockGrid* g) {
    RCMVS_REQUIRE(grid_host, "%s: null pointer", what);
    for (int a = 0; a < 4; ++a) RCMVS_REQUIRE(std::isfinite(grid_host[a]), "%s: grid value %d is %g (finite; the order is ox oy oz h)", what, a, grid_host[a]);
    RCMVS_REQUIRE(grid_host[3] > 0.0, "%s: voxel edge h = %g (finite, positive)", what, grid_host[3]);
    *g = tsdf_sp::BlockGrid{grid_host[0], grid_host[1], grid_host[2], grid_host[3], bdims_host[0], bdims_host[1], bdims_host[2]};
    return 0;
}

static int sp_views(const char* what, int n, int H, int W, const double* cams_host, double trunc, tsdf::Cams* cams) {
    RCMVS_REQUIRE(n >= 1 && n <= RCMVS_TSDF_MAX_VIEWS, "%s: %d views (1 .. %d per call)", what, n, RCMVS_TSDF_MAX_VIEWS);
    RCMVS_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "%s: bad image size H=%d W=%d (each >= 1, H * W < 2^31)", what, H, W);
    RCMVS_REQUIRE(std::isfinite(trunc) && trunc > 0.0, "%s: trunc = %g (finite, positive)", what, trunc);
    for (int s = 0; s < n; ++s) {
        const double* c = cams_host + 16 * s;
        for (int a = 0; a < 16; ++a) {
            RCMVS_REQUIRE(std::isfinite(c[a]), "%s: camera %d value %d is %g (finite; the order is R 9, t 3, fx fy cx cy)", what, s, a, c[a]);
            cams->c[s][a] = c[a];
        }
        RCMVS_REQUIRE(c[12] > 0.0 && c[13] > 0.0, "%s: camera %d focal lengths %g, %g (finite, positive)", what, s, c[12], c[13]);
    }
    return 0;
}

static int sp_active(const char* what, int n_active, long long blocks) {
    RCMVS_REQUIRE(n_active >= 1 && n_active <= RCMVS_TSDF_SP_MAX_ACTIVE && n_active <= blocks,
                  "%s: %d active blocks (1 .. 2^19, at most the grid's %lld)", what, n_active, blocks);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_tsdf_sp_mark_timed(const float* depth, int n, int H, int W, const double* cams_host, double trunc, const double* grid_host,
                                        const int* bdims_host, unsigned char* flags, unsigned long long* skipped, void* ev0, void* ev1,
                                        void* stream) {
    RCMVS_REQUIRE(depth && cams_host && grid_host && bdims_host && flags && skipped, "tsdf_sp_mark: null pointer");
    long long blocks;
    if (int rc = sp_bdims(bdims_host, "tsdf_sp_mark", &blocks)) return rc;
    tsdf::Cams cams = {};
    if (int rc = sp_views("tsdf_sp_mark", n, H, W, cams_host, trunc, &cams)) return rc;
    tsdf_sp::BlockGrid g;
    if (int rc = sp_grid(grid_host, bdims_host, "tsdf_sp_mark", &g)) return rc;
    const dim3 grid((unsigned)cdiv((long long)H * W, TM_BLOCK), (unsigned)n);
    RCMVS_LAUNCH_TIMED(tsdf_sp_mark_kernel, grid, dim3(TM_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1), depth,
                       H, W, cams, trunc, g, flags, skipped);
    return launch_status("tsdf_sp_mark");
}

extern "C" int rcmvs_tsdf_sp_mark(const float* depth, int n, int H, int W, const double* cams_host, double trunc, const double* grid_host,
                                  const int* bdims_host, unsigned char* flags, unsigned long long* skipped, void* stream) {
    return rcmvs_tsdf_sp_mark_timed(depth, n, H, W, cams_host, trunc, grid_host, bdims_host, flags, skipped, nullptr, nullptr, stream);
}

extern "C" int rcmvs_tsdf_sp_build_timed(const unsigned char* flags, const int* bdims_host, unsigned int* mask_words, unsigned int* word_rank,
                                         int* active, int active_capacity, int* scan_work, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(flags && bdims_host && mask_words && word_rank && active && scan_work, "tsdf_sp_build: null pointer");
    long long blocks;
    if (int rc = sp_bdims(bdims_host, "tsdf_sp_build", &blocks)) return rc;
    RCMVS_REQUIRE(active_capacity >= 1, "tsdf_sp_build: active_capacity = %d (>= 1)", active_capacity);
    const int words = (int)cdiv(blocks, 32), tiles = (int)cdiv(words, SP_TILE);             // tiles <= SP_TILE by the block cap
    unsigned* tile_sum = reinterpret_cast<unsigned*>(scan_work);
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(tsdf_sp_words_kernel, dim3(tiles), dim3(TM_BLOCK), 0, st, e0, none, flags, (int)blocks, words, mask_words, tile_sum);
    hipLaunchKernelGGL(tsdf_sp_tiles_kernel, dim3(1), dim3(TM_BLOCK), 0, st, tile_sum, tiles, word_rank + words);
    RCMVS_LAUNCH_TIMED(tsdf_sp_rank_kernel, dim3(tiles), dim3(TM_BLOCK), 0, st, none, e1, mask_words, words, tile_sum, word_rank, active, active_capacity);
    return launch_status("tsdf_sp_build");
}

extern "C" int rcmvs_tsdf_sp_build(const unsigned char* flags, const int* bdims_host, unsigned int* mask_words, unsigned int* word_rank, int* active,
                                   int active_capacity, int* scan_work, void* stream) {
    return rcmvs_tsdf_sp_build_timed(flags, bdims_host, mask_words, word_rank, active, active_capacity, scan_work, nullptr, nullptr, stream);
}

extern "C" int rcmvs_tsdf_sp_integrate_timed(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                                             const double* grid_host, const int* bdims_host, const int* active, int n_active, float* dsum,
                                             float* wsum, float* csum_r, float* csum_g, float* csum_b, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(depth && cams_host && grid_host && bdims_host && active && dsum && wsum, "tsdf_sp_integrate: null pointer");
    RCMVS_REQUIRE((csum_r && csum_g && csum_b) || (!csum_r && !csum_g && !csum_b), "tsdf_sp_integrate: null pointer (three colour planes or none)");
    long long blocks;
    if (int rc = sp_bdims(bdims_host, "tsdf_sp_integrate", &blocks)) return rc;
    if (int rc = sp_active("tsdf_sp_integrate", n_active, blocks)) return rc;
    tsdf::Cams cams = {};
    if (int rc = sp_views("tsdf_sp_integrate", n, H, W, cams_host, trunc, &cams)) return rc;
    tsdf_sp::BlockGrid g;
    if (int rc = sp_grid(grid_host, bdims_host, "tsdf_sp_integrate", &g)) return rc;
    RCMVS_LAUNCH_TIMED(tsdf_sp_integrate_kernel, dim3(n_active), dim3(SP_VOX), 0, as_stream(stream), static_cast<hipEvent_t>(ev0),
                       static_cast<hipEvent_t>(ev1), depth, rgb, n, H, W, cams, trunc, g, active, dsum, wsum, csum_r, csum_g, csum_b);
    return launch_status("tsdf_sp_integrate");
}

extern "C" int rcmvs_tsdf_sp_integrate(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                                       const double* grid_host, const int* bdims_host, const int* active, int n_active, float* dsum, float* wsum,
                                       float* csum_r, float* csum_g, float* csum_b, void* stream) {
    return rcmvs_tsdf_sp_integrate_timed(depth, rgb, n, H, W, cams_host, trunc, grid_host, bdims_host, active, n_active, dsum, wsum, csum_r, csum_g,
                                         csum_b, nullptr, nullptr, stream);
}

extern "C" int rcmvs_tsdf_sp_mesh_count_timed(const float* dsum, const float* wsum, const int* bdims_host, const unsigned int* mask_words,
                                              const unsigned int* word_rank, const int* active, int n_active, int min_weight,
                                              unsigned char* edge_mask, unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start,
                                              unsigned long long* totals, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(dsum && wsum && bdims_host && mask_words && word_rank && active && edge_mask && tri_count && scan_work && vert_start && tri_start &&
                  totals, "tsdf_sp_mesh_count: null pointer");
    long long blocks;
    if (int rc = sp_bdims(bdims_host, "tsdf_sp_mesh_count", &blocks)) return rc;
    if (int rc = sp_active("tsdf_sp_mesh_count", n_active, blocks)) return rc;
    RCMVS_REQUIRE(min_weight >= 1, "tsdf_sp_mesh_count: min_weight = %d (>= 1)", min_weight);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(scan_work) & 7) == 0, "tsdf_sp_mesh_count: scan_work must be 8-byte aligned");
    const SpTable t = {mask_words, word_rank, active, n_active, bdims_host[0], bdims_host[1], bdims_host[2]};
    const int nb2 = (int)cdiv(n_active, SP_TILE);                                     // nb2 <= SP_TOP by the cap on active blocks
    unsigned long long* top = reinterpret_cast<unsigned long long*>(scan_work);       // 2 * SP_TOP uint64 = 1024 ints
    unsigned* blk_v = reinterpret_cast<unsigned*>(scan_work) + 4 * SP_TOP;
    unsigned* blk_t = blk_v + n_active;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(tsdf_sp_count_kernel, dim3(n_active), dim3(TM_BLOCK), 0, st, e0, none, dsum, wsum, t, (float)min_weight, edge_mask, tri_count, blk_v,
                       blk_t);
    hipLaunchKernelGGL(tsdf_scan_up_kernel<SP_TOP>, dim3(nb2), dim3(TM_BLOCK), 0, st, blk_v, blk_t, n_active, top);
    hipLaunchKernelGGL(tsdf_scan_top_kernel<SP_TOP>, dim3(1), dim3(64), 0, st, top, nb2, totals);
    hipLaunchKernelGGL(tsdf_scan_mid_kernel<SP_TOP>, dim3(nb2), dim3(TM_BLOCK), 0, st, blk_v, blk_t, n_active, top);
    RCMVS_LAUNCH_TIMED(tsdf_sp_starts_kernel, dim3(n_active), dim3(TM_BLOCK), 0, st, none, e1, edge_mask, tri_count, n_active, blk_v, blk_t, totals,
                       vert_start, tri_start);
    return launch_status("tsdf_sp_mesh_count");
}

extern "C" int rcmvs_tsdf_sp_mesh_count(const float* dsum, const float* wsum, const int* bdims_host, const unsigned int* mask_words,
                                        const unsigned int* word_rank, const int* active, int n_active, int min_weight, unsigned char* edge_mask,
                                        unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                                        void* stream) {
    return rcmvs_tsdf_sp_mesh_count_timed(dsum, wsum, bdims_host, mask_words, word_rank, active, n_active, min_weight, edge_mask, tri_count, scan_work,
                                          vert_start, tri_start, totals, nullptr, nullptr, stream);
}

extern "C" int rcmvs_tsdf_sp_mesh_emit_timed(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                                             const double* grid_host, const int* bdims_host, const unsigned int* mask_words,
                                             const unsigned int* word_rank, const int* active, int n_active, int min_weight,
                                             const unsigned char* edge_mask, const unsigned char* tri_count, const int* vert_start,
                                             const int* tri_start, long long nv, long long nf, float* verts, unsigned char* vert_rgb, int* faces,
                                             void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(dsum && wsum && grid_host && bdims_host && mask_words && word_rank && active && edge_mask && tri_count && vert_start && tri_start,
                  "tsdf_sp_mesh_emit: null pointer");
    RCMVS_REQUIRE(nv >= 0 && nf >= 0 && nv < (1ll << 31) && nf < (1ll << 31), "tsdf_sp_mesh_emit: %lld vertices, %lld faces (0 .. 2^31-1 each)", nv, nf);
    RCMVS_REQUIRE((verts || nv == 0) && (faces || nf == 0), "tsdf_sp_mesh_emit: null pointer (verts / faces)");
    RCMVS_REQUIRE(!vert_rgb || (csum_r && csum_g && csum_b), "tsdf_sp_mesh_emit: null pointer (vert_rgb needs the three colour planes)");
    long long blocks;
    if (int rc = sp_bdims(bdims_host, "tsdf_sp_mesh_emit", &blocks)) return rc;
    if (int rc = sp_active("tsdf_sp_mesh_emit", n_active, blocks)) return rc;
    RCMVS_REQUIRE(min_weight >= 1, "tsdf_sp_mesh_emit: min_weight = %d (>= 1)", min_weight);
    tsdf_sp::BlockGrid g;
    if (int rc = sp_grid(grid_host, bdims_host, "tsdf_sp_mesh_emit", &g)) return rc;
    const SpTable t = {mask_words, word_rank, active, n_active, bdims_host[0], bdims_host[1], bdims_host[2]};
    RCMVS_LAUNCH_TIMED(tsdf_sp_emit_kernel, dim3(n_active), dim3(TM_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0),
                       static_cast<hipEvent_t>(ev1), dsum, wsum, csum_r, csum_g, csum_b, g, t, (float)min_weight, edge_mask, tri_count, vert_start,
                       tri_start, (int)nv, (int)nf, verts, vert_rgb, faces);
    return launch_status("tsdf_sp_mesh_emit");
}

extern "C" int rcmvs_tsdf_sp_mesh_emit(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                                       const double* grid_host, const int* bdims_host, const unsigned int* mask_words, const unsigned int* word_rank,
                                       const int* active, int n_active, int min_weight, const unsigned char* edge_mask, const unsigned char* tri_count,
                                       const int* vert_start, const int* tri_start, long long nv, long long nf, float* verts, unsigned char* vert_rgb,
                                       int* faces, void* stream) {
    return rcmvs_tsdf_sp_mesh_emit_timed(dsum, wsum, csum_r, csum_g, csum_b, grid_host, bdims_host, mask_words, word_rank, active, n_active, min_weight,
                                         edge_mask, tri_count, vert_start, tri_start, nv, nf, verts, vert_rgb, faces, nullptr, nullptr, stream);
}
