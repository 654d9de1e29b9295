// The mesh rasteriser: a triangle mesh into the cameras of a scan -- depth, face number, colour, shade -- and the comparison of a
// rendered depth map with a depth map (rc_mvsnet_amd/mesh_render.py; contract in mesh_render.h, the per-element rules in
// mesh_render_math.h).
//
//   clear      keys = all ones, the view's counters and the list's count = 0.
//   project    one thread per vertex: camera-frame position in fp64, the lattice coordinates, zc -> proj_work.
//   small      one lane per face: validity, usable vertices, area2, culling, the clamped bounding box.  A box of at most 8 x 8
//              pixels is walked by the lane; a larger face is appended to the list (integer atomicAdd).  TSDF faces are a few
//              pixels across, so the lanes of a wave walk boxes of like size; the limit bounds what one lane can hold a wave for.
//   large      one workgroup per listed face (a grid-stride loop over the list, RCMVS_MR_LARGE_SLICES workgroups sharing a face's
//              samples): thread t takes the samples t, t + 256 S, ... of the box in row-major order.
//   resolve    one thread per pixel: the key's depth bits and face number, the weights once more by the same function, colour, shade.
//   compare    per-tile counts and fp64 partial sums in a fixed order, then one workgroup per view.
// The only atomic on an image is the 64-bit integer atomicMin of the keys, after a plain load that skips a key that cannot win;
// counters are integer adds, one per workgroup.  No kernel waits for another workgroup, and there are no floating-point atomics.
// gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_render.h"
#include "mesh_render_math.h"
#include "scan_sort.h"                                            // gid, blocks, the overlap checks
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MR_BLOCK = TM_BLOCK;
constexpr int MR_LARGE_GRID = 1024;                               // workgroups that walk the list, each RCMVS_MR_LARGE_SLICES times
constexpr int MR_CMP_PER = RCMVS_MR_CMP_TILE / MR_BLOCK;

using u64 = unsigned long long;

static_assert(sizeof(mr::Proj) == RCMVS_MR_PROJ_BYTES, "proj_work holds one mr::Proj per vertex");
static_assert(mr::SMALL_SIDE == RCMVS_MR_SMALL_SIDE && mr::MAX_SIDE == RCMVS_MR_MAX_SIDE && mr::NONE == RCMVS_MR_CULL_NONE && mr::BACK == RCMVS_MR_CULL_BACK,
              "the constants of mesh_render.h");
static_assert(mr::COVERED < RCMVS_MR_STATS && RCMVS_MR_TRACE == 10 && RCMVS_MR_TABLE == 8, "the tables of mesh_render.h");
static_assert(MR_BLOCK == SS_BLOCK, "gid and blocks count in this family's block");

// ---- clear, project -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_clear_kernel(u64* __restrict__ keys, long long pixels, u64* __restrict__ stats, int* __restrict__ list) {
    for (long long i = gid(); i < pixels; i += (long long)gridDim.x * MR_BLOCK) keys[i] = mr::EMPTY;
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < RCMVS_MR_STATS) stats[threadIdx.x] = 0;
        if (threadIdx.x == 0) list[0] = 0;
    }
}

__global__ __launch_bounds__(MR_BLOCK) void mr_project_kernel(const float* __restrict__ verts, int nv, mr::Cam cam, double near_z, mr::Proj* __restrict__ proj) {
    const long long v = gid();
    if (v >= nv) return;
    proj[v] = mr::project(cam.c, near_z, mr::camera(cam.c, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]));
}

// ---- raster ---------------------------------------------------------------------------------------------------------------------
// One sample of one face: inside, a depth, and a key smaller than the one read -> the atomic.  x, y lie inside the image (the box
// is clamped), so the address is inside keys.  -> bit 0: inside with a depth, bit 1: the atomic was issued
__device__ inline unsigned mr_sample(const mr::Face& f, int face_number, int x, int y, int W, u64* keys) {
    long long w[3];
    if (!mr::weights(f, x, y, w)) return 0;
    float d;
    if (!mr::depth(f, w, &d)) return 0;
    const u64 k = mr::key(d, face_number);
    u64* cell = keys + ((size_t)y * (size_t)W + (size_t)x);
    if (!(k < *cell)) return 1;
    atomicMin(cell, k);
    return 3;
}

__device__ inline int mr_histogram_bin(int side) {
    return side <= 0 ? 0 : side == 1 ? 1 : side == 2 ? 2 : side <= 4 ? 3 : side <= 8 ? 4 : side <= 16 ? 5 : side <= 64 ? 6 : 7;
}

__global__ __launch_bounds__(MR_BLOCK) void mr_small_kernel(const int* __restrict__ faces, int nv, int nf, const mr::Proj* __restrict__ proj, int H, int W, int cull,
                                                            u64* keys, int* list, u64* stats, u64* trace) {
    __shared__ unsigned sh[MR_BLOCK];
    const long long f = gid();
    int what = -1;                                                // the counter this face adds to
    unsigned inside = 0, issued = 0, large = 0;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (!mc::face_valid(a, b, c, nv)) what = mr::INVALID;
        else {
            const mr::Proj pa = proj[a], pb = proj[b], pc = proj[c];
            if (!(pa.usable && pb.usable && pc.usable)) what = mr::CLIPPED;
            else {
                const long long a2 = mr::area2(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y);
                if (a2 == 0) what = mr::DEGENERATE;
                else if (cull == mr::BACK && a2 > 0) what = mr::CULLED;
                else {
                    what = mr::DRAWN;
                    const mr::Box bx = mr::box(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y, H, W);
                    const bool empty = mr::box_empty(bx);
                    if (trace) {
                        const int side = empty ? 0 : (bx.x1 - bx.x0 > bx.y1 - bx.y0 ? bx.x1 - bx.x0 : bx.y1 - bx.y0) + 1;
                        atomicAdd(&trace[2 + mr_histogram_bin(side)], (u64)1);
                    }
                    if (!empty && !mr::box_small(bx)) {
                        large = 1;
                        list[1 + atomicAdd(&list[0], 1)] = (int)f;       // at most nf appends: the slot lies inside the nf + 1 ints
                    } else if (!empty) {
                        const mr::Face fc = mr::face(pa, pb, pc, a2);
                        for (int y = bx.y0; y <= bx.y1; ++y)
                            for (int x = bx.x0; x <= bx.x1; ++x) {
                                const unsigned r = mr_sample(fc, (int)f, x, y, W, keys);
                                inside += r & 1;
                                issued += r >> 1;
                            }
                    }
                }
            }
        }
    }
    // six counters of at most 256 each, ten bits apiece in two block sums: counter k in word k / 3 at bit 10 (k % 3)
    const unsigned lo = what >= 0 && what < 3 ? 1u << (10 * what) : 0u;
    const unsigned hi = (what >= 3 ? 1u << (10 * (what - 3)) : 0u) | (large << (10 * (mr::LARGE - 3)));
    const unsigned slo = tm_block_sum(lo, sh), shi = tm_block_sum(hi, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k <= mr::LARGE; ++k) {
            const unsigned s = ((k < 3 ? slo : shi) >> (10 * (k % 3))) & 1023u;
            if (s) atomicAdd(&stats[k], (u64)s);
        }
    }
    if (trace) {
        const unsigned si = tm_block_sum(inside, sh), sa = tm_block_sum(issued, sh);
        if (threadIdx.x == 0) {
            if (si) atomicAdd(&trace[0], (u64)si);
            if (sa) atomicAdd(&trace[1], (u64)sa);
        }
    }
}

// blockIdx.x walks the list, blockIdx.y is the slice of a face's samples.  The list holds faces that passed every test.
__global__ __launch_bounds__(MR_BLOCK) void mr_large_kernel(const int* __restrict__ faces, int nv, int nf, const mr::Proj* __restrict__ proj, int H, int W,
                                                            u64* keys, const int* __restrict__ list, u64* trace) {
    __shared__ unsigned sh[MR_BLOCK];
    int count = list[0];
    if (count > nf) count = nf;
    unsigned inside = 0, issued = 0;
    for (int e = (int)blockIdx.x; e < count; e += (int)gridDim.x) {
        const int f = list[1 + e];
        if ((unsigned)f >= (unsigned)nf) continue;
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (!mc::face_valid(a, b, c, nv)) continue;
        const mr::Proj pa = proj[a], pb = proj[b], pc = proj[c];
        if (!(pa.usable && pb.usable && pc.usable)) continue;
        const long long a2 = mr::area2(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y);
        if (a2 == 0) continue;
        const mr::Box bx = mr::box(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y, H, W);
        if (mr::box_empty(bx)) continue;
        const mr::Face fc = mr::face(pa, pb, pc, a2);
        const long long bw = bx.x1 - bx.x0 + 1, total = bw * (long long)(bx.y1 - bx.y0 + 1);
        for (long long i = (long long)blockIdx.y * MR_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.y * MR_BLOCK) {
            const long long row = i / bw;
            const unsigned r = mr_sample(fc, f, bx.x0 + (int)(i - row * bw), bx.y0 + (int)row, W, keys);
            inside += r & 1;
            issued += r >> 1;
        }
    }
    if (trace) {
        const unsigned si = tm_block_sum(inside, sh), sa = tm_block_sum(issued, sh);
        if (threadIdx.x == 0) {
            if (si) atomicAdd(&trace[0], (u64)si);
            if (sa) atomicAdd(&trace[1], (u64)sa);
        }
    }
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_BLOCK) void mr_resolve_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ rgb, const int* __restrict__ faces,
                                                              int nv, int nf, mr::Cam cam, double near_z, int H, int W, const u64* __restrict__ keys, int background,
                                                              float* __restrict__ depth, int* __restrict__ face, unsigned char* __restrict__ out_rgb,
                                                              unsigned char* __restrict__ shade, u64* stats) {
    __shared__ unsigned sh[MR_BLOCK];
    const long long p = gid(), pixels = (long long)H * W;
    unsigned covered = 0;
    if (p < pixels) {
        const u64 k = keys[p];
        float d = 0.0f;
        int f = -1;
        unsigned char col[3] = {(unsigned char)(background & 255), (unsigned char)((background >> 8) & 255), (unsigned char)((background >> 16) & 255)};
        unsigned char sd = 0;
        const int kf = (int)(unsigned)(k & 0xffffffffull);
        if (k != mr::EMPTY && (unsigned)kf < (unsigned)nf) {
            const int a = faces[3 * (size_t)kf], b = faces[3 * (size_t)kf + 1], c = faces[3 * (size_t)kf + 2];
            if (mc::face_valid(a, b, c, nv)) {                        // a key is written for a valid face only: never false for keys of this call
                covered = 1;
                d = __builtin_bit_cast(float, (unsigned)(k >> 32));
                f = kf;
                const mr::Point qa = mr::camera(cam.c, verts[3 * (size_t)a], verts[3 * (size_t)a + 1], verts[3 * (size_t)a + 2]);
                const mr::Point qb = mr::camera(cam.c, verts[3 * (size_t)b], verts[3 * (size_t)b + 1], verts[3 * (size_t)b + 2]);
                const mr::Point qc = mr::camera(cam.c, verts[3 * (size_t)c], verts[3 * (size_t)c + 1], verts[3 * (size_t)c + 2]);
                sd = mr::shade(qa, qb, qc);
                col[0] = col[1] = col[2] = 255;
                if (rgb) {
                    const mr::Proj pa = mr::project(cam.c, near_z, qa), pb = mr::project(cam.c, near_z, qb), pc = mr::project(cam.c, near_z, qc);
                    const mr::Face fc = mr::face(pa, pb, pc, mr::area2(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y));
                    long long w[3];
                    const long long row = p / W;
                    mr::weights(fc, (int)(p - row * W), (int)row, w);
                    for (int ch = 0; ch < 3; ++ch)
                        col[ch] = mr::colour(fc, w, rgb[3 * (size_t)a + ch], rgb[3 * (size_t)b + ch], rgb[3 * (size_t)c + ch]);
                }
            }
        }
        depth[p] = d;
        face[p] = f;
        shade[p] = sd;
        out_rgb[3 * p] = col[0];
        out_rgb[3 * p + 1] = col[1];
        out_rgb[3 * p + 2] = col[2];
    }
    const unsigned s = tm_block_sum(covered, sh);
    if (threadIdx.x == 0 && s) atomicAdd(&stats[mr::COVERED], (u64)s);
}

// ---- compare --------------------------------------------------------------------------------------------------------------------
struct MrThresholds {
    double t[3];
    int n;
};

// the sum of v over the block in thread 0, a tree of fixed shape
__device__ inline double mr_block_sum_f64(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = MR_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(MR_BLOCK) void mr_compare_clear_kernel(u64* __restrict__ table, long long cells) {
    const long long i = gid();
    if (i < cells) table[i] = 0;
}

// grid (tiles, n): tile blockIdx.x of view blockIdx.y
__global__ __launch_bounds__(MR_BLOCK) void mr_compare_tile_kernel(const float* __restrict__ rendered, const float* __restrict__ depth, long long pixels,
                                                                   MrThresholds th, double* __restrict__ partial, u64* table) {
    __shared__ unsigned sh[MR_BLOCK];
    __shared__ double shd[MR_BLOCK];
    const size_t view = blockIdx.y;
    const float* r = rendered + view * (size_t)pixels;
    const float* d = depth + view * (size_t)pixels;
    unsigned cnt[6] = {0, 0, 0, 0, 0, 0};
    double sum = 0.0;
    for (int q = 0; q < MR_CMP_PER; ++q) {
        const long long p = (long long)blockIdx.x * RCMVS_MR_CMP_TILE + (long long)q * MR_BLOCK + threadIdx.x;
        if (p >= pixels) break;
        const float rv = r[p], dv = d[p];
        const bool hr = mr::has_depth(rv), hd = mr::has_depth(dv);
        if (hr && hd) {
            const double diff = mr::abs_diff(rv, dv);
            cnt[0] += 1;
            sum = sum + diff;
            for (int k = 0; k < th.n; ++k) cnt[3 + k] += mr::within(diff, th.t[k], dv);
        } else if (hr) cnt[1] += 1;
        else if (hd) cnt[2] += 1;
    }
    for (int k = 0; k < 6; ++k) {
        const unsigned s = tm_block_sum(cnt[k], sh);
        if (threadIdx.x == 0 && s) atomicAdd(&table[view * RCMVS_MR_TABLE + k], (u64)s);
    }
    const double total = mr_block_sum_f64(sum, shd);
    if (threadIdx.x == 0) partial[view * gridDim.x + blockIdx.x] = total;
}

// one workgroup per view: thread t sums the partials t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(MR_BLOCK) void mr_compare_sum_kernel(const double* __restrict__ partial, int tiles, u64* __restrict__ table) {
    __shared__ double shd[MR_BLOCK];
    const size_t view = blockIdx.x;
    double sum = 0.0;
    for (int t = (int)threadIdx.x; t < tiles; t += MR_BLOCK) sum = sum + partial[view * (size_t)tiles + t];
    const double total = mr_block_sum_f64(sum, shd);
    if (threadIdx.x == 0) table[view * RCMVS_MR_TABLE + 6] = __builtin_bit_cast(u64, total);
}

static int mr_size(const char* what, int n, int H, int W) {
    RCMVS_REQUIRE(n >= 1, "%s: n = %d views (at least 1)", what, n);
    RCMVS_REQUIRE(H >= 1 && H <= RCMVS_MR_MAX_SIDE, "%s: H = %d (1 .. %d)", what, H, RCMVS_MR_MAX_SIDE);
    RCMVS_REQUIRE(W >= 1 && W <= RCMVS_MR_MAX_SIDE, "%s: W = %d (1 .. %d)", what, W, RCMVS_MR_MAX_SIDE);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_mr_render_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host,
                                     double near_z, int cull, int background, void* proj_work, int* list_work, u64* keys, float* depth, int* face,
                                     unsigned char* out_rgb, unsigned char* shade, u64* stats, u64* trace, int phase, void* ev0, void* ev1, void* stream) {
    RCMVS_REQUIRE(nv >= 0 && nf >= 0, "mr_render: %d vertices, %d faces (0 .. 2^31-1 each)", nv, nf);
    if (int rc = mr_size("mr_render", n, H, W)) return rc;
    RCMVS_REQUIRE(near_z > 0.0 && near_z <= 1.7976931348623157e308, "mr_render: near_z = %g (finite and > 0)", near_z);
    RCMVS_REQUIRE(cull == RCMVS_MR_CULL_NONE || cull == RCMVS_MR_CULL_BACK, "mr_render: cull = %d (0: none, 1: back)", cull);
    RCMVS_REQUIRE(background >= 0 && background <= 0xffffff, "mr_render: background = %d (r | g << 8 | b << 16)", background);
    RCMVS_REQUIRE(phase >= RCMVS_MR_PHASE_ALL && phase <= RCMVS_MR_PHASE_RESOLVE, "mr_render: phase = %d (0 .. 4)", phase);
    RCMVS_REQUIRE(!rgb || verts, "mr_render: null pointer (rgb needs verts)");
    RCMVS_REQUIRE(cams_host && list_work && keys && depth && face && out_rgb && shade && stats && (nv == 0 || (verts && proj_work)) && (nf == 0 || faces),
                  "mr_render: null pointer");
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(proj_work) & 7) == 0 && (reinterpret_cast<uintptr_t>(keys) & 7) == 0, "mr_render: proj_work and keys must be 8-byte aligned");
    const size_t pixels = (size_t)H * (size_t)W, all = pixels * (size_t)n;
    {
        const void* ptr[] = {proj_work, list_work, keys, depth, face, out_rgb, shade, stats, trace, verts, rgb, faces};
        const size_t len[] = {(size_t)nv * RCMVS_MR_PROJ_BYTES, ((size_t)nf + 1) * 4, all * 8, all * 4, all * 4, all * 3, all, (size_t)n * RCMVS_MR_STATS * 8,
                              (size_t)RCMVS_MR_TRACE * 8, (size_t)nv * 12, (size_t)nv * 3, (size_t)nf * 12};
        if (int rc = buffers_overlap("mr_render", ptr, len, 9, 12)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    mr::Proj* proj = static_cast<mr::Proj*>(proj_work);
    for (int v = 0; v < n; ++v) {
        mr::Cam cam;
        for (int k = 0; k < 16; ++k) cam.c[k] = cams_host[16 * (size_t)v + k];
        const bool last = v == n - 1;
        // the events of launch number `which` (0: clear, 1: project, 2: small, 3: large, 4: resolve) of this view
        auto first = [&](int which) {
            if (phase == RCMVS_MR_PHASE_ALL) return v == 0 && which == 1 ? e0 : none;      // project is a view's first launch in the stream
            const int start = phase == RCMVS_MR_PHASE_PROJECT ? 1 : phase == RCMVS_MR_PHASE_SMALL ? 0 : phase == RCMVS_MR_PHASE_LARGE ? 3 : 4;
            return last && which == start ? e0 : none;
        };
        auto stop = [&](int which) {
            if (phase == RCMVS_MR_PHASE_ALL) return last && which == 4 ? e1 : none;
            const int end = phase == RCMVS_MR_PHASE_PROJECT ? 1 : phase == RCMVS_MR_PHASE_SMALL ? 2 : phase == RCMVS_MR_PHASE_LARGE ? 3 : 4;
            return last && which == end ? e1 : none;
        };
        u64* keys_v = keys + (size_t)v * pixels;
        u64* stats_v = stats + (size_t)v * RCMVS_MR_STATS;
        // project before clear in the stream, so that the phase "small" (clear + small) is one run of launches
        RCMVS_LAUNCH_TIMED(mr_project_kernel, dim3(blocks(nv)), dim3(MR_BLOCK), 0, st, first(1), stop(1), verts, nv, cam, near_z, proj);
        RCMVS_LAUNCH_TIMED(mr_clear_kernel, dim3(capped_blocks((long long)pixels)), dim3(MR_BLOCK), 0, st, first(0), stop(0), keys_v, (long long)pixels, stats_v,
                           list_work);
        RCMVS_LAUNCH_TIMED(mr_small_kernel, dim3(blocks(nf)), dim3(MR_BLOCK), 0, st, first(2), stop(2), faces, nv, nf, proj, H, W, cull, keys_v, list_work, stats_v,
                           trace);
        RCMVS_LAUNCH_TIMED(mr_large_kernel, dim3(nf < MR_LARGE_GRID ? (nf > 0 ? nf : 1) : MR_LARGE_GRID, RCMVS_MR_LARGE_SLICES), dim3(MR_BLOCK), 0, st, first(3),
                           stop(3), faces, nv, nf, proj, H, W, keys_v, list_work, trace);
        RCMVS_LAUNCH_TIMED(mr_resolve_kernel, dim3(blocks((long long)pixels)), dim3(MR_BLOCK), 0, st, first(4), stop(4), verts, rgb, faces, nv, nf, cam, near_z, H, W,
                           keys_v, background, depth + (size_t)v * pixels, face + (size_t)v * pixels, out_rgb + (size_t)v * pixels * 3, shade + (size_t)v * pixels,
                           stats_v);
    }
    return launch_status("mr_render");
}

extern "C" int rcmvs_mr_render(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host,
                               double near_z, int cull, int background, void* proj_work, int* list_work, u64* keys, float* depth, int* face, unsigned char* out_rgb,
                               unsigned char* shade, u64* stats, u64* trace, void* stream) {
    return rcmvs_mr_render_timed(verts, rgb, faces, nv, nf, n, H, W, cams_host, near_z, cull, background, proj_work, list_work, keys, depth, face, out_rgb, shade,
                                 stats, trace, RCMVS_MR_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mr_compare_timed(const float* rendered, const float* depth, int n, int H, int W, const double* thresholds_host, int nt, double* partial_work,
                                      u64* table, void* ev0, void* ev1, void* stream) {
    if (int rc = mr_size("mr_compare", n, H, W)) return rc;
    RCMVS_REQUIRE(n <= RCMVS_MR_CMP_MAX_VIEWS, "mr_compare: n = %d views (1 .. %d: a view is a row of the grid)", n, RCMVS_MR_CMP_MAX_VIEWS);
    RCMVS_REQUIRE(nt >= 0 && nt <= 3, "mr_compare: nt = %d thresholds (0 .. 3)", nt);
    RCMVS_REQUIRE(rendered && depth && partial_work && table && (nt == 0 || thresholds_host), "mr_compare: null pointer");
    MrThresholds th = {{0.0, 0.0, 0.0}, nt};
    for (int k = 0; k < nt; ++k) {
        th.t[k] = thresholds_host[k];
        RCMVS_REQUIRE(th.t[k] >= 0.0 && th.t[k] <= 1.7976931348623157e308, "mr_compare: thresholds[%d] = %g (finite and >= 0)", k, th.t[k]);
    }
    const long long pixels = (long long)H * W;
    const int tiles = (int)cdiv(pixels, RCMVS_MR_CMP_TILE);
    RCMVS_REQUIRE(!ranges_overlap(table, (size_t)n * RCMVS_MR_TABLE * 8, partial_work, (size_t)n * tiles * 8) &&
                  !ranges_overlap(table, (size_t)n * RCMVS_MR_TABLE * 8, rendered, (size_t)n * pixels * 4) &&
                  !ranges_overlap(table, (size_t)n * RCMVS_MR_TABLE * 8, depth, (size_t)n * pixels * 4) &&
                  !ranges_overlap(partial_work, (size_t)n * tiles * 8, rendered, (size_t)n * pixels * 4) &&
                  !ranges_overlap(partial_work, (size_t)n * tiles * 8, depth, (size_t)n * pixels * 4), "mr_compare: an output or work buffer overlaps another buffer");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(mr_compare_clear_kernel, dim3(blocks((long long)n * RCMVS_MR_TABLE)), dim3(MR_BLOCK), 0, st, e0, none, table, (long long)n * RCMVS_MR_TABLE);
    hipLaunchKernelGGL(mr_compare_tile_kernel, dim3(tiles, n), dim3(MR_BLOCK), 0, st, rendered, depth, pixels, th, partial_work, table);
    RCMVS_LAUNCH_TIMED(mr_compare_sum_kernel, dim3(n), dim3(MR_BLOCK), 0, st, none, e1, partial_work, tiles, table);
    return launch_status("mr_compare");
}

extern "C" int rcmvs_mr_compare(const float* rendered, const float* depth, int n, int H, int W, const double* thresholds_host, int nt, double* partial_work,
                                u64* table, void* stream) {
    return rcmvs_mr_compare_timed(rendered, depth, n, H, W, thresholds_host, nt, partial_work, table, nullptr, nullptr, stream);
}
