// Mesh texturing: one view per face, a size class per face, a Morton atlas, the texel fill and the textured pass over rendered views
// (rc_mvsnet_amd/mesh_texture.py; contract in mesh_texture.h, the per-element rules in mesh_texture_math.h).
//
//   vote    per view: a thread per pixel of the render's face image counts the face's samples (the only atomic, an integer add);
//           a thread per face projects the face and, in an eligible view with samples, raises best[f] to (count, -view).
//   class   a thread per face: seen or unseen, the size class from the longest lattice edge in the chosen view, the sort key.
//   sort    one stable 8-bit radix pass (scan_sort.hip's histogram, scan and scatter) on MAX_CLASS - k: classes descend, a class
//           keeps face order.
//   table   one thread: per class its start, faces, cells and Morton base; the total and the atlas size.
//   texel   a thread per sorted position: the face's cell and half, the texel centres of its corners.
//   fill    a thread per Morton index of the atlas: consecutive threads are in one cell; the class from at most nine bases, the
//           face through the sorted order, the colour from the chosen view's image or from the vertex colours.
//   shade   a thread per pixel of a rendered view: the face the render saw, projected again, the atlas sampled at the
//           perspective-correct texel position.
// Counters are integer adds, one per workgroup and counter.  No kernel waits for another workgroup, and there are no floating-point
// atomics.  gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_texture.h"
#include "mesh_texture_math.h"
#include "scan_sort.h"                                            // gid, blocks, buffers_overlap, radix_sort, zero_kernel

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MT_BLOCK = SS_BLOCK;
static_assert(MT_BLOCK == RCMVS_MT_SORT_BLOCK, "a sort block is one workgroup's threads");
static_assert(mt::MIN_CLASS == RCMVS_MT_MIN_CLASS && mt::MAX_CLASS == RCMVS_MT_MAX_CLASS && mt::MAX_SHIFT == RCMVS_MT_MAX_SHIFT, "the constants of mesh_texture.h");
static_assert(mt::PER_CLASS + mt::CLASSES <= RCMVS_MT_STATS && mt::T_SY < RCMVS_MT_TABLE && RCMVS_MT_STATS <= MT_BLOCK, "the tables of mesh_texture.h");

using u64 = unsigned long long;

__device__ inline mr::Proj mt_project(const double* cam, double near_z, const float* __restrict__ verts, int i) {
    return mr::project(cam, near_z, mr::camera(cam, verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2]));
}

// every lane adds one to at most one counter (what; -1: none): a histogram in LDS, then one atomic per counter that is not zero
__device__ inline void mt_count(int what, u64* stats, unsigned* sh) {
    if (threadIdx.x < RCMVS_MT_STATS) sh[threadIdx.x] = 0;
    __syncthreads();
    if (what >= 0) atomicAdd(&sh[what], 1u);
    __syncthreads();
    if (threadIdx.x < RCMVS_MT_STATS && sh[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (u64)sh[threadIdx.x]);
}

// ---- vote ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_count_kernel(const int* __restrict__ face_image, long long pixels, int nf, int* count) {
    const long long p = gid();
    if (p >= pixels) return;
    const int f = face_image[p];
    if ((unsigned)f < (unsigned)nf) atomicAdd(&count[f], 1);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_best_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf, mr::Cam cam, double near_z,
                                                           int H, int W, unsigned view, const int* __restrict__ count, u64* __restrict__ best) {
    const long long f = gid();
    if (f >= nf) return;
    const int n = count[f];
    if (n <= 0) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!mc::face_valid(a, b, c, nv)) return;
    const mr::Proj pa = mt_project(cam.c, near_z, verts, a), pb = mt_project(cam.c, near_z, verts, b), pc = mt_project(cam.c, near_z, verts, c);
    if (!mt::eligible(pa, pb, pc, H, W)) return;
    const u64 key = mt::vote_key((unsigned)n, view), old = best[f];
    if (key > old) best[f] = key;
}

// ---- classes ------------------------------------------------------------------------------------------------------------------------
// the face's chosen view when it is seen there: the key names a view below V in which the face is eligible
__device__ inline bool mt_seen(const float* __restrict__ verts, int a, int b, int c, u64 key, int V, int H, int W, const double* __restrict__ cams, double near_z,
                               int* view, mr::Proj* pa, mr::Proj* pb, mr::Proj* pc) {
    if (!mt::chosen_view(key, V, view)) return false;
    const double* cam = cams + 16 * (size_t)*view;
    *pa = mt_project(cam, near_z, verts, a);
    *pb = mt_project(cam, near_z, verts, b);
    *pc = mt_project(cam, near_z, verts, c);
    return mt::eligible(*pa, *pb, *pc, H, W);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_class_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf, int V, int H, int W,
                                                            const double* __restrict__ cams, double near_z, const u64* __restrict__ best, int shift,
                                                            int* __restrict__ klass, unsigned* __restrict__ key, int* __restrict__ idx, u64* stats) {
    __shared__ unsigned sh[RCMVS_MT_STATS];
    const long long f = gid();
    int what = -1, k = 0, capped = 0;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (!mc::face_valid(a, b, c, nv)) what = mt::INVALID;
        else {
            int view;
            mr::Proj pa, pb, pc;
            if (mt_seen(verts, a, b, c, best[f], V, H, W, cams, near_z, &view, &pa, &pb, &pc)) {
                what = mt::SEEN;
                k = mt::size_class(mt::longest_edge2(pa, pb, pc), shift, &capped);
            } else {
                what = mt::UNSEEN;
                k = mt::MIN_CLASS;
            }
        }
        klass[f] = k;
        key[f] = k ? (unsigned)(mt::MAX_CLASS - k) : mt::SENTINEL;
        idx[f] = (int)f;
    }
    mt_count(what, stats, sh);
    mt_count(k ? mt::PER_CLASS + k : -1, stats, sh);
    mt_count(capped ? mt::CAPPED : -1, stats, sh);
}

__global__ void mt_table_kernel(const u64* __restrict__ stats, long long* __restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < RCMVS_MT_TABLE; ++i) table[i] = 0;
    mt::layout_table(stats + mt::PER_CLASS, table);
}

// key and order are this call's own work; they are still tested before they are used
__global__ __launch_bounds__(MT_BLOCK) void mt_texel_kernel(const unsigned* __restrict__ key, const int* __restrict__ order, int nf, const long long* __restrict__ table,
                                                            int* __restrict__ texel) {
    const long long p = gid();
    if (p >= nf) return;
    const int f = order[p];
    if ((unsigned)f >= (unsigned)nf) return;
    int t[6] = {0, 0, 0, 0, 0, 0};
    const unsigned d = key[p];
    if (d <= (unsigned)(mt::MAX_CLASS - mt::MIN_CLASS)) {
        const int k = mt::MAX_CLASS - (int)d;
        const long long r = p - table[4 * k + mt::T_START];
        if (r >= 0 && r < table[4 * k + mt::T_COUNT]) mt::corner_texels(table[4 * k + mt::T_BASE], r, k, t);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) texel[6 * (size_t)f + q] = t[q];
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_fill_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ rgb, const int* __restrict__ faces, int nv,
                                                           int nf, int V, int H, int W, const double* __restrict__ cams, double near_z,
                                                           const unsigned char* __restrict__ images, const u64* __restrict__ best, const int* __restrict__ order,
                                                           const long long* __restrict__ table, int S, int Sy, int background, unsigned char* __restrict__ atlas,
                                                           int* __restrict__ owner, u64* stats) {
    __shared__ unsigned sh[RCMVS_MT_STATS];
    const long long m = gid();
    int what = -1;
    if (m < (long long)S * Sy) {
        const int x = mt::morton_x(m), y = mt::morton_y(m);
        unsigned char col[3] = {(unsigned char)(background & 255), (unsigned char)((background >> 8) & 255), (unsigned char)((background >> 16) & 255)};
        int own = -1;
        mt::Texel t;
        if (table[mt::T_S] == S && table[mt::T_SY] == Sy && mt::locate(table, m, &t) && t.pos >= 0 && t.pos < nf) {
            const int f = order[t.pos];
            if ((unsigned)f < (unsigned)nf) {
                const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
                if (mc::face_valid(a, b, c, nv)) {
                    own = f;
                    const mt::Weights w = mt::texel_weights(t.ip, t.jp, (1 << t.k) - 3);
                    int view;
                    mr::Proj pa, pb, pc;
                    what = mt::TEX_VERTEX;
                    if (mt_seen(verts, a, b, c, best[f], V, H, W, cams, near_z, &view, &pa, &pb, &pc)) {
                        const double* cam = cams + 16 * (size_t)view;
                        const double px = mt::mix(w, (double)verts[3 * (size_t)a], (double)verts[3 * (size_t)b], (double)verts[3 * (size_t)c]);
                        const double py = mt::mix(w, (double)verts[3 * (size_t)a + 1], (double)verts[3 * (size_t)b + 1], (double)verts[3 * (size_t)c + 1]);
                        const double pz = mt::mix(w, (double)verts[3 * (size_t)a + 2], (double)verts[3 * (size_t)b + 2], (double)verts[3 * (size_t)c + 2]);
                        double u, v;
                        what = mt::TEX_FALLBACK;
                        if (mt::image_position(cam, near_z, mt::camera_d(cam, px, py, pz), H, W, &u, &v)) {
                            what = mt::TEX_IMAGE;
                            const mt::Tap tp = mt::tap(u, v, H, W);
                            const unsigned char* img = images + (size_t)view * H * W * 3;
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) col[ch] = mt::bilinear(img, W, tp, ch);
                        }
                    }
                    if (what != mt::TEX_IMAGE) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            col[ch] = rgb ? mt::vertex_colour(w, rgb[3 * (size_t)a + ch], rgb[3 * (size_t)b + ch], rgb[3 * (size_t)c + ch]) : (unsigned char)255;
                    }
                }
            }
        }
        if (x < S && y < Sy) {
            const size_t at = (size_t)y * S + x;
            atlas[3 * at] = col[0];
            atlas[3 * at + 1] = col[1];
            atlas[3 * at + 2] = col[2];
            owner[at] = own;
        }
    }
    mt_count(what, stats, sh);
}

// ---- the textured pass --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_shade_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf, mr::Cam cam, double near_z,
                                                            int H, int W, const int* __restrict__ face_image, const int* __restrict__ texel,
                                                            const unsigned char* __restrict__ atlas, int S, int Sy, int background, unsigned char* __restrict__ tex_rgb) {
    const long long p = gid(), pixels = (long long)H * W;
    if (p >= pixels) return;
    unsigned char col[3] = {(unsigned char)(background & 255), (unsigned char)((background >> 8) & 255), (unsigned char)((background >> 16) & 255)};
    const int f = face_image[p];
    if ((unsigned)f < (unsigned)nf) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (mc::face_valid(a, b, c, nv)) {
            const mr::Proj pa = mt_project(cam.c, near_z, verts, a), pb = mt_project(cam.c, near_z, verts, b), pc = mt_project(cam.c, near_z, verts, c);
            const long long a2 = mr::area2(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y);
            if (pa.usable && pb.usable && pc.usable && a2 != 0) {
                const mr::Face fc = mr::face(pa, pb, pc, a2);
                int t[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) t[q] = texel[6 * (size_t)f + q];
                const long long row = p / W;
                double tx, ty;
                if (mt::atlas_position(fc, (int)(p - row * W), (int)row, t, Sy, S, &tx, &ty)) {
                    const mt::Tap tp = mt::tap(tx, ty, Sy, S);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) col[ch] = mt::bilinear(atlas, S, tp, ch);
                }
            }
        }
    }
    tex_rgb[3 * p] = col[0];
    tex_rgb[3 * p + 1] = col[1];
    tex_rgb[3 * p + 2] = col[2];
}

static int mt_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0, "%s: nv = %d vertices (0 .. 2^31-1)", what, nv);
    RCMVS_REQUIRE(nf >= 0 && nf <= RCMVS_MT_MAX_FACES, "%s: nf = %d faces (0 .. 2^30-256)", what, nf);
    return 0;
}

static int mt_view(const char* what, int H, int W, double near_z) {
    RCMVS_REQUIRE(H >= 1 && H <= mr::MAX_SIDE, "%s: H = %d (1 .. %d)", what, H, mr::MAX_SIDE);
    RCMVS_REQUIRE(W >= 1 && W <= mr::MAX_SIDE, "%s: W = %d (1 .. %d)", what, W, mr::MAX_SIDE);
    RCMVS_REQUIRE(near_z > 0.0 && near_z <= mt::F64_MAX, "%s: near_z = %g (finite and > 0)", what, near_z);
    return 0;
}

static int mt_atlas(const char* what, int S, int Sy) {
    RCMVS_REQUIRE(S >= 1 && S <= RCMVS_MT_MAX_ATLAS && (S & (S - 1)) == 0, "%s: S = %d (a power of two, 1 .. %d)", what, S, RCMVS_MT_MAX_ATLAS);
    RCMVS_REQUIRE(Sy == S || (S >= 2 && Sy == S / 2), "%s: Sy = %d (S or S / 2 of S = %d)", what, Sy, S);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_mt_vote_timed(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z,
                                   const int* face_image, int first_view, int reset, int* count, u64* best, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "mt_vote";
    if (int rc = mt_sizes(what, nv, nf)) return rc;
    RCMVS_REQUIRE(n >= 1, "%s: n = %d views (at least 1)", what, n);
    if (int rc = mt_view(what, H, W, near_z)) return rc;
    RCMVS_REQUIRE(first_view >= 0 && (long long)first_view + n <= 2147483647ll, "%s: first_view = %d (>= 0, first_view + n below 2^31)", what, first_view);
    RCMVS_REQUIRE(phase == RCMVS_MT_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    RCMVS_REQUIRE(cams_host && face_image, "%s: null pointer (cams_host, face_image)", what);
    RCMVS_REQUIRE(nv == 0 || verts, "%s: null pointer (verts)", what);
    RCMVS_REQUIRE(nf == 0 || (faces && count && best), "%s: null pointer (faces, count and best hold nf elements)", what);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(best) & 7) == 0, "%s: best must be 8-byte aligned", what);
    const size_t pixels = (size_t)H * (size_t)W;
    {
        const void* ptr[] = {count, best, verts, faces, face_image};
        const size_t len[] = {(size_t)nf * 4, (size_t)nf * 8, (size_t)nv * 12, (size_t)nf * 12, pixels * (size_t)n * 4};
        if (int rc = buffers_overlap(what, ptr, len, 2, 5)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    if (reset) {
        RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(blocks(nf)), dim3(MT_BLOCK), 0, st, e0, none, best, (long long)nf);
        e0 = none;
    }
    for (int v = 0; v < n; ++v) {
        mr::Cam cam;
        for (int k = 0; k < 16; ++k) cam.c[k] = cams_host[16 * (size_t)v + k];
        RCMVS_LAUNCH_TIMED(zero_kernel<int>, dim3(blocks(nf)), dim3(MT_BLOCK), 0, st, v == 0 ? e0 : none, none, count, (long long)nf);
        hipLaunchKernelGGL(mt_count_kernel, dim3(blocks((long long)pixels)), dim3(MT_BLOCK), 0, st, face_image + (size_t)v * pixels, (long long)pixels, nf, count);
        RCMVS_LAUNCH_TIMED(mt_best_kernel, dim3(blocks(nf)), dim3(MT_BLOCK), 0, st, none, v == n - 1 ? e1 : none, verts, faces, nv, nf, cam, near_z, H, W,
                           (unsigned)(first_view + v), count, best);
    }
    return launch_status(what);
}

extern "C" int rcmvs_mt_vote(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z, const int* face_image,
                             int first_view, int reset, int* count, u64* best, void* stream) {
    return rcmvs_mt_vote_timed(verts, faces, nv, nf, n, H, W, cams_host, near_z, face_image, first_view, reset, count, best, RCMVS_MT_PHASE_ALL, nullptr, nullptr,
                               stream);
}

extern "C" int rcmvs_mt_layout_timed(const float* verts, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev, double near_z, const u64* best,
                                     int shift, int* klass, unsigned* key_a, int* idx_a, unsigned* key_b, int* order, int* hist, int* hist_start, int* scan_work,
                                     long long* table, int* texel, u64* stats, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "mt_layout";
    if (int rc = mt_sizes(what, nv, nf)) return rc;
    RCMVS_REQUIRE(V >= 1, "%s: V = %d views (at least 1)", what, V);
    if (int rc = mt_view(what, H, W, near_z)) return rc;
    RCMVS_REQUIRE(shift >= 0 && shift <= RCMVS_MT_MAX_SHIFT, "%s: shift = %d (0 .. %d)", what, shift, RCMVS_MT_MAX_SHIFT);
    RCMVS_REQUIRE(phase == RCMVS_MT_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    RCMVS_REQUIRE(cams_dev && table && stats, "%s: null pointer (cams_dev, table, stats)", what);
    RCMVS_REQUIRE(nv == 0 || verts, "%s: null pointer (verts)", what);
    RCMVS_REQUIRE(nf == 0 || (faces && best && klass && key_a && idx_a && key_b && order && hist && hist_start && texel),
                  "%s: null pointer (faces, best, klass, key_a, idx_a, key_b, order, hist, hist_start and texel serve nf faces)", what);
    RCMVS_REQUIRE(scan_work, "%s: null pointer (scan_work)", what);
    if (int rc = scan_work_check(what, scan_work)) return rc;
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(best) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(cams_dev) & 7) == 0, "%s: stats, table, best and cams_dev must be 8-byte aligned", what);
    const long long n = nf, nblk = cdiv(n, MT_BLOCK), cells = 256 * nblk;
    {
        const void* ptr[] = {klass, key_a, idx_a, key_b, order, hist, hist_start, table, texel, stats, verts, faces, best, cams_dev};
        const size_t len[] = {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)cells * 4, (size_t)(cells + 1) * 4,
                              (size_t)RCMVS_MT_TABLE * 8, (size_t)n * 24, (size_t)RCMVS_MT_STATS * 8, (size_t)nv * 12, (size_t)n * 12, (size_t)n * 8, (size_t)V * 128};
        if (int rc = buffers_overlap(what, ptr, len, 10, 14)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MT_BLOCK), 0, st, e0, none, stats, (long long)RCMVS_MT_STATS);
    hipLaunchKernelGGL(mt_class_kernel, dim3(blocks(n)), dim3(MT_BLOCK), 0, st, verts, faces, nv, nf, V, H, W, cams_dev, near_z, best, shift, klass, key_a, idx_a,
                       stats);
    radix_sort<unsigned>(&key_a, &idx_a, &key_b, &order, n, 1, hist, hist_start, scan_work, st);      // one pass: sorted into key_b / order, now *key_a / *idx_a
    hipLaunchKernelGGL(mt_table_kernel, dim3(1), dim3(64), 0, st, stats, table);
    RCMVS_LAUNCH_TIMED(mt_texel_kernel, dim3(blocks(n)), dim3(MT_BLOCK), 0, st, none, e1, key_a, idx_a, nf, table, texel);
    return launch_status(what);
}

extern "C" int rcmvs_mt_layout(const float* verts, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev, double near_z, const u64* best,
                               int shift, int* klass, unsigned* key_a, int* idx_a, unsigned* key_b, int* order, int* hist, int* hist_start, int* scan_work,
                               long long* table, int* texel, u64* stats, void* stream) {
    return rcmvs_mt_layout_timed(verts, faces, nv, nf, V, H, W, cams_dev, near_z, best, shift, klass, key_a, idx_a, key_b, order, hist, hist_start, scan_work, table,
                                 texel, stats, RCMVS_MT_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mt_fill_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev,
                                   double near_z, const unsigned char* images, const u64* best, const int* order, const long long* table, int S, int Sy,
                                   int background, unsigned char* atlas, int* owner, u64* stats, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "mt_fill";
    if (int rc = mt_sizes(what, nv, nf)) return rc;
    RCMVS_REQUIRE(V >= 1, "%s: V = %d views (at least 1)", what, V);
    if (int rc = mt_view(what, H, W, near_z)) return rc;
    if (int rc = mt_atlas(what, S, Sy)) return rc;
    RCMVS_REQUIRE(background >= 0 && background <= 0xffffff, "%s: background = %d (r | g << 8 | b << 16)", what, background);
    RCMVS_REQUIRE(phase == RCMVS_MT_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    RCMVS_REQUIRE(cams_dev && images && table && atlas && owner && stats, "%s: null pointer (cams_dev, images, table, atlas, owner, stats)", what);
    RCMVS_REQUIRE(nv == 0 || verts, "%s: null pointer (verts)", what);
    RCMVS_REQUIRE(nf == 0 || (faces && best && order), "%s: null pointer (faces, best and order hold nf elements)", what);
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(best) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(cams_dev) & 7) == 0, "%s: stats, table, best and cams_dev must be 8-byte aligned", what);
    const size_t texels = (size_t)S * (size_t)Sy;
    {
        const void* ptr[] = {atlas, owner, stats, verts, rgb, faces, cams_dev, images, best, order, table};
        const size_t len[] = {texels * 3, texels * 4, (size_t)RCMVS_MT_STATS * 8, (size_t)nv * 12, (size_t)nv * 3, (size_t)nf * 12, (size_t)V * 128,
                              (size_t)V * H * W * 3, (size_t)nf * 8, (size_t)nf * 4, (size_t)RCMVS_MT_TABLE * 8};
        if (int rc = buffers_overlap(what, ptr, len, 3, 11)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MT_BLOCK), 0, st, e0, none, stats + mt::TEX_IMAGE, 4ll);
    RCMVS_LAUNCH_TIMED(mt_fill_kernel, dim3(blocks((long long)texels)), dim3(MT_BLOCK), 0, st, none, e1, verts, rgb, faces, nv, nf, V, H, W, cams_dev, near_z, images,
                       best, order, table, S, Sy, background, atlas, owner, stats);
    return launch_status(what);
}

extern "C" int rcmvs_mt_fill(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev,
                             double near_z, const unsigned char* images, const u64* best, const int* order, const long long* table, int S, int Sy, int background,
                             unsigned char* atlas, int* owner, u64* stats, void* stream) {
    return rcmvs_mt_fill_timed(verts, rgb, faces, nv, nf, V, H, W, cams_dev, near_z, images, best, order, table, S, Sy, background, atlas, owner, stats,
                               RCMVS_MT_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mt_shade_timed(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z,
                                    const int* face_image, const int* texel, const unsigned char* atlas, int S, int Sy, int background, unsigned char* tex_rgb,
                                    int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "mt_shade";
    if (int rc = mt_sizes(what, nv, nf)) return rc;
    RCMVS_REQUIRE(n >= 1, "%s: n = %d views (at least 1)", what, n);
    if (int rc = mt_view(what, H, W, near_z)) return rc;
    if (int rc = mt_atlas(what, S, Sy)) return rc;
    RCMVS_REQUIRE(background >= 0 && background <= 0xffffff, "%s: background = %d (r | g << 8 | b << 16)", what, background);
    RCMVS_REQUIRE(phase == RCMVS_MT_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    RCMVS_REQUIRE(cams_host && face_image && atlas && tex_rgb, "%s: null pointer (cams_host, face_image, atlas, tex_rgb)", what);
    RCMVS_REQUIRE(nv == 0 || verts, "%s: null pointer (verts)", what);
    RCMVS_REQUIRE(nf == 0 || (faces && texel), "%s: null pointer (faces and texel hold nf rows)", what);
    const size_t pixels = (size_t)H * (size_t)W, all = pixels * (size_t)n;
    {
        const void* ptr[] = {tex_rgb, verts, faces, face_image, texel, atlas};
        const size_t len[] = {all * 3, (size_t)nv * 12, (size_t)nf * 12, all * 4, (size_t)nf * 24, (size_t)S * Sy * 3};
        if (int rc = buffers_overlap(what, ptr, len, 1, 6)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    for (int v = 0; v < n; ++v) {
        mr::Cam cam;
        for (int k = 0; k < 16; ++k) cam.c[k] = cams_host[16 * (size_t)v + k];
        RCMVS_LAUNCH_TIMED(mt_shade_kernel, dim3(blocks((long long)pixels)), dim3(MT_BLOCK), 0, st, v == 0 ? e0 : none, v == n - 1 ? e1 : none, verts, faces, nv, nf,
                           cam, near_z, H, W, face_image + (size_t)v * pixels, texel, atlas, S, Sy, background, tex_rgb + (size_t)v * pixels * 3);
    }
    return launch_status(what);
}

extern "C" int rcmvs_mt_shade(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z, const int* face_image,
                              const int* texel, const unsigned char* atlas, int S, int Sy, int background, unsigned char* tex_rgb, void* stream) {
    return rcmvs_mt_shade_timed(verts, faces, nv, nf, n, H, W, cams_host, near_z, face_image, texel, atlas, S, Sy, background, tex_rgb, RCMVS_MT_PHASE_ALL, nullptr,
                                nullptr, stream);
}
