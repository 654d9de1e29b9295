// Mesh normals: face normals, oriented vertex normals under two weights, and the normal pass over rendered views
// (rc_mvsnet_amd/mesh_normals.py; contract in mesh_normals.h, the per-element rules in mesh_normals_math.h).
//
//   face       one thread per face: validity, finiteness, F, the unit normal.
//   key        one thread per face: the keys of its three corners (the vertex, or the sentinel nv for an invalid or skipped face),
//              the corner numbers, and the face's counter.
//   sort       stable 8-bit radix passes over the 3 nf (key, corner) pairs (scan_sort.hip's pass and scan), only as many as nv
//              needs: a vertex's corners become consecutive, in ascending corner number.
//   seg        one thread per sorted pair: where a vertex's segment starts and ends.
//   accumulate one lane per vertex walks its segment and adds the corners' contributions one by one in fp64: the fixed order forbids
//              a tree, and TSDF meshes have 6 to 14 corners at a vertex.
//   shade      one thread per pixel of a rendered view: the face the render saw, projected again, its vertex normals interpolated
//              perspective-correctly and rotated into the camera frame.
// Counters are integer adds, one per workgroup.  No kernel waits for another workgroup, and there are no floating-point atomics.
// gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mesh_normals.h"
#include "mesh_normals_math.h"
#include "scan_sort.h"                                            // gid, blocks, the overlap checks, radix_sort, segments_kernel, zero_kernel
#include "tsdf_mesh_cells.h"                                      // tm_block_sum (256 threads)

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int MN_BLOCK = TM_BLOCK;
static_assert(MN_BLOCK == RCMVS_MN_SORT_BLOCK && MN_BLOCK == SS_BLOCK, "a sort block is one workgroup's threads");
static_assert(mn::AREA == RCMVS_MN_WEIGHT_AREA && mn::SPHERE == RCMVS_MN_WEIGHT_SPHERE && mn::CANCELLED < RCMVS_MN_STATS, "the constants of mesh_normals.h");

using u64 = unsigned long long;

// the three vertices of a valid face into registers
__device__ inline void mn_load(const float* __restrict__ verts, int i, float* p) {
    p[0] = verts[3 * (size_t)i];
    p[1] = verts[3 * (size_t)i + 1];
    p[2] = verts[3 * (size_t)i + 2];
}

// every lane adds one to at most one of the counters first .. first + count - 1 (what; -1: none): a block sum and one atomic each
__device__ inline void mn_count(int what, int first, int count, u64* stats, unsigned* sh) {
    for (int k = first; k < first + count; ++k) {
        const unsigned s = tm_block_sum(what == k ? 1u : 0u, sh);
        if (threadIdx.x == 0 && s) atomicAdd(&stats[k], (u64)s);
    }
}

// ---- face normals -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MN_BLOCK) void mn_face_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf, float* __restrict__ out) {
    const long long f = gid();
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (mc::face_valid(a, b, c, nv)) {
        float pa[3], pb[3], pc[3];
        mn_load(verts, a, pa);
        mn_load(verts, b, pb);
        mn_load(verts, c, pc);
        if (mn::finite9(pa, pb, pc)) mn::unit(mn::face_vector(pa, pb, pc), n);
    }
    out[3 * f] = n[0];
    out[3 * f + 1] = n[1];
    out[3 * f + 2] = n[2];
}

// ---- incidence ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MN_BLOCK) void mn_key_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, int nf,
                                                          unsigned* __restrict__ key, int* __restrict__ idx, u64* stats) {
    __shared__ unsigned sh[MN_BLOCK];
    const long long f = gid();
    int what = -1;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        unsigned ka = (unsigned)nv, kb = (unsigned)nv, kc = (unsigned)nv;
        if (!mc::face_valid(a, b, c, nv)) what = mn::INVALID;
        else {
            float pa[3], pb[3], pc[3];
            mn_load(verts, a, pa);
            mn_load(verts, b, pb);
            mn_load(verts, c, pc);
            if (!mn::finite9(pa, pb, pc)) what = mn::NONFINITE;
            else {
                ka = (unsigned)a;
                kb = (unsigned)b;
                kc = (unsigned)c;
                if (mn::is_zero(mn::face_vector(pa, pb, pc))) what = mn::DEGENERATE;
            }
        }
        key[3 * f] = ka;
        key[3 * f + 1] = kb;
        key[3 * f + 2] = kc;
        idx[3 * f] = (int)(3 * f);
        idx[3 * f + 1] = (int)(3 * f + 1);
        idx[3 * f + 2] = (int)(3 * f + 2);
    }
    mn_count(what, mn::INVALID, 3, stats, sh);
}

// ---- accumulation -------------------------------------------------------------------------------------------------------------------
// seg and idx are this call's own work; they are still tested before they are used as addresses.
__global__ __launch_bounds__(MN_BLOCK) void mn_accumulate_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nv, long long n, int weight,
                                                                 const int* __restrict__ idx, const int* __restrict__ seg, float* __restrict__ normals, u64* stats) {
    __shared__ unsigned sh[MN_BLOCK];
    const long long v = gid();
    int what = -1;
    unsigned skipped = 0;
    if (v < nv) {
        long long i0 = seg[2 * v], i1 = seg[2 * v + 1];
        if (i0 < 0) i0 = 0;
        if (i1 > n) i1 = n;
        mn::Vec s = {0.0, 0.0, 0.0};
        unsigned used = 0;
        for (long long i = i0; i < i1; ++i) {
            const int e = idx[i];
            if ((unsigned)e >= (unsigned)n) continue;
            const int f = e / 3, k = e - 3 * f;
            const int ta = faces[3 * (size_t)f], tb = faces[3 * (size_t)f + 1], tc = faces[3 * (size_t)f + 2];
            if (!mc::face_valid(ta, tb, tc, nv) || (k == 0 ? ta : (k == 1 ? tb : tc)) != (int)v) continue;
            float pa[3], pb[3], pc[3];
            mn_load(verts, ta, pa);
            mn_load(verts, tb, pb);
            mn_load(verts, tc, pc);
            if (!mn::finite9(pa, pb, pc)) continue;
            mn::Vec c;
            if (weight == mn::AREA) c = mn::face_vector(pa, pb, pc);
            else {
                float p[3], q[3], r[3];                               // the corner, the next and the previous vertex: selects, no indexed registers
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    p[j] = k == 0 ? pa[j] : (k == 1 ? pb[j] : pc[j]);
                    q[j] = k == 0 ? pb[j] : (k == 1 ? pc[j] : pa[j]);
                    r[j] = k == 0 ? pc[j] : (k == 1 ? pa[j] : pb[j]);
                }
                if (!mn::sphere_corner(p, q, r, &c)) {
                    ++skipped;
                    continue;
                }
            }
            s = mn::add(s, c);
            ++used;
        }
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (!used) what = mn::UNREFERENCED;
        else what = mn::unit(s, out) ? mn::WITH_NORMAL : mn::CANCELLED;
        normals[3 * v] = out[0];
        normals[3 * v + 1] = out[1];
        normals[3 * v + 2] = out[2];
    }
    mn_count(what, mn::WITH_NORMAL, 3, stats, sh);
    // a lane may skip up to 2^31 corners: the halves of its count are summed apart, so that neither 32-bit block sum can wrap
    const unsigned lo = tm_block_sum(skipped & 0xffffu, sh), hi = tm_block_sum(skipped >> 16, sh);
    if (threadIdx.x == 0 && (lo | hi)) atomicAdd(&stats[mn::SKIPPED], (u64)lo + ((u64)hi << 16));
}

// ---- the normal pass ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MN_BLOCK) void mn_shade_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ normals, int nv,
                                                            int nf, mr::Cam cam, double near_z, int H, int W, const int* __restrict__ face_image, int background,
                                                            float* __restrict__ normal_map, unsigned char* __restrict__ smooth, unsigned char* __restrict__ normal_rgb) {
    const long long p = gid(), pixels = (long long)H * W;
    if (p >= pixels) return;
    mn::Pixel px;
    px.normal[0] = px.normal[1] = px.normal[2] = 0.0f;
    px.smooth = 0;
    px.rgb[0] = (unsigned char)(background & 255);
    px.rgb[1] = (unsigned char)((background >> 8) & 255);
    px.rgb[2] = (unsigned char)((background >> 16) & 255);
    const int f = face_image[p];
    if ((unsigned)f < (unsigned)nf) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (mc::face_valid(a, b, c, nv)) {
            const mr::Proj pa = mr::project(cam.c, near_z, mr::camera(cam.c, verts[3 * (size_t)a], verts[3 * (size_t)a + 1], verts[3 * (size_t)a + 2]));
            const mr::Proj pb = mr::project(cam.c, near_z, mr::camera(cam.c, verts[3 * (size_t)b], verts[3 * (size_t)b + 1], verts[3 * (size_t)b + 2]));
            const mr::Proj pc = mr::project(cam.c, near_z, mr::camera(cam.c, verts[3 * (size_t)c], verts[3 * (size_t)c + 1], verts[3 * (size_t)c + 2]));
            const long long a2 = mr::area2(pa.X, pa.Y, pb.X, pb.Y, pc.X, pc.Y);
            if (pa.usable && pb.usable && pc.usable && a2 != 0) {
                const mr::Face fc = mr::face(pa, pb, pc, a2);
                float na[3], nb[3], nc[3];
                mn_load(normals, a, na);
                mn_load(normals, b, nb);
                mn_load(normals, c, nc);
                const long long row = p / W;
                if (!mn::shade_pixel(cam.c, fc, (int)(p - row * W), (int)row, na, nb, nc, &px)) {
                    px.normal[0] = px.normal[1] = px.normal[2] = 0.0f;
                    px.smooth = 0;
                    px.rgb[0] = px.rgb[1] = px.rgb[2] = 128;
                }
            }
        }
    }
    normal_map[3 * p] = px.normal[0];
    normal_map[3 * p + 1] = px.normal[1];
    normal_map[3 * p + 2] = px.normal[2];
    smooth[p] = px.smooth;
    normal_rgb[3 * p] = px.rgb[0];
    normal_rgb[3 * p + 1] = px.rgb[1];
    normal_rgb[3 * p + 2] = px.rgb[2];
}

static int mn_sizes(const char* what, int nv, int nf) {
    RCMVS_REQUIRE(nv >= 0, "%s: nv = %d vertices (0 .. 2^31-1)", what, nv);
    RCMVS_REQUIRE(nf >= 0 && 3ll * nf <= RCMVS_MN_MAX_CORNERS, "%s: nf = %d faces (0 .. (2^31-256) / 3)", what, nf);
    return 0;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_mn_face_normals_timed(const float* verts, const int* faces, int nv, int nf, float* face_normals, int phase, void* ev0, void* ev1, void* stream) {
    if (int rc = mn_sizes("mn_face_normals", nv, nf)) return rc;
    RCMVS_REQUIRE(phase == RCMVS_MN_PHASE_ALL, "mn_face_normals: phase = %d (0: all)", phase);
    RCMVS_REQUIRE(nv == 0 || verts, "mn_face_normals: null pointer (verts)");
    RCMVS_REQUIRE(nf == 0 || faces, "mn_face_normals: null pointer (faces)");
    RCMVS_REQUIRE(nf == 0 || face_normals, "mn_face_normals: null pointer (face_normals)");
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(face_normals) & 3) == 0, "mn_face_normals: face_normals must be 4-byte aligned");
    RCMVS_REQUIRE(!ranges_overlap(face_normals, (size_t)nf * 12, verts, (size_t)nv * 12) && !ranges_overlap(face_normals, (size_t)nf * 12, faces, (size_t)nf * 12),
                  "mn_face_normals: face_normals overlaps an input");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    RCMVS_LAUNCH_TIMED(mn_face_kernel, dim3(blocks(nf)), dim3(MN_BLOCK), 0, st, e0, e1, verts, faces, nv, nf, face_normals);
    return launch_status("mn_face_normals");
}

extern "C" int rcmvs_mn_face_normals(const float* verts, const int* faces, int nv, int nf, float* face_normals, void* stream) {
    return rcmvs_mn_face_normals_timed(verts, faces, nv, nf, face_normals, RCMVS_MN_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mn_vertex_normals_timed(const float* verts, const int* faces, int nv, int nf, int weight, unsigned* key_a, int* idx_a, unsigned* key_b,
                                             int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, float* normals, u64* stats, int phase, void* ev0,
                                             void* ev1, void* stream) {
    if (int rc = mn_sizes("mn_vertex_normals", nv, nf)) return rc;
    RCMVS_REQUIRE(weight == RCMVS_MN_WEIGHT_AREA || weight == RCMVS_MN_WEIGHT_SPHERE, "mn_vertex_normals: weight = %d (0: area, 1: sphere)", weight);
    RCMVS_REQUIRE(phase >= RCMVS_MN_PHASE_ALL && phase <= RCMVS_MN_PHASE_ACCUMULATE, "mn_vertex_normals: phase = %d (0 .. 2)", phase);
    RCMVS_REQUIRE(stats, "mn_vertex_normals: null pointer (stats)");
    RCMVS_REQUIRE(nv == 0 || (verts && seg && normals), "mn_vertex_normals: null pointer (verts, seg and normals hold nv rows)");
    RCMVS_REQUIRE(nf == 0 || (faces && key_a && idx_a && key_b && idx_b && hist && hist_start),
                  "mn_vertex_normals: null pointer (faces, key_a, idx_a, key_b, idx_b, hist and hist_start serve 3 nf corners)");
    RCMVS_REQUIRE(scan_work, "mn_vertex_normals: null pointer (scan_work)");
    if (int rc = scan_work_check("mn_vertex_normals", scan_work)) return rc;
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "mn_vertex_normals: stats must be 8-byte aligned");
    const long long n = 3ll * nf, table = 256 * cdiv(n, MN_BLOCK);
    {
        const void* ptr[] = {key_a, idx_a, key_b, idx_b, hist, hist_start, seg, normals, stats, verts, faces};
        const size_t len[] = {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)table * 4, (size_t)(table + 1) * 4, (size_t)nv * 8,
                              (size_t)nv * 12, (size_t)RCMVS_MN_STATS * 8, (size_t)nv * 12, (size_t)nf * 12};
        if (int rc = buffers_overlap("mn_vertex_normals", ptr, len, 9, 11)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    const bool all = phase == RCMVS_MN_PHASE_ALL, inc = phase == RCMVS_MN_PHASE_INCIDENCE, acc = phase == RCMVS_MN_PHASE_ACCUMULATE;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(MN_BLOCK), 0, st, (all || inc) ? e0 : none, none, stats, (long long)RCMVS_MN_STATS);
    hipLaunchKernelGGL(zero_kernel<int>, dim3(blocks(2ll * nv)), dim3(MN_BLOCK), 0, st, seg, 2ll * nv);
    hipLaunchKernelGGL(mn_key_kernel, dim3(blocks(nf)), dim3(MN_BLOCK), 0, st, verts, faces, nv, nf, key_a, idx_a, stats);
    radix_sort<unsigned>(&key_a, &idx_a, &key_b, &idx_b, n, radix_passes((u64)nv), hist, hist_start, scan_work, st);      // the sentinel nv is the largest key
    RCMVS_LAUNCH_TIMED(segments_kernel, dim3(blocks(n)), dim3(MN_BLOCK), 0, st, none, inc ? e1 : none, key_a, n, nv, seg);
    RCMVS_LAUNCH_TIMED(mn_accumulate_kernel, dim3(blocks(nv)), dim3(MN_BLOCK), 0, st, acc ? e0 : none, (all || acc) ? e1 : none, verts, faces, nv, n, weight,
                       idx_a, seg, normals, stats);
    return launch_status("mn_vertex_normals");
}

extern "C" int rcmvs_mn_vertex_normals(const float* verts, const int* faces, int nv, int nf, int weight, unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b,
                                       int* hist, int* hist_start, int* scan_work, int* seg, float* normals, u64* stats, void* stream) {
    return rcmvs_mn_vertex_normals_timed(verts, faces, nv, nf, weight, key_a, idx_a, key_b, idx_b, hist, hist_start, scan_work, seg, normals, stats,
                                         RCMVS_MN_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_mn_shade_timed(const float* verts, const int* faces, const float* normals, int nv, int nf, int n, int H, int W, const double* cams_host,
                                    double near_z, const int* face_image, int background, float* normal_map, unsigned char* smooth, unsigned char* normal_rgb,
                                    int phase, void* ev0, void* ev1, void* stream) {
    if (int rc = mn_sizes("mn_shade", nv, nf)) return rc;
    RCMVS_REQUIRE(n >= 1, "mn_shade: n = %d views (at least 1)", n);
    RCMVS_REQUIRE(H >= 1 && H <= mr::MAX_SIDE, "mn_shade: H = %d (1 .. %d)", H, mr::MAX_SIDE);
    RCMVS_REQUIRE(W >= 1 && W <= mr::MAX_SIDE, "mn_shade: W = %d (1 .. %d)", W, mr::MAX_SIDE);
    RCMVS_REQUIRE(near_z > 0.0 && near_z <= 1.7976931348623157e308, "mn_shade: near_z = %g (finite and > 0)", near_z);
    RCMVS_REQUIRE(background >= 0 && background <= 0xffffff, "mn_shade: background = %d (r | g << 8 | b << 16)", background);
    RCMVS_REQUIRE(phase == RCMVS_MN_PHASE_ALL, "mn_shade: phase = %d (0: all)", phase);
    RCMVS_REQUIRE(cams_host && face_image && normal_map && smooth && normal_rgb, "mn_shade: null pointer (cams_host, face_image, normal_map, smooth, normal_rgb)");
    RCMVS_REQUIRE(nv == 0 || (verts && normals), "mn_shade: null pointer (verts and normals hold nv rows)");
    RCMVS_REQUIRE(nf == 0 || faces, "mn_shade: null pointer (faces)");
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(normal_map) & 3) == 0 && (reinterpret_cast<uintptr_t>(face_image) & 3) == 0,
                  "mn_shade: normal_map and face_image must be 4-byte aligned");
    const size_t pixels = (size_t)H * (size_t)W, all = pixels * (size_t)n;
    {
        const void* ptr[] = {normal_map, smooth, normal_rgb, verts, faces, normals, face_image};
        const size_t len[] = {all * 12, all, all * 3, (size_t)nv * 12, (size_t)nf * 12, (size_t)nv * 12, all * 4};
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 7; ++j)
                RCMVS_REQUIRE(!ranges_overlap(ptr[i], len[i], ptr[j], len[j]), "mn_shade: an output overlaps another buffer");
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    for (int v = 0; v < n; ++v) {
        mr::Cam cam;
        for (int k = 0; k < 16; ++k) cam.c[k] = cams_host[16 * (size_t)v + k];
        RCMVS_LAUNCH_TIMED(mn_shade_kernel, dim3(blocks((long long)pixels)), dim3(MN_BLOCK), 0, st, v == 0 ? e0 : none, v == n - 1 ? e1 : none, verts, faces, normals,
                           nv, nf, cam, near_z, H, W, face_image + (size_t)v * pixels, background, normal_map + (size_t)v * pixels * 3, smooth + (size_t)v * pixels,
                           normal_rgb + (size_t)v * pixels * 3);
    }
    return launch_status("mn_shade");
}

extern "C" int rcmvs_mn_shade(const float* verts, const int* faces, const float* normals, int nv, int nf, int n, int H, int W, const double* cams_host,
                              double near_z, const int* face_image, int background, float* normal_map, unsigned char* smooth, unsigned char* normal_rgb,
                              void* stream) {
    return rcmvs_mn_shade_timed(verts, faces, normals, nv, nf, n, H, W, cams_host, near_z, face_image, background, normal_map, smooth, normal_rgb,
                                RCMVS_MN_PHASE_ALL, nullptr, nullptr, stream);
}
