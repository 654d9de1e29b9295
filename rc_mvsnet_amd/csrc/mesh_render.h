/* C ABI of the mesh rasteriser in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_holes.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, a *_timed twin whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_RENDER_H
#define RCMVS_MESH_RENDER_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> depth, face number, colour and shade in the cameras of a scan (rc_mvsnet_amd/mesh_render.py;
 * csrc/mesh_render.hip; the per-element rules are csrc/mesh_render_math.h's, restated by tests/mesh_render_oracle.py) ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE; 0 <= nv, nf < 2^31, and a
 * pointer to an array of no elements may be NULL.  Validity of a face is mesh_clean.h's (three indices in [0, nv) that differ);
 * every kernel tests it before an index is used as an address.  n >= 1 views of one size H x W, 1 <= H, W <= RCMVS_MR_MAX_SIDE;
 * cams_host: HOST, n x 16 doubles {R row-major 9, t 3, fx, fy, cx, cy}, world -> camera, pixel centres at integers
 * (rcmvs_tsdf_integrate's layout); near_z finite and > 0; cull RCMVS_MR_CULL_NONE or RCMVS_MR_CULL_BACK.
 *
 * THE RULE (mesh_render_math.h states every expression).  A vertex's camera-frame position is formed in fp64 in the order of
 * tsdf_mesh_math.h, u = fx (xc / zc) + cx, v likewise.  It is USABLE when zc is finite and >= near_z and u, v are finite with
 * |u|, |v| <= 2^16; then X = (int)floor(256 u + 0.5), Y likewise: a lattice of 1/256 pixel on which every edge function is an
 * integer below 2^53.  A valid face with an unusable vertex is skipped and counted as clipped (there is no near-plane clipping);
 * area2 = (Xb - Xa)(Yc - Ya) - (Xc - Xa)(Yb - Ya) == 0 is skipped as degenerate; area2 < 0 faces the camera and cull = back skips
 * area2 > 0.  The sample of pixel (px, py) is (256 px, 256 py); it is inside when the three int64 edge functions, negated for
 * area2 < 0, are > 0, or == 0 on a top or left edge.  depth = (float)((double)|area2| / ((w0 iz0 + w1 iz1) + w2 iz2)), iz = 1.0 / zc;
 * a depth that is not finite and > 0 drops the sample.  key = depth bits << 32 | face number, merged into keys by a 64-bit
 * integer atomicMin, the only atomic on an image: the nearest depth wins, among equal bits the smallest face number, whatever
 * the schedule.  Counters are integer adds.
 * Resolve, one thread per pixel: an untouched key gives depth 0, face -1, the background colour and shade 0; otherwise the
 * key's depth bits and face number, the perspective-correct colour floor(sum(w iz c) / sum(w iz) + 0.5) per channel (white
 * without rgb) and shade = floor(255 |nz| / |n| + 0.5) of the camera-frame face normal.
 *
 * THE PASSES, per view in view order on the one stream: project (one thread per vertex into proj_work), clear, small faces (one
 * lane per face walks a clamped bounding box of at most RCMVS_MR_SMALL_SIDE x RCMVS_MR_SMALL_SIDE pixels; a larger one is
 * appended to list_work by an integer atomicAdd), large faces (one workgroup per listed face, RCMVS_MR_LARGE_SLICES workgroups
 * for its samples; no output depends on the list's order), resolve.  Views are not batched in one grid: the work buffers are
 * one view's and are reused by the next.  Before the atomicMin a lane reads the key with a plain load and skips when its own is
 * not smaller: keys only decrease, so a stale read can cost an atomic and never changes the result.  No kernel waits for another
 * workgroup.
 * proj_work: DEVICE, 8-byte aligned, nv x RCMVS_MR_PROJ_BYTES bytes.  list_work: DEVICE, nf + 1 ints (the count first).
 * keys: DEVICE n x H x W uint64 (all ones where nothing was drawn).  depth (n, H, W) fp32, face (n, H, W) int32, out_rgb
 * (n, H, W, 3) uint8, shade (n, H, W) uint8.  stats: DEVICE n x RCMVS_MR_STATS uint64 = {faces drawn (valid, usable, not
 * degenerate, not culled), clipped, degenerate, culled, invalid, on the large path, pixels covered, 0}.  trace: NULL, or DEVICE
 * RCMVS_MR_TRACE uint64 that the call ADDS to = {samples inside a face, atomics issued, then the faces drawn by the longer side
 * of their clamped box: empty, 1, 2, 3..4, 5..8, 9..16, 17..64, above}; the first two depend on the schedule.
 * background: r | g << 8 | b << 16.  No output or work buffer may overlap another or an input.
 * The _timed twin brackets with ev0 / ev1 every launch of every view (RCMVS_MR_PHASE_ALL) or one phase of the LAST view: project,
 * small (clear and the small faces), large, resolve. */
#define RCMVS_MR_MAX_SIDE 16384
#define RCMVS_MR_SMALL_SIDE 8
#define RCMVS_MR_LARGE_SLICES 4
#define RCMVS_MR_PROJ_BYTES 24
#define RCMVS_MR_STATS 8
#define RCMVS_MR_TRACE 10
#define RCMVS_MR_CULL_NONE 0
#define RCMVS_MR_CULL_BACK 1
#define RCMVS_MR_PHASE_ALL 0
#define RCMVS_MR_PHASE_PROJECT 1
#define RCMVS_MR_PHASE_SMALL 2
#define RCMVS_MR_PHASE_LARGE 3
#define RCMVS_MR_PHASE_RESOLVE 4

int rcmvs_mr_render(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host,
                    double near_z, int cull, int background, void* proj_work, int* list_work, unsigned long long* keys, float* depth, int* face,
                    unsigned char* out_rgb, unsigned char* shade, unsigned long long* stats, unsigned long long* trace, void* stream);
int rcmvs_mr_render_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host,
                          double near_z, int cull, int background, void* proj_work, int* list_work, unsigned long long* keys, float* depth, int* face,
                          unsigned char* out_rgb, unsigned char* shade, unsigned long long* stats, unsigned long long* trace, int phase, void* ev0,
                          void* ev1, void* stream);

/* A rendered depth map against a depth map of the same view.  rendered, depth: DEVICE (n, H, W) fp32; a value that is 0, negative
 * or not finite means none; 1 <= n <= RCMVS_MR_CMP_MAX_VIEWS (a view is a row of the grid).  thresholds_host: HOST, 0 <= nt <= 3 finite doubles >= 0.  table: DEVICE n x RCMVS_MR_TABLE uint64 =
 * {pixels with both, with only the mesh, with only the map, with |r - d| <= t d for each threshold (fp64; 0 beyond nt), the BITS
 * of the fp64 sum of |r - d| over the pixels with both, 0}.  The sum has a fixed order: a workgroup sums RCMVS_MR_CMP_TILE
 * consecutive pixels (a thread its pixels t, t + 256, ... in order, then a tree over the threads) into partial_work, and one
 * workgroup per view sums the partials the same way; two runs are bit-identical.  partial_work: DEVICE, n x ceil(H W /
 * RCMVS_MR_CMP_TILE) doubles.  Nothing is read back by the host. */
#define RCMVS_MR_TABLE 8
#define RCMVS_MR_CMP_TILE 4096
#define RCMVS_MR_CMP_MAX_VIEWS 65535
int rcmvs_mr_compare(const float* rendered, const float* depth, int n, int H, int W, const double* thresholds_host, int nt, double* partial_work,
                     unsigned long long* table, void* stream);
int rcmvs_mr_compare_timed(const float* rendered, const float* depth, int n, int H, int W, const double* thresholds_host, int nt, double* partial_work,
                           unsigned long long* table, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_RENDER_H */
