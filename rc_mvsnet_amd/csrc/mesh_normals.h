/* C ABI of the mesh normals in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_render.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, a *_timed twin whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_NORMALS_H
#define RCMVS_MESH_NORMALS_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> face normals, oriented vertex normals, and normal maps of rendered views (rc_mvsnet_amd/mesh_normals.py;
 * csrc/mesh_normals.hip; the per-element rules are csrc/mesh_normals_math.h's, restated by tests/mesh_normals_oracle.py) ----
 * A mesh is verts (nv, 3) fp32 and faces (nf, 3) int32, both DEVICE; 0 <= nv < 2^31, 0 <= 3 nf <= RCMVS_MN_MAX_CORNERS (a corner
 * number 3 face + corner is an int), and a pointer to an array of no elements may be NULL.  Validity of a face is mesh_clean.h's
 * (three indices in [0, nv) that differ); every kernel tests it before an index is used as an address.
 *
 * THE RULE (mesh_normals_math.h states every expression; fp64, one rounding per operation).  For a valid face (a, b, c): u = b - a,
 * v = c - a (one fp64 subtraction of the fp32 coordinates per component), F = u x v (one product minus another per component).  A
 * face with a non-finite coordinate is SKIPPED and counted as non-finite; F = (0, 0, 0) is counted as degenerate.  The face normal
 * is (float)(F_k / sqrt((Fx Fx + Fy Fy) + Fz Fz)), (0, 0, 0) for an invalid, skipped or degenerate face and for a squared length
 * that is not finite and > 0.
 * A vertex sums the contributions of its corners in fp64, one by one from (0, 0, 0) in ascending order of 3 face + corner, over
 * the valid faces that are not skipped.  weight = RCMVS_MN_WEIGHT_AREA: the face's F, the same bits at its three corners.
 * weight = RCMVS_MN_WEIGHT_SPHERE (Max's weights): at corner p with next vertex q and previous vertex r, e1 = q - p, e2 = r - p,
 * C = e1 x e2, l1 = e1 . e1, l2 = e2 . e2 (each (x x + y y) + z z), the contribution C_k / (l1 l2); a corner with l1 l2 not > 0 is
 * skipped and counted.  N = (float)(S_k / sqrt((Sx Sx + Sy Sy) + Sz Sz)); (0, 0, 0) when the vertex has no contributing corner
 * (counted as unreferenced) or when the squared length is not finite and > 0 (counted as cancelled: two sheets glued with opposite
 * orientation do this).  The extracted meshes are oriented from the inside to the outside (mesh_render_math.h), so N points out.
 *
 * THE PASSES of rcmvs_mn_vertex_normals on the one stream.  Incidence: one thread per face writes the keys of its three corners
 * (the vertex, or the sentinel nv for an invalid or skipped face) and counts the face; the 3 nf (key, corner) pairs are sorted by
 * stable 8-bit radix passes (scan_sort.hip's), only as many as nv needs, so that a vertex's corners are consecutive and ascending;
 * a thread per sorted pair marks where a vertex's segment starts and ends.  Accumulation: one lane per vertex walks its segment
 * (the fixed order forbids a tree).  No floating-point atomic, no kernel waits for another workgroup; counters are integer adds.
 * key_a, key_b: DEVICE 3 nf uint32 each; idx_a, idx_b: DEVICE 3 nf ints each; hist: DEVICE 256 ceil(3 nf / 256) ints; hist_start:
 * one more; scan_work: a work area of mesh_clean.h's scan for max(256 ceil(3 nf / 256), 3 nf) elements; seg: DEVICE 2 nv ints.
 * normals: DEVICE (nv, 3) fp32.  stats: DEVICE RCMVS_MN_STATS uint64 = {faces invalid, non-finite, degenerate, corners skipped
 * (SPHERE only), vertices with a normal, unreferenced, cancelled, 0}.  No output or work buffer may overlap another or an input.
 * The _timed twin brackets every launch (RCMVS_MN_PHASE_ALL), the incidence or the accumulation. */
#define RCMVS_MN_STATS 8
#define RCMVS_MN_MAX_CORNERS 2147483392
#define RCMVS_MN_SORT_BLOCK 256
#define RCMVS_MN_WEIGHT_AREA 0
#define RCMVS_MN_WEIGHT_SPHERE 1
#define RCMVS_MN_PHASE_ALL 0
#define RCMVS_MN_PHASE_INCIDENCE 1
#define RCMVS_MN_PHASE_ACCUMULATE 2

/* face_normals: DEVICE (nf, 3) fp32; one thread per face.  The twin's phase must be RCMVS_MN_PHASE_ALL. */
int rcmvs_mn_face_normals(const float* verts, const int* faces, int nv, int nf, float* face_normals, void* stream);
int rcmvs_mn_face_normals_timed(const float* verts, const int* faces, int nv, int nf, float* face_normals, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_mn_vertex_normals(const float* verts, const int* faces, int nv, int nf, int weight, unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b,
                            int* hist, int* hist_start, int* scan_work, int* seg, float* normals, unsigned long long* stats, void* stream);
int rcmvs_mn_vertex_normals_timed(const float* verts, const int* faces, int nv, int nf, int weight, unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b,
                                  int* hist, int* hist_start, int* scan_work, int* seg, float* normals, unsigned long long* stats, int phase, void* ev0,
                                  void* ev1, void* stream);

/* The normal pass over what rcmvs_mr_render produced, one thread per pixel.  normals: DEVICE (nv, 3) fp32; n >= 1 views of H x W,
 * cams_host, near_z as in mesh_render.h; face_image: DEVICE (n, H, W) int32, the render's face numbers.  For a pixel whose face
 * number f is in [0, nf), whose face is valid, whose three vertices are usable in the view and whose area2 is not zero, the
 * vertices are projected and the weights of the pixel formed again by mesh_render_math.h's functions; q_i = (double)w_i iz_i,
 * m = (q0 Na + q1 Nb) + q2 Nc per component, g = R m in camera()'s order without the translation.  normal_map (n, H, W, 3) fp32 =
 * (float)(g_k / len); smooth (n, H, W) uint8 = floor(255 |gz| / len + 0.5); normal_rgb (n, H, W, 3) uint8 = floor(127.5 (e_k + 1.0)
 * + 0.5) clamped to a byte, e = (gx, -gy, -gz) / len: a surface that faces the camera is (128, 128, 255).  A squared length of g
 * that is not finite and > 0 gives a zero normal, smooth 0 and (128, 128, 128).  Every other pixel -- f < 0, f >= nf, an invalid
 * face, an unusable vertex, area2 == 0 -- gives a zero normal, smooth 0 and background (r | g << 8 | b << 16): the image is never
 * trusted as an address.  The twin's phase must be RCMVS_MN_PHASE_ALL. */
int rcmvs_mn_shade(const float* verts, const int* faces, const float* normals, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z,
                   const int* face_image, int background, float* normal_map, unsigned char* smooth, unsigned char* normal_rgb, void* stream);
int rcmvs_mn_shade_timed(const float* verts, const int* faces, const float* normals, int nv, int nf, int n, int H, int W, const double* cams_host,
                         double near_z, const int* face_image, int background, float* normal_map, unsigned char* smooth, unsigned char* normal_rgb,
                         int phase, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_NORMALS_H */
