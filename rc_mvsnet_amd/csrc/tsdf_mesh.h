/* C ABI of the TSDF fusion and marching-tetrahedra kernels in librcmvs_hip.so (an extension header of include/rcmvs.h: same
 * conventions -- status-returning entry points, rcmvs_last_error_string for the message, a HIP stream as void*). */
#ifndef RCMVS_TSDF_MESH_H
#define RCMVS_TSDF_MESH_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- depth maps -> triangle mesh (rc_mvsnet_amd/tsdf_mesh.py; csrc/tsdf_mesh.hip; additive, RCMVS_VERSION stays 106) ----
 * Declared next to its kernels like csrc/undistort.h; rc_mvsnet_amd/_lib.py parses this file into EXT_SIGNATURES.
 * The volume: grid_host = {ox, oy, oz, h} (HOST, 4 doubles), dims_host = {gx, gy, gz} (HOST, 3 ints), gx * gy * gz <=
 * RCMVS_TSDF_MAX_VOXELS, voxel (i, j, k) has the number i + gx * (j + gy * k) and the centre o + (idx + 0.5) * h.  The state is
 * planar fp32 on the DEVICE, every plane with its own base pointer and zero-filled by the caller: dsum (sum of truncated signed
 * distances / trunc), wsum (number of views that saw the voxel), and optionally three colour sums (all three or none).
 * All arithmetic is fp64 without contraction in the order csrc/tsdf_mesh_math.h writes; tests/tsdf_oracle.py restates it. */
#define RCMVS_TSDF_MAX_VOXELS (1 << 28)
#define RCMVS_TSDF_MAX_VIEWS 16
#define RCMVS_TSDF_SCAN_TILE 2048

/* Adds n views (1 .. RCMVS_TSDF_MAX_VIEWS) to the state in ONE launch: a thread reads its voxel's state once, goes through the
 * views in order with the state in registers and writes it once.  depth: DEVICE (n, H, W) fp32.  rgb: DEVICE (n, H, W, 3) bytes
 * or NULL (then the colour planes, if given, stay as they are).  cams_host: HOST, n x 16 doubles {R row-major 9, t 3, fx, fy, cx,
 * cy}, world -> camera; pixel centres at integers.  Per voxel and view: the centre in the camera frame, zc > 0, the pixel
 * floor(u + 0.5), floor(v + 0.5) inside the image (tested in fp64, so NaN and +-inf are outside), its depth d finite and > 0,
 * sdf = d - zc >= -trunc, then dsum += (float)min(1, sdf / trunc), wsum += 1, colour sums += the pixel's bytes.  One fp32 add per
 * view in view order: splitting the views over several calls gives the same bits.  No atomics; no input makes the kernel read
 * outside depth or rgb.  H, W >= 1, H * W < 2^31; h, trunc and the focal lengths finite and positive, everything else finite. */
int rcmvs_tsdf_integrate(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                         const double* grid_host, const int* dims_host, float* dsum, float* wsum, float* csum_r, float* csum_g,
                         float* csum_b, void* stream);
int rcmvs_tsdf_integrate_timed(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                               const double* grid_host, const int* dims_host, float* dsum, float* wsum, float* csum_r, float* csum_g,
                               float* csum_b, void* ev0, void* ev1, void* stream);

/* Marching tetrahedra, step 1.  A voxel's value is (double)dsum / (double)wsum; it is observed when wsum >= min_weight (>= 1) and
 * inside when its value is < 0 (exactly 0 is outside).  Cube (i, j, k) has its corners at the voxel centres i..i+1, j..j+1, k..k+1
 * (corner code dx + 2 dy + 4 dz) and is cut into the six tetrahedra (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).
 * A grid edge belongs to its lower voxel (7 edges per voxel, to the neighbours at codes 1..7) and carries a vertex when both ends
 * are observed and exactly one is inside; a tetrahedron emits triangles when its four corners are observed.
 * Writes per voxel edge_mask (bit code-1 set = that edge has a vertex) and tri_count (triangles of the cube at this voxel), both
 * DEVICE bytes, their exclusive scans vert_start and tri_start (DEVICE, voxels + 1 ints each) and totals = {vertices, triangles}
 * (DEVICE, 2 uint64, exact even when a total does not fit the ints: the caller refuses totals >= 2^31 before it allocates).
 * scan_work: DEVICE, 256 + 2 * ceil(voxels / RCMVS_TSDF_SCAN_TILE) ints, 8-byte aligned (a three-level scan: tiles of
 * RCMVS_TSDF_SCAN_TILE voxels, tiles of RCMVS_TSDF_SCAN_TILE tile sums, at most 64 sums of those in 64 bits). */
int rcmvs_tsdf_mesh_count(const float* dsum, const float* wsum, const int* dims_host, int min_weight, unsigned char* edge_mask,
                          unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                          void* stream);
int rcmvs_tsdf_mesh_count_timed(const float* dsum, const float* wsum, const int* dims_host, int min_weight, unsigned char* edge_mask,
                                unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                                void* ev0, void* ev1, void* stream);

/* Step 2, after the caller has read totals.  verts (nv, 3) fp32 ordered by (owner voxel, edge code): from the lower voxel a to
 * the higher b, t = da / (da - db), position pa + t * (pb - pa) per axis in fp64 rounded to fp32 once.  vert_rgb (nv, 3) bytes or
 * NULL (needs the three colour planes): per channel ca + t * (cb - ca) with c = csum / wsum, floor(. + 0.5) clamped to a byte.
 * faces (nf, 3) int32 ordered by (cube, tetrahedron, triangle), every normal (v1 - v0) x (v2 - v0) pointing from negative to
 * positive values; a face finds a vertex as vert_start[owner] + popcount(edge_mask[owner] & lower bits).  nv, nf: the totals
 * (< 2^31); nothing is written at or beyond them.  verts may be NULL when nv is 0, faces when nf is 0. */
int rcmvs_tsdf_mesh_emit(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                         const double* grid_host, const int* dims_host, int min_weight, const unsigned char* edge_mask,
                         const unsigned char* tri_count, const int* vert_start, const int* tri_start, long long nv, long long nf,
                         float* verts, unsigned char* vert_rgb, int* faces, void* stream);
int rcmvs_tsdf_mesh_emit_timed(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                               const double* grid_host, const int* dims_host, int min_weight, const unsigned char* edge_mask,
                               const unsigned char* tri_count, const int* vert_start, const int* tri_start, long long nv, long long nf,
                               float* verts, unsigned char* vert_rgb, int* faces, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_TSDF_MESH_H */
