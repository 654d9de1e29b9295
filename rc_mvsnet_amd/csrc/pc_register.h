/* C ABI of the Tanks and Temples F-score kernels in librcmvs_hip.so (an extension header of include/rcmvs.h: same conventions --
 * status-returning entry points, rcmvs_last_error_string for the message, HOST arrays named *_host, a HIP stream as void*). */
#ifndef RCMVS_PC_REGISTER_H
#define RCMVS_PC_REGISTER_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py; csrc/pc_register.hip; additive, RCMVS_VERSION stays 106) ----
 * This family's C ABI is declared here, next to its kernels, and not in include/rcmvs.h: rc_mvsnet_amd/_lib.py parses this file
 * into its EXT_SIGNATURES table the same way it parses the primary header, and a caller checks for the entry points by symbol.
 * The benchmark's python_toolbox/evaluation (crop to a polygon prism, voxel down-sample, ICP refinement, thresholded distance
 * histograms) on the DTU scorer's bounding box, grid and capped nearest neighbour.  Point clouds are (n,3) fp32, n below 2^31.
 * A transform is 16 HOST doubles, a row-major 4x4 whose last row is taken as (0, 0, 0, 1) and not read; it is applied in fp64
 * as ((T0 x + T1 y) + T2 z) + T3 per row (csrc/pc_register_math.h).  Sums are fp64 over a fixed tree: two runs give the same bits. */
#define RCMVS_PC_MAX_POLYGON 128                  /* vertices of a crop polygon (it travels as a kernel argument) */
#define RCMVS_PC_MAX_VOXELS_PER_AXIS (1 << 21)    /* three of them pack into a 63-bit key */
#define RCMVS_PC_ICP_BLOCKS 2048                  /* block partials of one ICP step */
#define RCMVS_PC_ICP_MOMENTS 18
#define RCMVS_PC_HIST_MAX_BINS 4096
/* Open3D's SelectionPolygonVolume.  q = transform_host applied to pts[i] and rounded to fp32 once (NULL: q = pts[i], no
 * arithmetic).  flags[i] (u8) = axis_min <= q[axis] <= axis_max and (u, v) = q's two other coordinates, in axis order, inside the
 * polygon by the even-odd rule: over the edges (i, j = i - 1 mod m) with (v_i < v && v_j >= v) || (v_j < v && v_i >= v), an odd
 * number of crossings u_i + (v - v_i) / (v_j - v_i) * (u_j - u_i) < u (fp64).  polygon_host: m (u, v) pairs of doubles,
 * 3 <= m <= RCMVS_PC_MAX_POLYGON.  kept (n,3) receives the flagged q in input order.
 * work: 2 ceil(n / 256) + 1 + ceil(ceil(n / 256) / 2048) + 1 ints; the kept count lands in work[2 ceil(n / 256)]. */
int rcmvs_pc_crop(const float* pts, long long n, const double* transform_host, int axis, double axis_min, double axis_max,
                  const double* polygon_host, int m, unsigned char* flags, float* kept, int* work, void* stream);
/* Voxel-average down-sample in two steps, the host reading the voxel count in between.  lattice_host = {origin x, y, z, voxel}
 * (doubles; origin = the cloud's minimum - voxel / 2), dims_host = {gx, gy, gz} (int64, each 1 .. RCMVS_PC_MAX_VOXELS_PER_AXIS);
 * the voxel of a point is k = floor((p - origin) / voxel) per axis in fp64, its key (kz gy + ky) gx + kx.
 * sort: (key, index) pairs sorted by an LSD radix sort, 8 bits a pass (an even number of passes: the result is in key_a / idx_a,
 *       key_b / idx_b are work; all four hold n entries, keys uint64).  With b = ceil(n / 256): hist (256 b) and hist_start
 *       (256 b + 1) ints, scan_work (ceil(max(256 b, n) / 2048) + 1) ints, head (n) ints; head_start (n + 1) receives the output
 *       slot of every sorted entry and head_start[n] = the number of occupied voxels m.  n <= 2^31 - 256.
 * emit: out (m,3) = per voxel, in ascending key order, the mean of its points: added in fp64 in input-index order, divided once,
 *       rounded to fp32 once.  No array over the lattice, no floating-point atomics. */
int rcmvs_pc_voxel_sort(const float* pts, long long n, const double* lattice_host, const long long* dims_host,
                        unsigned long long* key_a, int* idx_a, unsigned long long* key_b, int* idx_b, int* hist, int* hist_start,
                        int* scan_work, int* head, int* head_start, void* stream);
int rcmvs_pc_voxel_emit(const float* pts, long long n, const unsigned long long* key, const int* idx, const int* head_start,
                        long long m, float* out, void* stream);
/* One ICP evaluation in one search launch (plus the finish of the partials).  For every src[i]: s' = transform_host applied in
 * fp64 (not rounded), t = its nearest of the n_to points of a rcmvs_pc_grid_build grid (cell_start, sorted, sorted_idx) by
 * rcmvs_pc_nearest's shell search stopped at max_dist, equidistant targets resolved to the lower input index; the pair counts
 * when |s' - t| < max_dist.  out[RCMVS_PC_ICP_MOMENTS] (DEVICE doubles) = {count, sum d^2, sum s' (3), sum t (3), sum s'_a t_b
 * (9, a-major), sum |s'|^2} over the pairs.  corr = NULL or (n) ints: the target's input index, -1 for none.
 * part: RCMVS_PC_ICP_MOMENTS * RCMVS_PC_ICP_BLOCKS doubles of work. */
int rcmvs_pc_icp_step(const float* src, long long n, const double* transform_host, const double* grid_host, const int* dims_host,
                      const int* cell_start, const float* sorted, const int* sorted_idx, long long n_to, double max_dist, int* corr,
                      double* part, double* out, void* stream);
/* counts (nbins) uint64: counts[b] = the d[i] (doubles) with floor(d[i] / w) == b (fp64; others dropped), *below (uint64) = the
 * d[i] < tau.  Both are zeroed by the call; exact integers (LDS counts per block, then integer atomics).
 * 1 <= nbins <= RCMVS_PC_HIST_MAX_BINS. */
int rcmvs_pc_dist_hist(const double* d, long long n, double tau, int nbins, double w, unsigned long long* counts,
                       unsigned long long* below, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_PC_REGISTER_H */
