/* C ABI of the point-cloud clean-up in librcmvs_hip.so (an extension header of include/rcmvs.h like fusion_dyn.h, whose conventions
 * it keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, a *_timed twin whose ev0 / ev1 receive
 * the first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_CLOUD_KNN_H
#define RCMVS_CLOUD_KNN_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused cloud -> k nearest neighbours, outlier flags, oriented normals (rc_mvsnet_amd/cloud_clean.py; csrc/cloud_knn.hip; the
 * per-element rules are csrc/cloud_knn_math.h's, restated by tests/cloud_clean_oracle.py) ----
 * A cloud is pts (n, 3) fp32 on the DEVICE, 0 <= n < 2^31; a pointer to an array of no elements may be NULL.  The searches run on
 * the uniform grid of rcmvs_pc_bbox / rcmvs_pc_grid_build (include/rcmvs.h): grid_host = {origin x, y, z, cell edge}, dims_host =
 * {gx, gy, gz}, cell_start (cells + 1 ints), sorted (n, 4) fp32 and sorted_idx (n ints) as the build left them.  The grid holds
 * FINITE points only (rcmvs_ck_finite and rcmvs_ck_compact come first), and no answer depends on its cell edge.
 * Every entry point refuses, with the argument named and before anything is written: n outside its range, a null, misaligned or
 * overlapping buffer, and what is listed with it.  The _timed twins take phase = RCMVS_CK_PHASE_ALL only (every family here is
 * one phase; the scans inside compact and stat are bracketed with it).
 *
 * k NEAREST: for every point its k nearest OTHER points, ordered by (d2, input index) ascending; d2 = ((dx dx + dy dy) + dz dz)
 * in fp64 from the fp32 coordinates (pc::dist2).  The point itself is excluded by its index; a duplicate at another index is a
 * neighbour with d2 = 0.  Slots that do not exist (n - 1 < k) hold index -1 and d2 = +inf.  1 <= k <= RCMVS_CK_MAX_K and
 * n k <= RCMVS_CK_MAX_NK.  Thread i takes the point in sorted slot i, so that a wave walks the same cells; each lane keeps its k
 * best as a sorted list in LDS laid out [slot][lane] (a register array indexed at run time would live in scratch memory), the
 * current worst in a register; cells are visited in shells around the point's cell until the lower bound of everything unvisited,
 * squared, exceeds the worst (pc_nn_kernel's walk and slack).  Outputs, each nullable, rows in INPUT numbering: idx (n, k) int32,
 * d2 (n, k) fp64, mean (n) fp64 = (sum of sqrt(d2_j) in slot order) / k, NaN where a slot is missing.  counters: NULL or 2 uint64
 * on the DEVICE that receive += the cells whose points were read and the candidates tested.
 *
 * RADIUS: count[i] = the other points with d2 <= r2, saturating at cap (the walk stops there); keep (n bytes, nullable): count[i] >=
 * cap.  r2 >= 0, +inf allowed, NaN and negative refused; cap >= 0.
 *
 * STATISTICAL: a point is valid when its mean is not NaN.  mu and sigma are rcmvs_pc_moments' mean and sqrt of the N - 1 variance
 * of the valid means in input order (its fixed summation tree: lane t of 65536 adds x[t], x[t + 65536], ...; a block halves its
 * 256 sums down; the 256 block sums are added in order), sigma = 0 for one valid point, both NaN for none.  keep[i] = valid and
 * mean[i] <= threshold(mu, sigma, ratio) (mu + ratio sigma; +inf for ratio = +inf).  ratio >= 0.  stats (DEVICE, 8 doubles) =
 * {valid points, mu, sigma, threshold, then rcmvs_pc_moments' own n, mean, variance, and 0}.  Work: flags n bytes, offsets n + 1 ints,
 * scan_work a work area of scan_sort.h's scan for n elements, valid_mean n doubles, part RCMVS_PC_MOMENT_BLOCKS doubles.
 *
 * NORMALS from idx (n, k): the covariance of the point and its existing neighbours (m = 1 + existing; an index outside [0, n) is
 * no neighbour), summed in slot order with the point first about their mean, in fp64; a cyclic Jacobi iteration over (0,1), (0,2),
 * (1,2), a rotation skipped when its entry is exactly 0, at most RCMVS_CK_MAX_SWEEPS sweeps; the eigenvector of the smallest
 * eigenvalue (ties to the lower column), normalised, its largest component (ties to the first) made positive.  (0, 0, 0) for
 * m < 3 and for lambda2 == 0 or lambda1 <= 1e-12 lambda2.  view (n int32) and centres (nc, 3) fp64 on the DEVICE, both or neither:
 * the normal is flipped when n . (c - p) < 0; a view outside [0, nc) leaves it.  normals (n, 3) fp32, one rounding per component.
 * counters: RCMVS_CK_COUNTERS int64 on the DEVICE = {with a normal, too few, degenerate, unconverged, unoriented, flipped,
 * oriented and kept, 0}.
 *
 * COMPACT: the rows of xyz, rgb (n, 3 uint8, nullable with out_rgb) and view (n int32, nullable with out_view) whose keep byte is
 * not 0, in input order; out_index[j] = the input index of survivor j; total (DEVICE, one uint64) = the survivors.  offsets
 * n + 1 ints and scan_work are work.  keep bytes must be 0 or 1. */
#define RCMVS_CK_MAX_K 32
#define RCMVS_CK_MAX_NK 2147483392
#define RCMVS_CK_MAX_SWEEPS 32
#define RCMVS_CK_COUNTERS 8
#define RCMVS_CK_PHASE_ALL 0

/* flags[i] = 1 where the three coordinates of point i are finite, else 0; *count (DEVICE int) = the finite points */
int rcmvs_ck_finite(const float* pts, long long n, unsigned char* flags, int* count, void* stream);
int rcmvs_ck_finite_timed(const float* pts, long long n, unsigned char* flags, int* count, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_ck_knn(long long n, int k, const double* grid_host, const int* dims_host, const int* cell_start, const float* sorted,
                 const int* sorted_idx, int* idx, double* d2, double* mean, unsigned long long* counters, void* stream);
int rcmvs_ck_knn_timed(long long n, int k, const double* grid_host, const int* dims_host, const int* cell_start, const float* sorted,
                       const int* sorted_idx, int* idx, double* d2, double* mean, unsigned long long* counters, int phase, void* ev0,
                       void* ev1, void* stream);

int rcmvs_ck_radius(long long n, double r2, int cap, const double* grid_host, const int* dims_host, const int* cell_start,
                    const float* sorted, const int* sorted_idx, int* count, unsigned char* keep, void* stream);
int rcmvs_ck_radius_timed(long long n, double r2, int cap, const double* grid_host, const int* dims_host, const int* cell_start,
                          const float* sorted, const int* sorted_idx, int* count, unsigned char* keep, int phase, void* ev0, void* ev1,
                          void* stream);

int rcmvs_ck_stat(const double* mean, long long n, double ratio, unsigned char* flags, int* offsets, int* scan_work, double* valid_mean,
                  double* part, double* stats, unsigned char* keep, void* stream);
int rcmvs_ck_stat_timed(const double* mean, long long n, double ratio, unsigned char* flags, int* offsets, int* scan_work,
                        double* valid_mean, double* part, double* stats, unsigned char* keep, int phase, void* ev0, void* ev1,
                        void* stream);

int rcmvs_ck_normals(const float* pts, long long n, int k, const int* idx, const int* view, const double* centres, int nc, float* normals,
                     long long* counters, void* stream);
int rcmvs_ck_normals_timed(const float* pts, long long n, int k, const int* idx, const int* view, const double* centres, int nc,
                           float* normals, long long* counters, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_ck_compact(const unsigned char* keep, const float* xyz, const unsigned char* rgb, const int* view, long long n, int* offsets,
                     int* scan_work, float* out_xyz, unsigned char* out_rgb, int* out_view, int* out_index, unsigned long long* total,
                     void* stream);
int rcmvs_ck_compact_timed(const unsigned char* keep, const float* xyz, const unsigned char* rgb, const int* view, long long n,
                           int* offsets, int* scan_work, float* out_xyz, unsigned char* out_rgb, int* out_view, int* out_index,
                           unsigned long long* total, int phase, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_CLOUD_KNN_H */
