/* C ABI of the Poisson surface reconstruction in librcmvs_hip.so (an extension header of include/rcmvs.h like cloud_knn.h, whose
 * conventions it keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, a *_timed twin whose ev0 / ev1
 * receive the start of the first launch and the stop of the last launch of the chosen phase; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_POISSON_H
#define RCMVS_POISSON_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- oriented cloud -> indicator field on a dense grid (rc_mvsnet_amd/poisson_mesh.py; csrc/poisson.hip; the per-element rules are
 * csrc/poisson_math.h's, restated by tests/poisson_oracle.py) ----
 * Unscreened Poisson reconstruction (Kazhdan, Bolitho, Hoppe 2006) on a uniform grid, solved by geometric multigrid.  The grid is
 * tsdf_mesh.h's: grid_host = {ox, oy, oz, h} (HOST, 4 doubles), dims_host = {gx, gy, gz} (HOST, 3 ints), voxel (i, j, k) has the
 * number i + gx (j + gy k) and its centre at o + (idx + 0.5) h, so rcmvs_tsdf_mesh_count / _emit read the field unchanged.  Every
 * side >= 1, gx gy gz <= RCMVS_PO_MAX_VOXELS; h and the origin finite, h > 0.  A cloud is xyz (n, 3) fp32, normals (n, 3) fp32 and
 * optionally rgb (n, 3) bytes on the DEVICE, 0 <= n < 2^31; a pointer to an array of no elements may be NULL.  Planes are fp32 on
 * the DEVICE, one value per voxel.  All arithmetic is fp64 without contraction, one rounding per stored value.
 * Every entry point refuses, with the argument named and before anything is written: a size outside its range, a null, misaligned
 * or overlapping buffer, and what is listed with it.
 *
 * SPLAT.  A point is skipped and counted when a coordinate or a normal component is not finite (NON_FINITE), else when its normal
 * has squared length 0 (ZERO_NORMAL), else when the eight voxels around it are not all in the grid (OUTSIDE): u = (p - o) / h - 0.5,
 * 0 <= floor(u) <= g - 2 per axis.  A splatted point has the weights (wx wy) wz on its eight corners (code dx + 2 dy + 4 dz).
 * Accumulation is FIXED POINT in acc (RCMVS_PO_ACC planes of voxels int64 with rgb, the first 4 without; zeroed by the call): 64-bit integer atomic adds, whose
 * sums do not depend on the order, so two runs give the same bits with no sort.  There are no floating-point atomics.
 *   plane 0       += llrint(w 2^28)                         W = (float)(acc 2^-28)
 *   W_p            = sum over the corners in code order of w (double)W, from 0.0, in fp64; s = 1 / W_p (density_weight) or 1
 *   planes 1..3   += llrint(((s w) n_c) 2^28), n = the normal / sqrt(its squared length)      V = (float)(acc 2^-28)
 *   planes 4..6   += llrint((w byte) 2^20) when rgb is given      C = (float)((acc 2^-20) / (acc0 2^-28)), 128 where acc0 == 0
 * Overflow: a point's own weights give W_p >= sum w^2 >= 1/8 (eight weights that sum to 1), so s <= 8 up to the rounding of W, a
 * point adds at most 8 2^28 = 2^31 to a voxel's plane and 2^31 points stay below 2^62; the density adds at most 2^28 and a colour
 * at most 255 2^20 < 2^28 per point.
 * Outputs: W, V (3 planes), C (3 planes: all three with rgb, else NULL), point (n, 2) doubles = {s, W_p} per point, {0, 0} for a
 * skipped one, counters (RCMVS_PO_COUNTERS int64) = {splatted, non-finite, zero normal, outside, 0, 0, 0, 0}.
 *
 * RHS.  b = ((Vx[i+1] - Vx[i-1]) + (Vy[j+1] - Vy[j-1]) + (Vz[k+1] - Vz[k-1])) / (2 h), V = 0 outside the grid.
 *
 * SOLVE.  cycles V(2, 2) cycles on Laplace chi = b, chi = 0 on the faces of the box: the wall lies between the outermost cell and
 * a ghost cell that holds MINUS the inner value, in the operator, the smoother and the prolongation alike.  Level l has the sides
 * g >> l and the edge h 2^l; a level is coarsened while all its sides are even and the smallest coarser side is >= 4; at most
 * RCMVS_PO_MAX_LEVELS levels.  Smoother: x' = (1 - w) x + w (S - h^2 b) / 6, w = 6/7, S the neighbours added in the order -x +x -y
 * +y -z +z; two planes are ping-ponged, never updated in place.  The residual b - (S - 6 x) / h^2 of the eight children (code
 * order) is averaged into the coarse b in the kernel that computes it.  The coarse x starts at 0.  The coarsest level takes
 * RCMVS_PO_COARSEST_SWEEPS sweeps.  Prolongation: per axis 3/4 of the parent + 1/4 of the neighbour on the fine cell's side (x, then
 * y, then z), added to the fine x in the same kernel.  x is in and out: cycles calls of one cycle equal one call.  tmp: voxels
 * floats.  coarse: 3 (the voxels of all coarser levels) floats, level l >= 1 as {x, tmp, b} after the levels before it.
 * resid (cycles doubles, NULL for 0 cycles) receives max |b - Laplace x| on the fine grid after every cycle; part:
 * RCMVS_PO_PART doubles of work.  0 <= cycles <= RCMVS_PO_MAX_CYCLES.  Nothing is read back by the host.
 * Phases of the _timed twin: ALL, or the first fine-level launch of a SWEEP, a RESTRICT (residual + restriction) or a PROLONG.
 *
 * ISO.  Per point in input order the terms {s chi(p), s, W_p, 1} (chi(p) interpolated like W_p; zeros for a skipped point, s == 0),
 * written to terms (4 planes of n doubles) and summed by rcmvs_pc_moments' fixed tree (lane t of 65536 adds x[t], x[t + 65536], ...;
 * a block halves its 256 sums down; the 256 block sums are added in order).  stats (DEVICE, RCMVS_PO_STATS doubles) = {iso =
 * sum s chi / sum s (0 when nothing was splatted), sum s chi, sum s, sum W_p, splatted, mean W_p (0 for none), min W_p (+inf for
 * none), 0}.  part: 5 RCMVS_PC_MOMENT_BLOCKS doubles of work.
 *
 * FIELD.  dsum = (float)(chi - iso), iso read from stats on the device; wsum = 1 where D >= trim, else 0, D the maximum of W over
 * the voxel's 3 x 3 x 3 neighbourhood inside the grid (a tetrahedron needs its four corners observed and they lie up to sqrt(3) h
 * from the surface: an undilated mask tears the surface).  trim finite and >= 0.  trimmed (DEVICE, one int64) = voxels with wsum 0. */
#define RCMVS_PO_MAX_VOXELS (1 << 27)
#define RCMVS_PO_MAX_LEVELS 16
#define RCMVS_PO_MAX_CYCLES 64
#define RCMVS_PO_COARSEST_SWEEPS 64
#define RCMVS_PO_ACC 7
#define RCMVS_PO_COUNTERS 8
#define RCMVS_PO_STATS 8
#define RCMVS_PO_PART 1024
#define RCMVS_PO_PHASE_ALL 0
#define RCMVS_PO_PHASE_DENSITY 1
#define RCMVS_PO_PHASE_NORMAL 2
#define RCMVS_PO_PHASE_SWEEP 1
#define RCMVS_PO_PHASE_RESTRICT 2
#define RCMVS_PO_PHASE_PROLONG 3

int rcmvs_po_splat(const float* xyz, const float* normals, const unsigned char* rgb, long long n, int density_weight,
                   const double* grid_host, const int* dims_host, long long* acc, float* W, float* Vx, float* Vy, float* Vz, float* Cr,
                   float* Cg, float* Cb, double* point, long long* counters, void* stream);
int rcmvs_po_splat_timed(const float* xyz, const float* normals, const unsigned char* rgb, long long n, int density_weight,
                         const double* grid_host, const int* dims_host, long long* acc, float* W, float* Vx, float* Vy, float* Vz,
                         float* Cr, float* Cg, float* Cb, double* point, long long* counters, int phase, void* ev0, void* ev1,
                         void* stream);

int rcmvs_po_rhs(const float* Vx, const float* Vy, const float* Vz, const double* grid_host, const int* dims_host, float* b, void* stream);
int rcmvs_po_rhs_timed(const float* Vx, const float* Vy, const float* Vz, const double* grid_host, const int* dims_host, float* b,
                       int phase, void* ev0, void* ev1, void* stream);

int rcmvs_po_solve(float* x, float* tmp, const float* b, float* coarse, const double* grid_host, const int* dims_host, int cycles,
                   double* part, double* resid, void* stream);
int rcmvs_po_solve_timed(float* x, float* tmp, const float* b, float* coarse, const double* grid_host, const int* dims_host, int cycles,
                         double* part, double* resid, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_po_iso(const float* xyz, const double* point, long long n, const float* chi, const double* grid_host, const int* dims_host,
                 double* terms, double* part, double* stats, void* stream);
int rcmvs_po_iso_timed(const float* xyz, const double* point, long long n, const float* chi, const double* grid_host,
                       const int* dims_host, double* terms, double* part, double* stats, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_po_field(const float* chi, const float* W, const double* stats, double trim, const int* dims_host, float* dsum, float* wsum,
                   long long* trimmed, void* stream);
int rcmvs_po_field_timed(const float* chi, const float* W, const double* stats, double trim, const int* dims_host, float* dsum,
                         float* wsum, long long* trimmed, int phase, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_POISSON_H */
