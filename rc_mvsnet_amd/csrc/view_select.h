/* C ABI of the COLMAP-import kernels in librcmvs_hip.so (an extension header of include/rcmvs.h: same conventions --
 * status-returning entry points, rcmvs_last_error_string for the message, a HIP stream as void*). */
#ifndef RCMVS_VIEW_SELECT_H
#define RCMVS_VIEW_SELECT_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- COLMAP import (rc_mvsnet_amd/colmap_import.py; csrc/view_select.hip; additive, RCMVS_VERSION stays 106) ----
 * Declared next to its kernels like csrc/pc_register.h; rc_mvsnet_amd/_lib.py parses this file into EXT_SIGNATURES.
 * A sparse model is n images and m 3-D points, all DEVICE arrays: centres (n,3) and points (m,3) doubles, and per image an
 * ascending duplicate-free list of point indices as CSR: offsets (n+1) int64 into ids (nnz) int32.  Offsets are clamped to
 * [0, nnz] and an index outside [0, m) is skipped by the kernels, so no input makes them read out of bounds.  All arithmetic
 * is fp64 without contraction in the order csrc/view_select_math.h writes; no floating-point atomics: two runs give the same bits. */
#define RCMVS_VS_MAX_IMAGES 4096                  /* the (n,n) fp64 score table is 134 MB there */
#define RCMVS_VS_MAX_SRC 32                       /* partners listed per image */
/* scores (n,n) doubles: scores[i][j] = the sum over the points p in both lists of w(theta_p), theta_p = the angle in degrees
 * between centre_i - X_p and centre_j - X_p as atan2(|a x b|, a.b), w = exp(-(theta - theta0)^2 / (2 sigma^2)) with
 * sigma = sigma1 if theta <= theta0, else sigma2.  One wave per pair i < j: lanes stride over the shorter list (list i when the
 * lengths agree), binary-search the longer one and add their terms in ascending order; a fixed butterfly adds the lanes and one
 * lane stores (i,j) and (j,i).  The diagonal is written as 0.  1 <= n <= RCMVS_VS_MAX_IMAGES, 1 <= m < 2^31. */
int rcmvs_vs_pair_scores(const double* centres, int n, const double* points, long long m, const long long* offsets, const int* ids,
                         long long nnz, double theta0, double sigma1, double sigma2, double* scores, void* stream);
/* Per row of scores, one block: the k best partners in the order (score descending, index ascending) among those with
 * score > 0 -> top_ids (n,k) ints (-1 where there is none), top_scores (n,k) doubles (0 there), counts (n) ints = the row's
 * partners with score > 0 (it may exceed k).  1 <= k <= RCMVS_VS_MAX_SRC. */
int rcmvs_vs_top_views(const double* scores, int n, int k, int* top_ids, double* top_scores, int* counts, void* stream);
/* Per image, one block: z = ((r20 x + r21 y) + r22 z) + t2 for every point of its list, zrow (n,4) doubles = {r20, r21, r22, t2};
 * out (n,2) doubles = the order statistics of the image's z at the two ranks of ranks (n,2) ints (0-based; a rank outside the
 * list gives NaN): an MSB-first radix select, 8 bits a pass, over the order-preserving 64-bit key of z, bit-identical to sorting
 * the values.  zkey: nnz uint64 of work (the keys, at the CSR positions). */
int rcmvs_vs_depth_ranks(const double* points, long long m, const double* zrow, int n, const long long* offsets, const int* ids,
                         long long nnz, const int* ranks, unsigned long long* zkey, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_VIEW_SELECT_H */
