/* C ABI of the dynamic depth-map fusion filter in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_simplify.h,
 * whose conventions it keeps: a status-returning entry point, rcmvs_last_error_string, a HIP stream as void*, refusals that
 * launch nothing; additive, RCMVS_VERSION stays 106; rc_mvsnet_amd/_lib.py parses this file into EXT_SIGNATURES). */
#ifndef RCMVS_FUSION_DYN_H
#define RCMVS_FUSION_DYN_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- one reference view against its N source views, dynamic consistency and optional duplicate suppression (rc_mvsnet_amd/
 * fusion.py: fuse_view_dynamic; csrc/fusion_dyn.hip; the per-pixel rule is csrc/fusion_dyn_math.h's, restated by
 * tests/fusion_dyn_oracle.py; DESIGN.md, "Dynamic consistency and one point per surface") ----
 * depth_all (n_views,H,W) fp32, ref_idx, src_idx_host (HOST, N ints), conf, img, mats and N, H, W are rcmvs_fuse_view's
 * (include/rcmvs.h); n_views bounds every view index.  With dist_i (fp64, pixels) and rel_i (fp32) the reprojection distance and
 * the relative depth difference of source i exactly as rcmvs_fuse_view forms them, source i PASSES LEVEL n when
 * dist_i < (double)n * dist_base and rel_i < (float)n * rel_base.  count_n = sources that pass level n; the pixel's level is the
 * smallest n in [level_lo, level_hi] with count_n >= n, or 0; geo = level != 0.  1 <= level_lo <= level_hi <= RCMVS_FUSE_MAX_SRC
 * (level_hi may exceed N: such a level is never reached).  The averaged depth is taken over the sources that pass level_hi:
 * depth_avg = (fp32 sequential sum of their reprojected depths + depth_ref) / (count_hi + 1).
 * used (n_views,H,W) u8, may be NULL: zero-filled by the caller once per scan.  claimed = photo && geo && used[ref_idx][p] != 0;
 * final = photo && geo && !claimed; a final pixel stores 1 at used[src_i][round(y_src) * W + round(x_src)] (ties to even) for every
 * source that passes level_hi, is not the reference view itself and whose position is inside the image.  The launch reads only
 * plane ref_idx of `used` and writes only other planes, so its result does not depend on the schedule; it does depend on the
 * order in which the reference views of a scan are launched, which the caller fixes (pair.txt's, on one stream).
 * Outputs: masks (4,H,W) u8 = photo, geo, final, claimed; level (H,W) u8; depth_avg (H,W); xyz (H,W,3); rgb (H,W,3) u8 (NULL
 * together with img).  Optional (NULL to skip): dbg_depth (N,H,W) the reprojected depth where the source passes level_hi, else 0;
 * dbg_level (N,H,W) u8 the smallest level of [level_lo, level_hi] the source passes, 0 for none; dbg_xy (N,H,W,2) as
 * rcmvs_fuse_view's. */
int rcmvs_fuse_view_dyn(const float* depth_all, int n_views, int ref_idx, const int* src_idx_host, const float* conf, const float* img,
                        const double* mats, float prob_thresh, int level_lo, int level_hi, double dist_base, float rel_base,
                        unsigned char* used, unsigned char* masks, unsigned char* level, float* depth_avg, float* xyz, unsigned char* rgb,
                        float* dbg_depth, unsigned char* dbg_level, float* dbg_xy, int N, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
