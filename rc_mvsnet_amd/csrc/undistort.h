/* C ABI of the image-undistortion kernel in librcmvs_hip.so (an extension header of include/rcmvs.h: same conventions --
 * status-returning entry points, rcmvs_last_error_string for the message, a HIP stream as void*). */
#ifndef RCMVS_UNDISTORT_H
#define RCMVS_UNDISTORT_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- COLMAP import with lens distortion (rc_mvsnet_amd/colmap_import.py; csrc/undistort.hip; additive, RCMVS_VERSION stays 106) ----
 * Declared next to its kernel like csrc/view_select.h; rc_mvsnet_amd/_lib.py parses this file into EXT_SIGNATURES.
 * Resamples an image of the camera (fx, fy, cx, cy) with the polynomial (Brown) distortion dist8 = {k1, k2, p1, p2, k3, k4, k5, k6}
 * (COLMAP's SIMPLE_RADIAL / RADIAL / OPENCV / FULL_OPENCV, missing coefficients 0) to the pinhole camera (fxo, fyo, cx, cy) of the
 * same size: per output pixel the source position in fp64 (pixel centres at +0.5), bilinear over the four neighbours with the
 * border pixel repeated, round half up.  All arithmetic is fp64 without contraction in the order csrc/undistort_math.h writes.
 * src, dst: DEVICE arrays of (h, w, 3) interleaved bytes, dst != src.  dist8: HOST, 8 doubles.  blank: DEVICE, 1 int, set by the
 * call to the number of output pixels whose source position is not inside the image (us >= 0 && us < w && vs >= 0 && vs < h, so
 * NaN and +-inf are not); those are written (0, 0, 0).  No input makes the kernel read outside src.  Integer atomics only: two
 * runs give the same bytes and the same count.  h, w >= 1, h * w * 3 < 2^31; focal lengths finite and positive, the principal
 * point and the coefficients finite. */
int rcmvs_undistort_rgb8(const unsigned char* src, unsigned char* dst, int h, int w, double fx, double fy, double cx, double cy,
                         double fxo, double fyo, const double* dist8, int* blank, void* stream);
/* The same launch with the kernel's own start / stop timestamps in two caller-owned HIP events (either may be NULL), as
 * rcmvs_depth_metrics_timed does: what tools/colmap_import_bench.py reads. */
int rcmvs_undistort_rgb8_timed(const unsigned char* src, unsigned char* dst, int h, int w, double fx, double fy, double cx, double cy,
                               double fxo, double fyo, const double* dist8, int* blank, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_UNDISTORT_H */
