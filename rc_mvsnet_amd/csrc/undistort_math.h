// Arithmetic of the image undistortion of the COLMAP import (rc_mvsnet_amd/colmap_import.py): plain C++ shared by undistort.hip
// and restated by the tests' fp64 oracle (tests/undistort_oracle.py) with the same operation order, so the bytes can be demanded
// equal.  Everything is fp64 under `fp contract(off)`.  COLMAP's pixel convention: the centre of pixel (i, j) is (i + 0.5, j + 0.5).
#pragma once
#include <cmath>

#ifndef RCMVS_HD
#if defined(__HIPCC__)
#define RCMVS_HD __host__ __device__ inline
#else
#define RCMVS_HD inline
#endif
#endif

namespace rcmvs {
namespace ud {

// the source camera (fx, fy, cx, cy) with its distortion d = {k1, k2, p1, p2, k3, k4, k5, k6} and the focal lengths of the output
// pinhole camera (fxo, fyo), which keeps the principal point and the size.  Passed to the kernel by value.
struct Camera {
    double fx, fy, cx, cy, fxo, fyo;
    double d[8];
};

#pragma clang fp contract(off)
// Where output pixel (column i, row j) looks in the source image: the pixel centre through the output camera onto the
// normalised plane, COLMAP's SIMPLE_RADIAL / RADIAL / OPENCV / FULL_OPENCV distortion (missing coefficients are 0), then the
// source camera.  A vanishing denominator or an overflow gives NaN or +-inf, which valid() refuses.
RCMVS_HD void source_position(const Camera& c, int i, int j, double* us, double* vs) {
    const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3], k3 = c.d[4], k4 = c.d[5], k5 = c.d[6], k6 = c.d[7];
    const double x = (((double)i + 0.5) - c.cx) / c.fxo;
    const double y = (((double)j + 0.5) - c.cy) / c.fyo;
    const double r2 = x * x + y * y;
    const double rad = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)));
    const double xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x));
    const double yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y);
    *us = c.fx * xd + c.cx;
    *vs = c.fy * yd + c.cy;
}

// inside the source image; written so that NaN and +-inf are not.  Tested before any conversion to an integer.
RCMVS_HD bool valid(double us, double vs, int w, int h) { return us >= 0.0 && us < (double)w && vs >= 0.0 && vs < (double)h; }

// one axis of the bilinear footprint of a VALID position u in an image of n pixels: s = clamp(u - 0.5, 0, n - 1) (half a pixel at
// the border samples the border pixel), i0 = floor(s), i1 = min(i0 + 1, n - 1), a = s - i0.  0 <= i0 <= i1 <= n - 1.
RCMVS_HD void footprint(double u, int n, int* i0, int* i1, double* a) {
    double s = u - 0.5;
    s = s < 0.0 ? 0.0 : s;
    s = s > (double)(n - 1) ? (double)(n - 1) : s;
    const double f = floor(s);
    *i0 = (int)f;
    *i1 = *i0 + 1 < n - 1 ? *i0 + 1 : n - 1;
    *a = s - f;
}

// the blend of the four neighbours {p00 p01; p10 p11} (row, column): two horizontal blends, the vertical one, round half up
RCMVS_HD unsigned char blend(unsigned char p00, unsigned char p01, unsigned char p10, unsigned char p11, double ax, double ay) {
    const double a = (double)p00, b = (double)p01, c = (double)p10, d = (double)p11;
    const double top = a + ax * (b - a);
    const double bot = c + ax * (d - c);
    const double v = top + ay * (bot - top);
    return (unsigned char)(int)(v + 0.5);
}

}  // namespace ud
}  // namespace rcmvs
