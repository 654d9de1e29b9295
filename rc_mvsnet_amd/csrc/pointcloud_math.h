// Per-point predicates of the DTU point-cloud scorer (rc_mvsnet_amd/dtu_eval.py): plain C++ shared by pointcloud.hip and
// restated in numpy by the tests' fp64 oracle (tests/dtu_oracle.py) with the same operation order.
//
// Coordinates are fp32 (as in the PLY files) and are promoted to fp64 before any arithmetic.  Every expression below is
// evaluated under `fp contract(off)` in the order written, so the GPU, the CPU emulation and numpy round identically
// (sqrt and round are correctly rounded / exact everywhere): the reduction's kept mask is bit-identical to the oracle's.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RCMVS_HD __host__ __device__ inline
#else
#define RCMVS_HD inline
#endif

namespace rcmvs {
namespace pc {

enum : unsigned char { UNDECIDED = 0, KEPT = 1, REMOVED = 2 };

#pragma clang fp contract(off)
// squared Euclidean distance ((dx*dx + dy*dy) + dz*dz) of two fp32 points, in fp64
RCMVS_HD double dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// reducePts_haa's neighbourhood test (rangesearch: ||p - q|| <= dst)
RCMVS_HD bool within(float ax, float ay, float az, float bx, float by, float bz, double dst) {
    return sqrt(dist2(ax, ay, az, bx, by, bz)) <= dst;
}

// PointCompareMain's DataInMask: v = round((q - BB(1,:)) / Res + 1) (MATLAB round: half away from zero, which is C's round),
// in the mask when 1 <= v <= size in every axis and ObsMask(v) is set.  mask is column-major (MATLAB's layout): s1 x s2 x s3.
RCMVS_HD bool in_mask(float qx, float qy, float qz, const double* bb0, double res, const unsigned char* mask, int s1, int s2, int s3) {
    const double v1 = round(((double)qx - bb0[0]) / res + 1.0);
    const double v2 = round(((double)qy - bb0[1]) / res + 1.0);
    const double v3 = round(((double)qz - bb0[2]) / res + 1.0);
    if (!(v1 >= 1.0 && v1 <= (double)s1 && v2 >= 1.0 && v2 <= (double)s2 && v3 >= 1.0 && v3 <= (double)s3)) return false;
    const long long i = ((long long)v1 - 1) + (long long)s1 * (((long long)v2 - 1) + (long long)s2 * ((long long)v3 - 1));
    return mask[i] != 0;
}

// PointCompareMain's StlAbovePlane: P' * [q; 1] > 0, summed left to right
RCMVS_HD bool above_plane(float qx, float qy, float qz, const double* P) {
    return ((P[0] * (double)qx + P[1] * (double)qy) + P[2] * (double)qz) + P[3] > 0.0;
}

// MaxDistCP's 60 mm block lattice: a from-point outside [lo, hi) in some axis is never visited there
RCMVS_HD bool in_lattice(float qx, float qy, float qz, const double* lo, const double* hi) {
    const double x = qx, y = qy, z = qz;
    return x >= lo[0] && y >= lo[1] && z >= lo[2] && x < hi[0] && y < hi[1] && z < hi[2];
}

}  // namespace pc
}  // namespace rcmvs
