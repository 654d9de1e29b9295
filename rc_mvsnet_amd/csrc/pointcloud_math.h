// Per-point predicates of the DTU point-cloud scorer (rc_mvsnet_amd/dtu_eval.py) and the mesh super-sampling of its surface
// mode: plain C++ shared by pointcloud.hip / mesh_sample.hip and restated by the tests' fp64 oracles (tests/dtu_oracle.py,
// tests/mesh_oracle.py) with the same operation order.
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

// ---- mesh super-sampling: MeshSupSamp.cpp's SubTri (matlab_eval/MeshSupSamp_web), restated by tests/mesh_oracle.py --------
// The triangle (Q0, Q1, Q2) gives the points ((k1*v1) + (k2*v2)) + Q0 for the doubles c1 = 0, 1, ... while c1 <= n1 and
// c2 = 0, 1, ... while c2 <= n2 (c1-major) with k1 = (c1 + 0.5) / n1, k2 = (c2 + 0.5) / n2 and k1 + k2 < 1.  Degenerate
// triangles fall out of the arithmetic: a zero edge gives n = NaN (no loop runs), zero area with non-zero edges n = 0 and
// k = inf (nothing kept).  The keep test is monotone in c1 and in c2 (IEEE + and / are), so the kept (c1, c2) of a row are a
// prefix of it and the non-empty rows a prefix of the triangle: both are counted by binary search.
struct SubTri { double q0[3], v1[3], v2[3]; double n1, n2; };

RCMVS_HD void subtri_setup(const float* a, const float* b, const float* c, double dst, SubTri* t) {
    for (int k = 0; k < 3; ++k) {
        t->q0[k] = (double)a[k];
        t->v1[k] = (double)b[k] - t->q0[k];
        t->v2[k] = (double)c[k] - t->q0[k];
    }
    const double* v1 = t->v1;
    const double* v2 = t->v2;
    const double l1 = sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2]);
    const double l2 = sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2]);
    const double x = v1[1] * v2[2] - v1[2] * v2[1], y = v1[2] * v2[0] - v1[0] * v2[2], z = v1[0] * v2[1] - v1[1] * v2[0];
    const double area2 = sqrt((x * x + y * y) + z * z);
    const double thr = dst * sqrt((l1 * l2) / area2);
    t->n1 = floor(l1 / thr);
    t->n2 = floor(l2 / thr);
}

RCMVS_HD bool subtri_keep(double c1, double c2, double n1, double n2) {
    const double k1 = (c1 + 0.5) / n1;
    const double k2 = (c2 + 0.5) / n2;
    return k1 + k2 < 1.0;
}

// one coordinate of the point (c1, c2), in fp64 (the caller rounds it to fp32 once)
RCMVS_HD double subtri_coord(const SubTri& t, double c1, double c2, int k) {
    const double k1 = (c1 + 0.5) / t.n1;
    const double k2 = (c2 + 0.5) / t.n2;
    return (k1 * t.v1[k] + k2 * t.v2[k]) + t.q0[k];
}

// counts beyond SUBTRI_CAP are reported as SUBTRI_CAP: far past the 2^31 points the scorer accepts, and no int64 sum of
// 2^31 of them overflows
constexpr long long SUBTRI_CAP = 1ll << 31;

// iterations of `for (double c = 0; c <= n; c++)` (n is a floor: an integer, inf or NaN), capped
RCMVS_HD long long subtri_extent(double n) {
    if (!(n >= 0.0)) return 0;
    return n < (double)SUBTRI_CAP ? (long long)n + 1 : SUBTRI_CAP;
}

// non-empty rows c1 = 0 .. rows - 1 (a row is non-empty when its c2 = 0 is kept): the first c1 whose c2 = 0 is dropped
RCMVS_HD long long subtri_rows(double n1, double n2) {
    if (subtri_extent(n2) == 0) return 0;
    long long lo = 0, hi = subtri_extent(n1);
    while (lo < hi) {
        const long long c = lo + (hi - lo) / 2;
        if (subtri_keep((double)c, 0.0, n1, n2)) lo = c + 1; else hi = c;
    }
    return lo;
}

// kept points of row c1: c2 = 0 .. len - 1
RCMVS_HD long long subtri_row_len(double c1, double n1, double n2) {
    long long lo = 0, hi = subtri_extent(n2);
    while (lo < hi) {
        const long long c = lo + (hi - lo) / 2;
        if (subtri_keep(c1, (double)c, n1, n2)) lo = c + 1; else hi = c;
    }
    return lo;
}

}  // namespace pc
}  // namespace rcmvs
