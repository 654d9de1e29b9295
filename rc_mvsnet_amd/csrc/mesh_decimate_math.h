// The per-element rules of mesh decimation by vertex clustering with quadric placement (rc_mvsnet_amd/mesh_decimate.py; contract
// in mesh_decimate.h).  Plain C++ shared by mesh_decimate.hip and host code, restated by tests/mesh_decimate_oracle.py with the
// same operation order: this header is normative for that order.  Floating point is fp64 under `fp contract(off)`: every
// expression below is evaluated as written, left to right, one rounding per operation, no fused multiply-add.
#pragma once
#include <cmath>

#include "mesh_clean_math.h"                                      // RCMVS_HD, mc::face_valid

namespace rcmvs {
namespace md {

constexpr double DEFAULT_REG = 1e-3;                              // lambda = reg * trace(A)

#pragma clang fp contract(off)

// ---- the lattice ----------------------------------------------------------------------------------------------------------
// a vertex takes part when its three coordinates are finite (exponent bits not all ones)
RCMVS_HD bool finite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u; }
RCMVS_HD bool finite3(float x, float y, float z) { return finite(x) && finite(y) && finite(z); }

// An unsigned key that orders finite floats as the reals order them, with -0.0 below +0.0: the minimum and the maximum of the
// keys do not depend on the order in which they are taken (integer atomicMin / atomicMax).
RCMVS_HD unsigned ordered(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RCMVS_HD float unordered(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

RCMVS_HD double origin(float lo, double cell) { return (double)lo - cell / 2.0; }
// the number of cells on an axis, as a double (the caller refuses what is not in 1 .. 2^21)
RCMVS_HD double cells(float hi, double org, double cell) { return floor(((double)hi - org) / cell) + 1.0; }
// the cell of a coordinate, as a double; the vertex is clustered when 0 <= k < g on all three axes
RCMVS_HD double cell_coord(float p, double org, double cell) { return floor(((double)p - org) / cell); }
RCMVS_HD double centre(double org, long long k, double cell) { return org + ((double)k + 0.5) * cell; }
// a coordinate in its cluster's frame, in units of the cell
RCMVS_HD double local(float p, double ctr, double cell) { return ((double)p - ctr) / cell; }
RCMVS_HD float world(double ctr, double cell, double x) { return (float)(ctr + cell * x); }

// ---- faces ------------------------------------------------------------------------------------------------------------------
// (a, b, c) rotated so that its smallest entry comes first; two triples are the same face with the same orientation when their
// rotations are equal.  For three distinct entries the smallest is unique.
RCMVS_HD void rotate_min_first(int a, int b, int c, int* r) {
    if (a <= b && a <= c) { r[0] = a; r[1] = b; r[2] = c; }
    else if (b <= a && b <= c) { r[0] = b; r[1] = c; r[2] = a; }
    else { r[0] = c; r[1] = a; r[2] = b; }
}

// ---- the quadric ------------------------------------------------------------------------------------------------------------
struct Quadric {
    double a[6];                                                  // A00 A01 A02 A11 A12 A22
    double b[3];
};

// One corner's contribution: the un-normalised plane of the face (q0, q1, q2), all three in the corner's cluster's frame.
//   n = (q1 - q0) x (q2 - q0), d = -(n . q0); A += n n^T, b += n d
RCMVS_HD void add_corner(Quadric& Q, const double* q0, const double* q1, const double* q2) {
    const double ux = q1[0] - q0[0], uy = q1[1] - q0[1], uz = q1[2] - q0[2];
    const double vx = q2[0] - q0[0], vy = q2[1] - q0[1], vz = q2[2] - q0[2];
    const double nx = uy * vz - uz * vy;
    const double ny = uz * vx - ux * vz;
    const double nz = ux * vy - uy * vx;
    const double d = -((nx * q0[0] + ny * q0[1]) + nz * q0[2]);
    Q.a[0] = Q.a[0] + nx * nx;
    Q.a[1] = Q.a[1] + nx * ny;
    Q.a[2] = Q.a[2] + nx * nz;
    Q.a[3] = Q.a[3] + ny * ny;
    Q.a[4] = Q.a[4] + ny * nz;
    Q.a[5] = Q.a[5] + nz * nz;
    Q.b[0] = Q.b[0] + nx * d;
    Q.b[1] = Q.b[1] + ny * d;
    Q.b[2] = Q.b[2] + nz * d;
}

RCMVS_HD bool fin(double v) { return __builtin_isfinite(v); }

// how a cluster's position was chosen (the RCMVS_MD_VIA_* values of mesh_decimate.h)
constexpr int VIA_QUADRIC = 0, VIA_NO_FACES = 1, VIA_SINGULAR = 2, VIA_OUTSIDE = 3, VIA_MEAN = 4;

// (A + lambda I) x = -b + lambda mean by Cramer's rule, lambda = reg * (A00 + A11 + A22).  x is written only for VIA_QUADRIC.
RCMVS_HD int solve(const Quadric& Q, const double* mean, double reg, double* x) {
    const double trace = (Q.a[0] + Q.a[3]) + Q.a[5];
    if (!fin(trace) || trace == 0.0) return VIA_NO_FACES;
    const double lam = reg * trace;
    const double m00 = Q.a[0] + lam, m11 = Q.a[3] + lam, m22 = Q.a[5] + lam;
    const double m01 = Q.a[1], m02 = Q.a[2], m12 = Q.a[4];
    const double r0 = -Q.b[0] + lam * mean[0], r1 = -Q.b[1] + lam * mean[1], r2 = -Q.b[2] + lam * mean[2];
    const double c00 = m11 * m22 - m12 * m12;                     // minors shared by the determinants
    const double c01 = m01 * m22 - m12 * m02;
    const double c02 = m01 * m12 - m11 * m02;
    const double det = (m00 * c00 - m01 * c01) + m02 * c02;
    if (!fin(det) || !(det > 0.0)) return VIA_SINGULAR;
    const double s12 = r1 * m22 - m12 * r2;
    const double s21 = r1 * m12 - m11 * r2;
    const double s02 = m01 * r2 - r1 * m02;
    const double x0 = ((r0 * c00 - m01 * s12) + m02 * s21) / det;
    const double x1 = ((m00 * s12 - r0 * c01) + m02 * s02) / det;
    const double x2 = ((m00 * (m11 * r2 - r1 * m12) - m01 * s02) + r0 * c02) / det;
    if (!fin(x0) || !fin(x1) || !fin(x2)) return VIA_SINGULAR;
    if (fabs(x0) > 0.5 || fabs(x1) > 0.5 || fabs(x2) > 0.5) return VIA_OUTSIDE;
    x[0] = x0; x[1] = x1; x[2] = x2;
    return VIA_QUADRIC;
}

// ---- colour -----------------------------------------------------------------------------------------------------------------
// the members' mean of one channel rounded half up, in integers: s the sum over the c >= 1 members
RCMVS_HD unsigned char colour(unsigned long long s, unsigned long long c) { return (unsigned char)((2ull * s + c) / (2ull * c)); }

}  // namespace md
}  // namespace rcmvs
