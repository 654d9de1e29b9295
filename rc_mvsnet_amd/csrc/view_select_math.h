// Arithmetic of the COLMAP import (rc_mvsnet_amd/colmap_import.py): plain C++ shared by view_select.hip and restated by the
// tests' fp64 oracle (tests/colmap_oracle.py) with the same operation order.  Everything is fp64 under `fp contract(off)`.
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
namespace vs {

#pragma clang fp contract(off)
// the angle in degrees that the centres ci and cj subtend at x: a = ci - x, b = cj - x, atan2(|a x b|, a.b) * (180 / pi).
// Well conditioned at small angles (acos is not); a point on a centre gives atan2(0, 0) = 0.
RCMVS_HD double angle_deg(const double* ci, const double* cj, const double* x) {
    const double a0 = ci[0] - x[0], a1 = ci[1] - x[1], a2 = ci[2] - x[2];
    const double b0 = cj[0] - x[0], b1 = cj[1] - x[1], b2 = cj[2] - x[2];
    const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const double cross = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    const double dot = (a0 * b0 + a1 * b1) + a2 * b2;
    return atan2(cross, dot) * (180.0 / 3.14159265358979323846);
}

// exp(-(theta - theta0)^2 / (2 sigma^2)), sigma = sigma1 up to theta0 and sigma2 beyond (both give 1 at theta0)
RCMVS_HD double weight(double theta, double theta0, double sigma1, double sigma2) {
    const double sigma = theta <= theta0 ? sigma1 : sigma2;
    const double d = theta - theta0;
    return exp(-(d * d) / (2.0 * sigma * sigma));
}

// depth of x in a camera whose third extrinsic row is r = {r20, r21, r22, t2}: left to right
RCMVS_HD double depth(const double* r, const double* x) { return ((r[0] * x[0] + r[1] * x[1]) + r[2] * x[2]) + r[3]; }

// order-preserving key of a double (negative: all bits flipped; otherwise the sign bit set) and its inverse
RCMVS_HD unsigned long long order_key(double z) {
    unsigned long long b;
    __builtin_memcpy(&b, &z, 8);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
RCMVS_HD double key_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    double z;
    __builtin_memcpy(&z, &b, 8);
    return z;
}

}  // namespace vs
}  // namespace rcmvs
