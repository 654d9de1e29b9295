// Per-element rules of the point-cloud clean-up (rc_mvsnet_amd/cloud_clean.py; kernels in cloud_knn.hip, contract in cloud_knn.h):
// the order of two neighbour candidates, the mean neighbour distance, the statistical threshold, and the normal of a neighbourhood
// (covariance, cyclic Jacobi, the choice and the orientation of the eigenvector).  Plain C++ for host and device, restated by
// tests/cloud_clean_oracle.py operation by operation.
//
// Coordinates are fp32 and are promoted to fp64 before any arithmetic.  Every expression is evaluated under `fp contract(off)` in
// the order written, with + - * /, sqrt, fabs and comparisons only (all correctly rounded everywhere), so the GPU, the CPU emulation
// and numpy give the same bits.
#pragma once
#include <cmath>

#include "pointcloud_math.h"                                      // RCMVS_HD, pc::dist2

namespace rcmvs {
namespace ck {

constexpr int MAX_K = 32;
constexpr int MAX_SWEEPS = 32;                                    // CK_MAX_SWEEPS: a cyclic Jacobi of a symmetric 3 x 3 needs about 6 to 10
constexpr double DEGENERATE = 1e-12;                              // lambda1 <= DEGENERATE lambda2: no plane through the neighbourhood
enum { WITH_NORMAL = 0, TOO_FEW = 1, DEGENERATE_N = 2, UNCONVERGED = 3, UNORIENTED = 4, FLIPPED = 5, ORIENTED = 6 };

#pragma clang fp contract(off)

// (d2, index) ascending: is candidate a before b?
RCMVS_HD bool before(double a_d2, int a_idx, double b_d2, int b_idx) { return a_d2 < b_d2 || (a_d2 == b_d2 && a_idx < b_idx); }

// the statistical filter's bound mu + ratio sigma; ratio = +inf keeps every valid point (also where sigma is 0)
RCMVS_HD double threshold(double mu, double sigma, double ratio) {
    if (ratio > 1.7976931348623157e308) return ratio;
    return mu + ratio * sigma;
}

struct Sym3 { double xx, xy, xz, yy, yz, zz; };

// One point of the two passes over a neighbourhood.  Pass 1 adds the coordinates (s), pass 2 the products of the differences to
// the mean; both run over the point first and then its existing neighbours in slot order.
RCMVS_HD void cov_add(const double* mean, float px, float py, float pz, Sym3* c) {
    const double dx = (double)px - mean[0], dy = (double)py - mean[1], dz = (double)pz - mean[2];
    c->xx = c->xx + dx * dx;
    c->xy = c->xy + dx * dy;
    c->xz = c->xz + dx * dz;
    c->yy = c->yy + dy * dy;
    c->yz = c->yz + dy * dz;
    c->zz = c->zz + dz * dz;
}

RCMVS_HD void cov_finish(Sym3* c, int m) {
    const double d = (double)m;
    c->xx = c->xx / d;
    c->xy = c->xy / d;
    c->xz = c->xz / d;
    c->yy = c->yy / d;
    c->yz = c->yz / d;
    c->zz = c->zz / d;
}

// One Jacobi rotation of the pair (p, q), r the third index: app, aqq the diagonal entries, apq the entry to annihilate, arp, arq
// the third row's; vp, vq the two columns of the eigenvector matrix.  apq is set to 0 exactly.
RCMVS_HD void rotate(double* app, double* aqq, double* apq, double* arp, double* arq, double* vp, double* vq) {
    const double theta = (*aqq - *app) / (2.0 * *apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * *apq;
    *app = *app - h;
    *aqq = *aqq + h;
    *apq = 0.0;
    const double rp = *arp, rq = *arq;
    *arp = c * rp - s * rq;
    *arq = s * rp + c * rq;
    for (int i = 0; i < 3; ++i) {
        const double a = vp[i], b = vq[i];
        vp[i] = c * a - s * b;
        vq[i] = s * a + c * b;
    }
}

// Cyclic Jacobi over (0,1), (0,2), (1,2); a rotation is skipped when its entry is exactly 0, and the iteration ends after a sweep
// that rotated nothing.  lam: the diagonal at the end; v0, v1, v2: the columns.  -> false when MAX_SWEEPS sweeps all rotated.
RCMVS_HD bool jacobi(const Sym3& c, double* lam, double* v0, double* v1, double* v2) {
    double a00 = c.xx, a01 = c.xy, a02 = c.xz, a11 = c.yy, a12 = c.yz, a22 = c.zz;
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
    v1[0] = 0.0; v1[1] = 1.0; v1[2] = 0.0;
    v2[0] = 0.0; v2[1] = 0.0; v2[2] = 1.0;
    bool done = false;
    for (int sweep = 0; sweep < MAX_SWEEPS && !done; ++sweep) {
        done = true;
        if (a01 != 0.0) { rotate(&a00, &a11, &a01, &a02, &a12, v0, v1); done = false; }
        if (a02 != 0.0) { rotate(&a00, &a22, &a02, &a01, &a12, v0, v2); done = false; }
        if (a12 != 0.0) { rotate(&a11, &a22, &a12, &a01, &a02, v1, v2); done = false; }
    }
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
    return done || (a01 == 0.0 && a02 == 0.0 && a12 == 0.0);
}

// The normal of a covariance: the eigenvector of the smallest eigenvalue (ties to the lower column), normalised, its component of
// largest magnitude (ties to the first) made positive.  -> WITH_NORMAL or DEGENERATE_N (n = 0 then); *converged as jacobi's.
RCMVS_HD int normal_of(const Sym3& c, double* n, bool* converged) {
    double lam[3], v[3][3];
    *converged = jacobi(c, lam, v[0], v[1], v[2]);
    // the order of the three eigenvalues by selects (no indexed registers): lo, mid, hi with ties to the lower column
    int lo = 0;
    if (lam[1] < lam[lo]) lo = 1;
    if (lam[2] < lam[lo]) lo = 2;
    int hi = 2;
    if (lam[1] > lam[hi]) hi = 1;
    if (lam[0] > lam[hi]) hi = 0;
    const int mid = 3 - lo - hi;
    const double l1 = mid == 0 ? lam[0] : (mid == 1 ? lam[1] : lam[2]);
    const double l2 = hi == 0 ? lam[0] : (hi == 1 ? lam[1] : lam[2]);
    n[0] = n[1] = n[2] = 0.0;
    if (l2 == 0.0 || !(l1 > DEGENERATE * l2)) return DEGENERATE_N;
    const double x = lo == 0 ? v[0][0] : (lo == 1 ? v[1][0] : v[2][0]);
    const double y = lo == 0 ? v[0][1] : (lo == 1 ? v[1][1] : v[2][1]);
    const double z = lo == 0 ? v[0][2] : (lo == 1 ? v[1][2] : v[2][2]);
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0)) return DEGENERATE_N;
    double ux = x / len, uy = y / len, uz = z / len;
    const double ax = fabs(ux), ay = fabs(uy), az = fabs(uz);
    const double big = ax >= ay && ax >= az ? ux : (ay >= az ? uy : uz);
    if (big < 0.0) { ux = -ux; uy = -uy; uz = -uz; }
    n[0] = ux; n[1] = uy; n[2] = uz;
    return WITH_NORMAL;
}

// flip n towards the centre c seen from p: true when n . (c - p) < 0 (0 keeps n)
RCMVS_HD bool orient(double* n, float px, float py, float pz, const double* c) {
    const double dx = c[0] - (double)px, dy = c[1] - (double)py, dz = c[2] - (double)pz;
    const double d = (n[0] * dx + n[1] * dy) + n[2] * dz;
    if (!(d < 0.0)) return false;
    n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2];
    return true;
}

}  // namespace ck
}  // namespace rcmvs
