// Per-element rules of the Poisson reconstruction (rc_mvsnet_amd/poisson_mesh.py; kernels in poisson.hip, contract in poisson.h):
// which points are splatted, the trilinear cell and weights of a point, the fixed-point terms of the splats, the planes they become,
// the right-hand side, the mirrored Dirichlet ghost, the damped Jacobi update, the residual, the cell-centred prolongation and the
// field handed to the extraction.  Plain C++ for host and device, restated by tests/poisson_oracle.py operation by operation.
//
// Planes are fp32 and are promoted to fp64 before any arithmetic; every stored value is rounded once.  Every expression is evaluated
// under `fp contract(off)` in the order written, with + - * /, sqrt, floor, llrint (to nearest, ties to even) and comparisons only,
// so the GPU, the CPU emulation and numpy give the same bits.
#pragma once
#include <cmath>

#include "pointcloud_math.h"                                      // RCMVS_HD

namespace rcmvs {
namespace po {

constexpr double FIX = 268435456.0;                               // 2^28: the fixed point of the density and normal splats
constexpr double FIX_INV = 1.0 / 268435456.0;
constexpr double CFIX = 1048576.0;                                // 2^20: the fixed point of the colour sums (a byte needs 8 bits more)
constexpr double CFIX_INV = 1.0 / 1048576.0;
constexpr double OMEGA = 6.0 / 7.0;                               // the damping of the Jacobi smoother
constexpr int COARSEST_SWEEPS = 64;
enum { SPLATTED = 0, NON_FINITE = 1, ZERO_NORMAL = 2, OUTSIDE = 3 };

#pragma clang fp contract(off)

RCMVS_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }       // false for NaN

struct Cell { int b[3]; double w[3][2]; };                        // the lower corner's voxel and the two weights per axis

// The cell of a position and its weights.  u = (p - o) / h - 0.5 per axis is the coordinate in voxel centres; the lower corner is
// floor(u) and all eight corners must be voxels: 0 <= floor(u) <= g - 2, tested in fp64 before any conversion (NaN and +-inf fail).
RCMVS_HD bool cell_of(const float* p, const double* o, double h, const int* g, Cell* c) {
    for (int a = 0; a < 3; ++a) {
        const double u = ((double)p[a] - o[a]) / h - 0.5;
        const double f = floor(u);
        if (!(f >= 0.0 && f <= (double)(g[a] - 2))) return false;
        c->b[a] = (int)f;
        c->w[a][1] = u - f;
        c->w[a][0] = 1.0 - c->w[a][1];
    }
    return true;
}

// the class of one point, and for SPLATTED its cell and weights
RCMVS_HD int classify(const float* p, const float* n, const double* o, double h, const int* g, Cell* c) {
    for (int a = 0; a < 3; ++a)
        if (!finite((double)p[a]) || !finite((double)n[a])) return NON_FINITE;
    const double l2 = ((double)n[0] * (double)n[0] + (double)n[1] * (double)n[1]) + (double)n[2] * (double)n[2];
    if (l2 == 0.0) return ZERO_NORMAL;
    return cell_of(p, o, h, g, c) ? SPLATTED : OUTSIDE;
}

// the weight of corner `code` (dx + 2 dy + 4 dz) and its voxel number
RCMVS_HD double corner_weight(const Cell& c, int code) { return (c.w[0][code & 1] * c.w[1][(code >> 1) & 1]) * c.w[2][code >> 2]; }
RCMVS_HD long long corner_voxel(const Cell& c, int code, const int* g) {
    return (long long)(c.b[0] + (code & 1)) + (long long)g[0] * ((long long)(c.b[1] + ((code >> 1) & 1)) + (long long)g[1] * (long long)(c.b[2] + (code >> 2)));
}

// the unit normal's component a
RCMVS_HD double unit_component(const float* n, int a) {
    const double l2 = ((double)n[0] * (double)n[0] + (double)n[1] * (double)n[1]) + (double)n[2] * (double)n[2];
    return (double)n[a] / sqrt(l2);
}

// the fixed-point terms a point adds to a corner: density, one normal component, one colour channel
RCMVS_HD long long density_term(double w) { return llrint(w * FIX); }
RCMVS_HD long long normal_term(double s, double w, double nc) { return llrint(((s * w) * nc) * FIX); }
RCMVS_HD long long colour_term(double w, unsigned char byte) { return llrint((w * (double)byte) * CFIX); }

// the planes the accumulators become
RCMVS_HD float plane_of(long long acc) { return (float)((double)acc * FIX_INV); }
RCMVS_HD float colour_of(long long csum, long long wacc) {
    if (wacc == 0) return 128.0f;
    return (float)(((double)csum * CFIX_INV) / ((double)wacc * FIX_INV));
}

// Kazhdan's density normalisation: 1 / W_p, or 1 without it
RCMVS_HD double scale_of(double wp, bool density_weight) { return density_weight ? 1.0 / wp : 1.0; }

// ---- the grid rules.  A neighbour outside the grid is the ghost: MINUS the cell itself (chi = 0 on the wall between them). --------
// the six neighbours of x in the order -x +x -y +y -z +z, added from the left
RCMVS_HD double six(double xm, double xp, double ym, double yp, double zm, double zp) { return ((((xm + xp) + ym) + yp) + zm) + zp; }

RCMVS_HD double rhs(double vxm, double vxp, double vym, double vyp, double vzm, double vzp, double h) {
    return (((vxp - vxm) + (vyp - vym)) + (vzp - vzm)) / (2.0 * h);
}

RCMVS_HD double jacobi(double x, double S, double b, double h2) { return (1.0 - OMEGA) * x + (OMEGA * (S - h2 * b)) / 6.0; }

RCMVS_HD double residual(double x, double S, double b, double h2) { return b - (S - 6.0 * x) / h2; }

// one axis of the cell-centred prolongation: the parent and the neighbour on the fine cell's side
RCMVS_HD double prolong_axis(double parent, double neighbour) { return 0.75 * parent + 0.25 * neighbour; }

RCMVS_HD float field_value(float chi, double iso) { return (float)((double)chi - iso); }
RCMVS_HD float field_weight(float dmax, double trim) { return (double)dmax >= trim ? 1.0f : 0.0f; }

}  // namespace po
}  // namespace rcmvs
