// The per-element rules of mesh simplification by quadric edge collapse in independent sets (rc_mvsnet_amd/mesh_simplify.py;
// contract in mesh_simplify.h).  Plain C++ shared by mesh_simplify.hip and host code, restated by tests/mesh_simplify_oracle.py with
// the same operation order: this header is normative for that order.  Floating point is fp64 under `fp contract(off)`: every
// expression below is evaluated as written, left to right, one rounding per operation, no fused multiply-add.
#pragma once
#include <cmath>

#include "mesh_decimate_math.h"                                   // md::finite3, md::ordered, md::local, md::world, md::colour, md::fin

namespace rcmvs {
namespace ms {

#pragma clang fp contract(off)

// ---- the frame --------------------------------------------------------------------------------------------------------------
// One frame for the whole call: the centre of the finite vertices' box (md::ordered keys of rcmvs_md_bounds) in units of its
// longest side.  x = md::local(p, centre, side) = ((double)p - centre) / side, p = md::world(centre, side, x) = (float)(centre +
// side * x).  A box of no extent (or no finite vertex: centre 0) takes side 1.
RCMVS_HD double centre(float lo, float hi) { return ((double)lo + (double)hi) * 0.5; }
RCMVS_HD double side(const float* lo, const float* hi) {
    double s = (double)hi[0] - (double)lo[0];
    const double sy = (double)hi[1] - (double)lo[1], sz = (double)hi[2] - (double)lo[2];
    if (sy > s) s = sy;
    if (sz > s) s = sz;
    return s > 0.0 ? s : 1.0;
}

// ---- the quadric ------------------------------------------------------------------------------------------------------------
// cost(x) = x^T A x + 2 b^T x + c
struct Quadric {
    double a[6];                                                  // A00 A01 A02 A11 A12 A22
    double b[3];
    double c;
};
constexpr int QUADRIC_DOUBLES = 10;                               // a row of the quadric array: a[0 .. 6), b[0 .. 3), c

RCMVS_HD Quadric zero() { return Quadric{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0}; }

// One corner's contribution: the un-normalised plane of its face (q0, q1, q2 in corner order, frame coordinates), the same for
// the face's three corners.  n = (q1 - q0) x (q2 - q0), |n| = twice the area, d = -(n . q0): the squared distance to the plane
// WEIGHTED BY FOUR TIMES THE SQUARED AREA, as md::add_corner weighs it.  (The area itself would need a square root and a division
// per face: a planar patch with dyadic coordinates would stop being exactly planar, and the exact known answers with it.)
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
    Q.c = Q.c + d * d;
}

// the quadric of a merged vertex: u's plus v's, u < v
RCMVS_HD Quadric add(const Quadric& U, const Quadric& V) {
    Quadric Q;
    for (int j = 0; j < 6; ++j) Q.a[j] = U.a[j] + V.a[j];
    for (int j = 0; j < 3; ++j) Q.b[j] = U.b[j] + V.b[j];
    Q.c = U.c + V.c;
    return Q;
}

// the quadric at x; negative rounding noise is clamped to 0, a NaN stays a NaN
RCMVS_HD double cost(const Quadric& Q, const double* x) {
    const double r0 = (Q.a[0] * x[0] + Q.a[1] * x[1]) + Q.a[2] * x[2];
    const double r1 = (Q.a[1] * x[0] + Q.a[3] * x[1]) + Q.a[4] * x[2];
    const double r2 = (Q.a[2] * x[0] + Q.a[4] * x[1]) + Q.a[5] * x[2];
    const double quad = (x[0] * r0 + x[1] * r1) + x[2] * r2;
    const double lin = (Q.b[0] * x[0] + Q.b[1] * x[1]) + Q.b[2] * x[2];
    const double v = (quad + 2.0 * lin) + Q.c;
    return v < 0.0 ? 0.0 : v;
}

// ---- placement --------------------------------------------------------------------------------------------------------------
// how an edge's target position was chosen (the RCMVS_MS_PATH_* values of mesh_simplify.h)
constexpr int PATH_LOCKED = 0, PATH_QUADRIC = 1, PATH_MIDPOINT = 2, PATH_END_U = 3, PATH_END_V = 4, PATHS = 5;
// which position the target is: computed, or one endpoint's coordinates copied in every bit
constexpr int FROM_X = 0, FROM_U = 1, FROM_V = 2;

constexpr double DET_EPS = 1e-9;                                  // A is singular when det <= DET_EPS trace^3
constexpr double FAR = 4.0;                                       // a minimiser further than 2 edge lengths from the midpoint is no answer

// A x = -b by Cramer's rule (md::solve without its regularisation): true and x when A is well enough conditioned, the answer is
// finite and lies within sqrt(FAR) edge lengths of the edge's midpoint mid (len2: the squared edge length).
RCMVS_HD bool solve(const Quadric& Q, const double* mid, double len2, double* x) {
    const double trace = (Q.a[0] + Q.a[3]) + Q.a[5];
    if (!md::fin(trace) || !(trace > 0.0)) return false;
    const double m00 = Q.a[0], m11 = Q.a[3], m22 = Q.a[5], m01 = Q.a[1], m02 = Q.a[2], m12 = Q.a[4];
    const double r0 = -Q.b[0], r1 = -Q.b[1], r2 = -Q.b[2];
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m01 * m22 - m12 * m02;
    const double c02 = m01 * m12 - m11 * m02;
    const double det = (m00 * c00 - m01 * c01) + m02 * c02;
    if (!md::fin(det) || !(det > DET_EPS * ((trace * trace) * trace))) return false;
    const double s12 = r1 * m22 - m12 * r2;
    const double s21 = r1 * m12 - m11 * r2;
    const double s02 = m01 * r2 - r1 * m02;
    const double x0 = ((r0 * c00 - m01 * s12) + m02 * s21) / det;
    const double x1 = ((m00 * s12 - r0 * c01) + m02 * s02) / det;
    const double x2 = ((m00 * (m11 * r2 - r1 * m12) - m01 * s02) + r0 * c02) / det;
    if (!md::fin(x0) || !md::fin(x1) || !md::fin(x2)) return false;
    const double e0 = x0 - mid[0], e1 = x1 - mid[1], e2 = x2 - mid[2];
    if (!(((e0 * e0 + e1 * e1) + e2 * e2) <= FAR * len2)) return false;
    x[0] = x0; x[1] = x1; x[2] = x2;
    return true;
}

// The target of the edge {u < v}: Q = add(Qu, Qv), pu / pv the endpoints in the frame.  -> the path; *from says whether the target
// is x (FROM_X) or a copy of an endpoint.  A locked endpoint is the target.  Otherwise the minimiser of Q; failing that, whichever
// of the midpoint, u and v has the lowest cost, ties in that order (plain < : a NaN never compares lower).
RCMVS_HD int place(const Quadric& Q, const double* pu, const double* pv, bool locked_u, bool locked_v, double* x, int* from) {
    if (locked_u) { *from = FROM_U; return PATH_LOCKED; }
    if (locked_v) { *from = FROM_V; return PATH_LOCKED; }
    double mid[3];
    for (int a = 0; a < 3; ++a) mid[a] = (pu[a] + pv[a]) * 0.5;
    const double e0 = pv[0] - pu[0], e1 = pv[1] - pu[1], e2 = pv[2] - pu[2];
    const double len2 = (e0 * e0 + e1 * e1) + e2 * e2;
    *from = FROM_X;
    if (solve(Q, mid, len2, x)) return PATH_QUADRIC;
    const double cm = cost(Q, mid), cu = cost(Q, pu), cv = cost(Q, pv);
    int path = PATH_MIDPOINT;
    double best = cm;
    if (cu < best) { path = PATH_END_U; best = cu; }
    if (cv < best) { path = PATH_END_V; best = cv; }
    if (path == PATH_MIDPOINT) { x[0] = mid[0]; x[1] = mid[1]; x[2] = mid[2]; }
    else *from = path == PATH_END_U ? FROM_U : FROM_V;
    return path;
}

// ---- rejection ----------------------------------------------------------------------------------------------------------------
// an edge's state (the RCMVS_MS_EDGE_* values): a candidate that may be selected, the first reason that rejects it, or no candidate
constexpr int EDGE_OK = 0, EDGE_COST = 1, EDGE_LINK = 2, EDGE_FLIP = 3, EDGE_NONE = 255;

// the cost is compared as !(cost <= max_error): a NaN cost is rejected
RCMVS_HD bool cost_ok(double c, double max_error) { return c <= max_error; }

// the vertices two ascending rings share
RCMVS_HD int common(const int* a, int na, const int* b, int nb) {
    int i = 0, j = 0, n = 0;
    while (i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (a[i] > b[j]) ++j;
        else { ++n; ++i; ++j; }
    }
    return n;
}

// The link condition of an edge of multiplicity 2 from the rings alone: the rings share exactly the edge's two opposite vertices,
// and the merged vertex keeps at least three neighbours (lu + lv - 4: u, v and the two shared ones counted once).  The second
// half is what is left of "the links share no EDGE" on a manifold: two rings that share c, d and the edge cd are the triangles
// v c d and u c d, both of length 3 (the tetrahedron).
RCMVS_HD bool link_ok(int shared, int lu, int lv) { return shared == 2 && lu + lv - 4 >= 3; }

// A surviving face (q0, q1, q2 in corner order, frame coordinates) whose corner k moves to t keeps its side when the new cross
// product . the old one > 0 (false for a NaN, and for a face that is or becomes degenerate).
RCMVS_HD void cross(const double* q0, const double* q1, const double* q2, double* n) {
    const double ux = q1[0] - q0[0], uy = q1[1] - q0[1], uz = q1[2] - q0[2];
    const double vx = q2[0] - q0[0], vy = q2[1] - q0[1], vz = q2[2] - q0[2];
    n[0] = uy * vz - uz * vy;
    n[1] = uz * vx - ux * vz;
    n[2] = ux * vy - uy * vx;
}
RCMVS_HD bool keeps_side(const double* q0, const double* q1, const double* q2, int k, const double* t) {
    double n[3], m[3];
    cross(q0, q1, q2, n);
    cross(k == 0 ? t : q0, k == 1 ? t : q1, k == 2 ? t : q2, m);
    return ((m[0] * n[0] + m[1] * n[1]) + m[2] * n[2]) > 0.0;
}

// ---- selection ----------------------------------------------------------------------------------------------------------------
// (ordered bits of (float)cost) << 32 | the CSR entry of u -> v: unique, totally ordered; NO_KEY for everything else
constexpr unsigned long long NO_KEY = ~0ull;
RCMVS_HD unsigned long long key(double c, long long entry) { return ((unsigned long long)md::ordered((float)c) << 32) | (unsigned long long)(unsigned)entry; }

// the collapses a round may apply: each removes two faces
RCMVS_HD long long budget(long long live, long long target) { return live > target ? (live - target + 1) / 2 : 0; }

}  // namespace ms
}  // namespace rcmvs
