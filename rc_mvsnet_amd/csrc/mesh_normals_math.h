// The per-element rules of the mesh normals (rc_mvsnet_amd/mesh_normals.py; contract in mesh_normals.h): a face's vector and unit
// normal, a corner's contribution to its vertex under the two weights, a vertex's normal from the sum of its corners, and one pixel
// of the normal pass over a rendered view.  Plain C++ shared by mesh_normals.hip and host code, restated by
// tests/mesh_normals_oracle.py with the same operation order: this header is normative for that order.  Floating point is fp64
// under `fp contract(off)`: every expression is evaluated as written, one rounding per operation.
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_render_math.h"                                     // RCMVS_HD, mc::face_valid, mr::camera, project, area2, face, weights

namespace rcmvs {
namespace mn {

constexpr int AREA = 0, SPHERE = 1;                               // weight
// the counters (RCMVS_MN_STATS uint64)
constexpr int INVALID = 0, NONFINITE = 1, DEGENERATE = 2, SKIPPED = 3, WITH_NORMAL = 4, UNREFERENCED = 5, CANCELLED = 6;
constexpr double F64_MAX = 1.7976931348623157e308;
// Magnitudes.  A finite fp32 coordinate is at most 2^128 in size, a difference of two at most 2^129 and exact in fp64 unless the
// exponents lie more than 52 apart (then it rounds once).  A component of a cross product is a difference of two products of such
// differences, below 2^259; a squared length (x x + y y) + z z of a cross product is below 3 * 2^518 < 2^520, and of an edge below
// 2^260.  AREA: a vertex sums at most 3 * 2^31 < 2^33 face vectors, each component below 2^292, the squared length of the sum
// below 2^586.  SPHERE: l1 l2 < 2^520; the smallest non-zero difference of two fp32 values is 2^-149, so a non-zero l is at least
// 2^-298 and l1 l2 at least 2^-596 -- never rounded to zero -- and |C_k| <= |e1| |e2| bounds a contribution by 1 / (|e1| |e2|) <=
// 2^298, a sum by 2^331, its squared length by 2^664.  Every intermediate of both weights stays finite below 2^1024 for every
// finite fp32 input; the tests `> 0 and finite` on squared lengths guard exact cancellation and underflow to zero (a sum whose
// components are all below 2^-538 squares to zero and the vertex counts as cancelled), not overflow.

#pragma clang fp contract(off)

struct Vec {
    double x, y, z;
};

RCMVS_HD bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }     // false for a NaN
RCMVS_HD bool finite9(const float* a, const float* b, const float* c) {
    return finite(a[0]) && finite(a[1]) && finite(a[2]) && finite(b[0]) && finite(b[1]) && finite(b[2]) && finite(c[0]) && finite(c[1]) && finite(c[2]);
}

// (q - p) x (r - p): each difference one fp64 subtraction of the fp32 coordinates, each component one product minus another
RCMVS_HD Vec cross_at(const float* p, const float* q, const float* r, double* l1, double* l2) {
    const double ux = (double)q[0] - (double)p[0], uy = (double)q[1] - (double)p[1], uz = (double)q[2] - (double)p[2];
    const double vx = (double)r[0] - (double)p[0], vy = (double)r[1] - (double)p[1], vz = (double)r[2] - (double)p[2];
    Vec n;
    n.x = uy * vz - uz * vy;
    n.y = uz * vx - ux * vz;
    n.z = ux * vy - uy * vx;
    *l1 = (ux * ux + uy * uy) + uz * uz;
    *l2 = (vx * vx + vy * vy) + vz * vz;
    return n;
}

// the face vector F = (b - a) x (c - a) of a face whose coordinates are finite
RCMVS_HD Vec face_vector(const float* a, const float* b, const float* c) {
    double l1, l2;
    return cross_at(a, b, c, &l1, &l2);
}

RCMVS_HD double length2(Vec v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
RCMVS_HD bool usable_length2(double len2) { return len2 > 0.0 && len2 <= F64_MAX; }
RCMVS_HD bool is_zero(Vec v) { return v.x == 0.0 && v.y == 0.0 && v.z == 0.0; }

// v / |v| rounded to fp32 per component; (0, 0, 0) and false when the squared length is not finite and > 0
RCMVS_HD bool unit(Vec v, float* out) {
    const double len2 = length2(v);
    if (!usable_length2(len2)) {
        out[0] = out[1] = out[2] = 0.0f;
        return false;
    }
    const double len = sqrt(len2);
    out[0] = (float)(v.x / len);
    out[1] = (float)(v.y / len);
    out[2] = (float)(v.z / len);
    return true;
}

// The contribution of the corner at p, with q the next and r the previous vertex in the face's own order.  AREA: the face vector
// of the face (a, b, c) as stored, the same bits at its three corners (fv).  SPHERE (Max's weights): C / (l1 l2) with C = (q - p) x
// (r - p); false when l1 l2 is not > 0 (the corner is skipped).
RCMVS_HD bool sphere_corner(const float* p, const float* q, const float* r, Vec* out) {
    double l1, l2;
    const Vec c = cross_at(p, q, r, &l1, &l2);
    const double d = l1 * l2;
    if (!(d > 0.0)) return false;
    out->x = c.x / d;
    out->y = c.y / d;
    out->z = c.z / d;
    return true;
}

RCMVS_HD Vec add(Vec s, Vec c) {
    Vec r;
    r.x = s.x + c.x;
    r.y = s.y + c.y;
    r.z = s.z + c.z;
    return r;
}

// ---- the normal pass over a rendered view ------------------------------------------------------------------------------------------
// One pixel that sees the valid face (a, b, c) whose projected vertices are usable and whose area2 is not zero: the weights of
// mr::weights for the pixel, q_i = (double)w_i iz_i, m = (q0 Na + q1 Nb) + q2 Nc per component, g = R m in mr::camera's order.
// false when the squared length of g is not finite and > 0.
struct Pixel {
    float normal[3];
    unsigned char smooth, rgb[3];
};
RCMVS_HD unsigned char byte_of(double x) { return (unsigned char)(int)(x >= 255.0 ? 255.0 : (x >= 0.0 ? x : 0.0)); }
RCMVS_HD bool shade_pixel(const double* cam, const mr::Face& f, int px, int py, const float* na, const float* nb, const float* nc, Pixel* out) {
    long long w[3];
    mr::weights(f, px, py, w);
    const double q0 = (double)w[0] * f.iz[0], q1 = (double)w[1] * f.iz[1], q2 = (double)w[2] * f.iz[2];
    const double mx = (q0 * (double)na[0] + q1 * (double)nb[0]) + q2 * (double)nc[0];
    const double my = (q0 * (double)na[1] + q1 * (double)nb[1]) + q2 * (double)nc[1];
    const double mz = (q0 * (double)na[2] + q1 * (double)nb[2]) + q2 * (double)nc[2];
    Vec g;
    g.x = (cam[0] * mx + cam[1] * my) + cam[2] * mz;
    g.y = (cam[3] * mx + cam[4] * my) + cam[5] * mz;
    g.z = (cam[6] * mx + cam[7] * my) + cam[8] * mz;
    const double len2 = length2(g);
    if (!usable_length2(len2)) return false;
    const double len = sqrt(len2);
    const double ex = g.x / len, ey = g.y / len, ez = g.z / len;
    out->normal[0] = (float)ex;
    out->normal[1] = (float)ey;
    out->normal[2] = (float)ez;
    out->smooth = byte_of(floor(255.0 * fabs(g.z) / len + 0.5));
    out->rgb[0] = byte_of(floor(127.5 * (ex + 1.0) + 0.5));
    out->rgb[1] = byte_of(floor(127.5 * (-ey + 1.0) + 0.5));
    out->rgb[2] = byte_of(floor(127.5 * (-ez + 1.0) + 0.5));
    return true;
}

}  // namespace mn
}  // namespace rcmvs
