// Arithmetic and tables of the TSDF fusion and the marching-tetrahedra extraction (rc_mvsnet_amd/tsdf_mesh.py): plain C++ shared
// by tsdf_mesh.hip and restated by the tests' fp64 oracle (tests/tsdf_oracle.py) with the same operation order, so the planes, the
// vertices and the faces can be demanded equal in every bit.  Everything is fp64 under `fp contract(off)`.  MVSNet's pixel
// convention: the centre of pixel (i, j) is (i, j), as in fusion.hip.
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
namespace tsdf {

constexpr int MAX_VIEWS = 16;

// the voxel grid: voxel (i, j, k) has the number i + gx * (j + gy * k) and the centre o + (idx + 0.5) * h
struct Grid {
    double ox, oy, oz, h;
    int gx, gy, gz;
};

// n views, each {R row-major 9, t 3, fx, fy, cx, cy}, world -> camera.  Passed to the kernel by value (2 KiB of uniform loads).
struct Cams {
    double c[MAX_VIEWS][16];
};

#pragma clang fp contract(off)
RCMVS_HD double centre(double o, int idx, double h) { return o + ((double)idx + 0.5) * h; }

// One view of one voxel centre (px, py, pz): true when the view sees the voxel in front of or on the truncated surface; then
// *val = min(1, sdf / trunc) and *pix = the pixel's index in the H x W image.  The pixel test is made on the fp64 position
// before any conversion, so NaN and +-inf fail and no index outside the image is ever formed.
RCMVS_HD bool observe(const double* c, double px, double py, double pz, const float* depth, int H, int W, double trunc, double* val, int* pix) {
    const double xc = ((c[0] * px + c[1] * py) + c[2] * pz) + c[9];
    const double yc = ((c[3] * px + c[4] * py) + c[5] * pz) + c[10];
    const double zc = ((c[6] * px + c[7] * py) + c[8] * pz) + c[11];
    if (!(zc > 0.0)) return false;
    const double u = c[12] * (xc / zc) + c[14];
    const double v = c[13] * (yc / zc) + c[15];
    const double ub = u + 0.5, vb = v + 0.5;
    if (!(ub >= 0.0 && ub < (double)W && vb >= 0.0 && vb < (double)H)) return false;
    const int p = (int)floor(vb) * W + (int)floor(ub);
    const float d = depth[p];
    if (!(d > 0.0f && d <= 3.402823466e+38f)) return false;       // finite and positive (NaN fails both)
    const double sdf = (double)d - zc;
    if (sdf < -trunc) return false;
    const double q = sdf / trunc;
    *val = q > 1.0 ? 1.0 : q;
    *pix = p;
    return true;
}

// where the surface crosses the edge from the lower voxel (value da) to the higher (db); exactly one of them is < 0
RCMVS_HD double crossing(double da, double db) { return da / (da - db); }
RCMVS_HD double lerp(double a, double b, double t) { return a + t * (b - a); }
RCMVS_HD unsigned char colour_byte(double ca, double cb, double t) {
    const double x = floor(lerp(ca, cb, t) + 0.5);
    return (unsigned char)(int)(x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x));
}

// ---- marching tetrahedra ----------------------------------------------------------------------------------------------------
// Cube corner code dx + 2 dy + 4 dz.  The Kuhn split along the 0-7 diagonal: every tetrahedron is 0 -> a -> a|b -> 7, so it is
// the same in every cube and the triangles on a cube face match the neighbour's.  Along a tetrahedron the codes grow by one bit
// at a time: the edge between local corners a < b belongs to the voxel at code T[a] and has the edge code T[b] ^ T[a].
RCMVS_HD int tet_corner(int t, int c) {
    constexpr unsigned char T[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
    return T[t][c];
}

// sign of det [P1 - P0, P2 - P0, P3 - P0] of each tetrahedron
RCMVS_HD int tet_sign(int t) {
    constexpr signed char S[6] = {1, -1, -1, 1, 1, -1};
    return S[t];
}

// The 16 cases of a tetrahedron (bit c of the case = local corner c inside): the number of triangles and their edges, an edge
// between local corners a < b written 4 a + b, in the order a tetrahedron of POSITIVE determinant emits them; one of negative
// determinant swaps the last two edges of each triangle.  One corner apart: the triangle over its three edges, the other corners
// ascending, turned by the parity of [corner, others] (and once more when the corner is the outside one).  Two and two: the quad
// (i0o0, i0o1, i1o1, i1o0) as (q0, q1, q2), (q0, q2, q3), turned by the parity of [i0, i1, o0, o1].  Every normal
// (v1 - v0) x (v2 - v0) then points from the inside (negative) corners to the outside ones.
struct TetCase {
    unsigned char n, e[6];
};
RCMVS_HD TetCase tet_case(int m) {
    constexpr TetCase C[16] = {
        {0, {0, 0, 0, 0, 0, 0}},      // 0000
        {1, {1, 2, 3, 0, 0, 0}},      // 1000
        {1, {1, 7, 6, 0, 0, 0}},      // 0100
        {2, {2, 3, 7, 2, 7, 6}},      // 1100
        {1, {2, 6, 11, 0, 0, 0}},     // 0010
        {2, {1, 11, 3, 1, 6, 11}},    // 1010
        {2, {1, 7, 11, 1, 11, 2}},    // 0110
        {1, {3, 7, 11, 0, 0, 0}},     // 1110
        {1, {3, 11, 7, 0, 0, 0}},     // 0001
        {2, {1, 2, 11, 1, 11, 7}},    // 1001
        {2, {1, 11, 6, 1, 3, 11}},    // 0101
        {1, {2, 11, 6, 0, 0, 0}},     // 1101
        {2, {2, 6, 7, 2, 7, 3}},      // 0011
        {1, {1, 6, 7, 0, 0, 0}},      // 1011
        {1, {1, 3, 2, 0, 0, 0}},      // 0111
        {0, {0, 0, 0, 0, 0, 0}},      // 1111
    };
    return C[m];
}

// number of set bits of a 7-bit edge mask
RCMVS_HD int popcount7(unsigned m) {
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (int)((m & 0x0fu) + (m >> 4));
}

}  // namespace tsdf
}  // namespace rcmvs
