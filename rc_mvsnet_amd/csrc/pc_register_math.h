// Knife-edge arithmetic of the Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py): plain C++ shared by pc_register.hip
// and restated by the tests' fp64 oracle (tests/tanks_fscore_oracle.py) with the same operation order.
//
// Coordinates are fp32 and are promoted to fp64 before any arithmetic.  Every expression below is evaluated under
// `fp contract(off)` in the order written, so the GPU, the CPU emulation and numpy round identically: crop flags, voxel
// indices and the nearest-neighbour comparisons are bit-identical to the oracle's.
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
namespace pcr {

#pragma clang fp contract(off)
// row a of the 4x4 row-major T applied to (x, y, z, 1): ((T0 x + T1 y) + T2 z) + T3.  The last row of T is not read.
RCMVS_HD double xform(const double* T, int a, double x, double y, double z) {
    return ((T[4 * a + 0] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
}

// Open3D's SelectionPolygonVolume, even-odd rule: over the edges (i, j = i - 1 mod m) that straddle pv
// ((v_i < pv && v_j >= pv) || (v_j < pv && v_i >= pv)) count the crossings u_i + (pv - v_i) / (v_j - v_i) * (u_j - u_i) < pu
RCMVS_HD bool in_polygon(double pu, double pv, const double* u, const double* v, int m) {
    bool odd = false;
    int j = m - 1;
    for (int i = 0; i < m; ++i) {
        if ((v[i] < pv && v[j] >= pv) || (v[j] < pv && v[i] >= pv)) {
            const double x = u[i] + (pv - v[i]) / (v[j] - v[i]) * (u[j] - u[i]);
            if (x < pu) odd = !odd;
        }
        j = i;
    }
    return odd;
}

// the crop test on an fp32 point: axis_min <= p[axis] <= axis_max and (u, v) = the two other coordinates, in axis order, inside
RCMVS_HD bool in_crop(float x, float y, float z, int axis, double amin, double amax, const double* u, const double* v, int m) {
    const double p[3] = {(double)x, (double)y, (double)z};
    if (!(p[axis] >= amin && p[axis] <= amax)) return false;
    const double pu = p[axis == 0 ? 1 : 0], pv = p[axis == 2 ? 1 : 2];
    return in_polygon(pu, pv, u, v, m);
}

// voxel index of one coordinate: floor((p - org) / voxel), org = min - voxel / 2 (computed once by the caller)
RCMVS_HD long long voxel_coord(float p, double org, double voxel) {
    return (long long)floor(((double)p - org) / voxel);
}

// squared distance ((dx*dx + dy*dy) + dz*dz) of an fp64 query to an fp32 point
RCMVS_HD double dist2(double ax, double ay, double az, float bx, float by, float bz) {
    const double dx = ax - (double)bx, dy = ay - (double)by, dz = az - (double)bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// histogram bin of a distance: floor(d / w) as a double (the caller drops what is not in [0, nbins))
RCMVS_HD double hist_bin(double d, double w) { return floor(d / w); }

}  // namespace pcr
}  // namespace rcmvs
