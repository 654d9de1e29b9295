// The marking rule of the block-sparse TSDF volume (rc_mvsnet_amd/tsdf_mesh.py SparseTsdfVolume; contract in tsdf_sparse.h): which
// 8 x 8 x 8-voxel blocks the truncation slab of one depth pixel can touch.  Plain C++ shared by tsdf_sparse.hip and restated by
// tests/tsdf_sparse_oracle.py with the same operation order.  Everything is fp64 under `fp contract(off)`; everything per voxel is
// tsdf_mesh_math.h's, unchanged.
#pragma once
#include <cmath>

#include "tsdf_mesh_math.h"

namespace rcmvs {
namespace tsdf_sp {

constexpr int BLOCK = 8;                                          // voxels per block side
constexpr int BLOCK_VOXELS = BLOCK * BLOCK * BLOCK;
constexpr int MARK_SPAN = 4;                                      // blocks per axis a pixel may mark

// the virtual grid: bx x by x bz blocks, block (X, Y, Z) has the number X + bx * (Y + by * Z); voxels as in tsdf::Grid of 8 * bdims
struct BlockGrid {
    double ox, oy, oz, h;
    int bx, by, bz;
};

enum MarkResult { MARK_NOTHING = 0, MARK_SKIPPED = 1, MARK_RANGE = 2 };

#pragma clang fp contract(off)
// Pixel (i, j) (column, row) of depth d seen by the view c = {R row-major 9, t 3, fx, fy, cx, cy}: the slab d - trunc .. d + trunc of
// the pixel's footprint, back-projected, its bounding box grown by h, in blocks.  MARK_RANGE: bl[k] .. bh[k] (inclusive, inside the
// grid, at most MARK_SPAN per axis) are to be marked.  MARK_SKIPPED: a coordinate is not finite or a range is longer than MARK_SPAN
// (the caller counts it).  MARK_NOTHING: no usable depth, or the box misses the grid.  Every comparison is made in fp64 before any
// conversion and written so that NaN fails it, so no block number outside the grid is ever formed.
RCMVS_HD MarkResult mark_range(const double* c, int i, int j, float depth, double trunc, const BlockGrid& g, int* bl, int* bh) {
    if (!(depth > 0.0f && depth <= 3.402823466e+38f)) return MARK_NOTHING;      // finite and positive (NaN fails both)
    const double d = (double)depth;
    double z0 = d - trunc;
    if (!(z0 > 0.0)) z0 = 0.0;
    const double z1 = d + trunc;
    double lo[3], hi[3];
    bool finite = true;
    for (int n = 0; n < 8; ++n) {
        const double z = (n & 4) ? z1 : z0;
        const double a = (double)i + ((n & 1) ? 0.5 : -0.5), b = (double)j + ((n & 2) ? 0.5 : -0.5);
        const double xc = ((a - c[14]) / c[12]) * z;
        const double yc = ((b - c[15]) / c[13]) * z;
        const double q0 = xc - c[9], q1 = yc - c[10], q2 = z - c[11];
        for (int k = 0; k < 3; ++k) {
            const double w = (c[k] * q0 + c[3 + k] * q1) + c[6 + k] * q2;
            finite = finite && std::isfinite(w);
            if (n == 0 || w < lo[k]) lo[k] = w;
            if (n == 0 || w > hi[k]) hi[k] = w;
        }
    }
    const double o[3] = {g.ox, g.oy, g.oz};
    const int bdim[3] = {g.bx, g.by, g.bz};
    const double edge = 8.0 * g.h;
    double fl[3], fh[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = lo[k] - g.h;
        hi[k] = hi[k] + g.h;
        finite = finite && std::isfinite(lo[k]) && std::isfinite(hi[k]);
    }
    if (!finite) return MARK_SKIPPED;
    for (int k = 0; k < 3; ++k) {
        fl[k] = floor((lo[k] - o[k]) / edge);
        fh[k] = floor((hi[k] - o[k]) / edge);
        if (!(fh[k] >= 0.0 && fl[k] < (double)bdim[k])) return MARK_NOTHING;
    }
    for (int k = 0; k < 3; ++k) {
        const double cl = fl[k] < 0.0 ? 0.0 : fl[k], ch = fh[k] > (double)(bdim[k] - 1) ? (double)(bdim[k] - 1) : fh[k];
        if (ch - cl + 1.0 > (double)MARK_SPAN) return MARK_SKIPPED;
        bl[k] = (int)cl;
        bh[k] = (int)ch;
    }
    return MARK_RANGE;
}

// the slot of block B among the set bits of the mask: the same lookup the emit kernels use for a voxel's vertices
RCMVS_HD unsigned bits_below(unsigned word, unsigned bit) { return word & ((1u << bit) - 1u); }

}  // namespace tsdf_sp
}  // namespace rcmvs
