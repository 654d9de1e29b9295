// Poisson surface reconstruction on a dense grid: the density and normal splats, the right-hand side, the multigrid solver, the
// isovalue and the field handed to the marching tetrahedra of tsdf_mesh.hip (rc_mvsnet_amd/poisson_mesh.py; contract in poisson.h,
// the per-element rules in poisson_math.h).
//
//   splat     one thread per point, twice: the density (8 integer atomics), then W_p from the finished density and the normal and
//             colour terms (8 x 3 or 8 x 6 integer atomics).  Fixed point in int64: the sums do not depend on the order.  One thread
//             per voxel turns the accumulators into fp32 planes.
//   rhs       one thread per voxel, a wave along x: six reads, one write.
//   sweep     damped Jacobi, one thread per voxel, a wave along x: x and b read once and x' written once from memory (12 bytes per
//             voxel), the +-y and +-z rows from L2.  Two planes are ping-ponged.
//   restrict  one thread per COARSE cell: the residuals of its eight children, averaged; the fine residual never reaches memory.
//   prolong   one thread per fine cell: eight coarse values, 3/4 and 1/4 per axis, added to x.
//   norm      max |residual| by blocks that stride over the grid, then one block over their maxima (a maximum has no order).
//   iso       one thread per point writes its terms in input order; rcmvs_pc_moments' tree adds them.
//   field     one thread per voxel: chi - iso, and the 27-voxel maximum of W against trim.
// No kernel waits for another workgroup, and there are no floating-point atomics.
// gfx950 only; __syncthreads, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <cmath>
#include <cstdint>

#include "common.h"
#include "poisson.h"
#include "poisson_math.h"
#include "scan_sort.h"                                            // gid, blocks, the overlap checks, zero_kernel

#pragma clang fp contract(off)

namespace rcmvs {

static_assert(po::COARSEST_SWEEPS == RCMVS_PO_COARSEST_SWEEPS && po::OUTSIDE < RCMVS_PO_COUNTERS && RCMVS_PO_ACC == 7, "the constants of poisson.h");
static_assert(RCMVS_PO_COARSEST_SWEEPS % 2 == 0, "the ping-pong ends in x");

using u64 = unsigned long long;
constexpr int PO_TREE = RCMVS_PC_MOMENT_BLOCKS;                   // blocks of the summation tree, each of SS_BLOCK lanes

struct PoGrid { double o[3]; double h; int g[3]; };
struct PoDims { int g[3]; };

// ---- splats -------------------------------------------------------------------------------------------------------------------------
__device__ inline void po_count(int what, long long* counters) {
    for (int c = 0; c <= po::OUTSIDE; ++c) {
        const int s = __syncthreads_count(what == c);
        if (threadIdx.x == 0 && s) atomicAdd(reinterpret_cast<u64*>(counters) + c, (u64)s);
    }
}

__global__ __launch_bounds__(SS_BLOCK) void po_density_kernel(const float* __restrict__ xyz, const float* __restrict__ normals, long long n, PoGrid g,
                                                              u64* __restrict__ acc, long long* counters) {
    const long long i = gid();
    int what = -1;
    if (i < n) {
        po::Cell c;
        what = po::classify(xyz + 3 * i, normals + 3 * i, g.o, g.h, g.g, &c);
        if (what == po::SPLATTED)
            for (int code = 0; code < 8; ++code) {
                const long long t = po::density_term(po::corner_weight(c, code));
                if (t) atomicAdd(acc + po::corner_voxel(c, code, g.g), (u64)t);
            }
    }
    po_count(what, counters);
}

__global__ __launch_bounds__(SS_BLOCK) void po_density_plane_kernel(const long long* __restrict__ acc, long long voxels, float* __restrict__ W) {
    const long long v = gid();
    if (v < voxels) W[v] = po::plane_of(acc[v]);
}

__global__ __launch_bounds__(SS_BLOCK) void po_normal_kernel(const float* __restrict__ xyz, const float* __restrict__ normals, const unsigned char* __restrict__ rgb,
                                                             long long n, int density_weight, PoGrid g, long long voxels, const float* __restrict__ W,
                                                             u64* __restrict__ acc, double* __restrict__ point) {
    const long long i = gid();
    if (i >= n) return;
    po::Cell c;
    if (po::classify(xyz + 3 * i, normals + 3 * i, g.o, g.h, g.g, &c) != po::SPLATTED) {
        point[2 * i] = 0.0;
        point[2 * i + 1] = 0.0;
        return;
    }
    double w[8], wp = 0.0;
    long long vox[8];
    for (int code = 0; code < 8; ++code) {
        w[code] = po::corner_weight(c, code);
        vox[code] = po::corner_voxel(c, code, g.g);
        wp = wp + w[code] * (double)W[vox[code]];
    }
    const double s = po::scale_of(wp, density_weight != 0);
    point[2 * i] = s;
    point[2 * i + 1] = wp;
    for (int a = 0; a < 3; ++a) {
        const double nc = po::unit_component(normals + 3 * i, a);
        for (int code = 0; code < 8; ++code) {
            const long long t = po::normal_term(s, w[code], nc);
            if (t) atomicAdd(acc + (1 + a) * voxels + vox[code], (u64)t);
        }
    }
    if (rgb)
        for (int a = 0; a < 3; ++a) {
            const unsigned char byte = rgb[3 * i + a];
            for (int code = 0; code < 8; ++code) {
                const long long t = po::colour_term(w[code], byte);
                if (t) atomicAdd(acc + (4 + a) * voxels + vox[code], (u64)t);
            }
        }
}

__global__ __launch_bounds__(SS_BLOCK) void po_planes_kernel(const long long* __restrict__ acc, long long voxels, int colour, float* __restrict__ Vx,
                                                             float* __restrict__ Vy, float* __restrict__ Vz, float* __restrict__ Cr, float* __restrict__ Cg,
                                                             float* __restrict__ Cb) {
    const long long v = gid();
    if (v >= voxels) return;
    Vx[v] = po::plane_of(acc[voxels + v]);
    Vy[v] = po::plane_of(acc[2 * voxels + v]);
    Vz[v] = po::plane_of(acc[3 * voxels + v]);
    if (colour) {
        const long long wa = acc[v];
        Cr[v] = po::colour_of(acc[4 * voxels + v], wa);
        Cg[v] = po::colour_of(acc[5 * voxels + v], wa);
        Cb[v] = po::colour_of(acc[6 * voxels + v], wa);
    }
}

// ---- the grid kernels ---------------------------------------------------------------------------------------------------------------
struct PoVoxel { int i, j, k; };

__device__ inline PoVoxel po_voxel(long long v, const PoDims& d) {
    PoVoxel p;
    p.i = (int)(v % d.g[0]);
    const long long r = v / d.g[0];
    p.j = (int)(r % d.g[1]);
    p.k = (int)(r / d.g[1]);
    return p;
}

__global__ __launch_bounds__(SS_BLOCK) void po_rhs_kernel(const float* __restrict__ Vx, const float* __restrict__ Vy, const float* __restrict__ Vz, PoDims d,
                                                          long long voxels, double h, float* __restrict__ b) {
    const long long v = gid();
    if (v >= voxels) return;
    const PoVoxel p = po_voxel(v, d);
    const long long sy = d.g[0], sz = (long long)d.g[0] * d.g[1];
    const double xm = p.i > 0 ? (double)Vx[v - 1] : 0.0, xp = p.i < d.g[0] - 1 ? (double)Vx[v + 1] : 0.0;
    const double ym = p.j > 0 ? (double)Vy[v - sy] : 0.0, yp = p.j < d.g[1] - 1 ? (double)Vy[v + sy] : 0.0;
    const double zm = p.k > 0 ? (double)Vz[v - sz] : 0.0, zp = p.k < d.g[2] - 1 ? (double)Vz[v + sz] : 0.0;
    b[v] = (float)po::rhs(xm, xp, ym, yp, zm, zp, h);
}

// the six neighbours of voxel v = (i, j, k), the ghost MINUS the cell itself
__device__ inline double po_six(const float* __restrict__ x, long long v, const PoVoxel& p, const PoDims& d, double c) {
    const long long sy = d.g[0], sz = (long long)d.g[0] * d.g[1];
    const double xm = p.i > 0 ? (double)x[v - 1] : -c, xp = p.i < d.g[0] - 1 ? (double)x[v + 1] : -c;
    const double ym = p.j > 0 ? (double)x[v - sy] : -c, yp = p.j < d.g[1] - 1 ? (double)x[v + sy] : -c;
    const double zm = p.k > 0 ? (double)x[v - sz] : -c, zp = p.k < d.g[2] - 1 ? (double)x[v + sz] : -c;
    return po::six(xm, xp, ym, yp, zm, zp);
}

__global__ __launch_bounds__(SS_BLOCK) void po_sweep_kernel(const float* __restrict__ x, const float* __restrict__ b, PoDims d, long long voxels, double h2,
                                                            float* __restrict__ y) {
    const long long v = gid();
    if (v >= voxels) return;
    const PoVoxel p = po_voxel(v, d);
    const double c = (double)x[v];
    y[v] = (float)po::jacobi(c, po_six(x, v, p, d, c), (double)b[v], h2);
}

__device__ inline double po_residual(const float* __restrict__ x, const float* __restrict__ b, long long v, const PoVoxel& p, const PoDims& d, double h2) {
    const double c = (double)x[v];
    return po::residual(c, po_six(x, v, p, d, c), (double)b[v], h2);
}

// d: the FINE dims (all even); one thread per coarse cell
__global__ __launch_bounds__(SS_BLOCK) void po_restrict_kernel(const float* __restrict__ x, const float* __restrict__ b, PoDims d, PoDims dc, long long coarse_voxels,
                                                               double h2, float* __restrict__ bc) {
    const long long v = gid();
    if (v >= coarse_voxels) return;
    const PoVoxel q = po_voxel(v, dc);
    double s = 0.0;
    for (int code = 0; code < 8; ++code) {
        PoVoxel p;
        p.i = 2 * q.i + (code & 1);
        p.j = 2 * q.j + ((code >> 1) & 1);
        p.k = 2 * q.k + (code >> 2);
        const long long f = (long long)p.i + (long long)d.g[0] * ((long long)p.j + (long long)d.g[1] * p.k);
        s = s + po_residual(x, b, f, p, d, h2);
    }
    bc[v] = (float)(0.125 * s);
}

// d: the FINE dims; e: the coarse correction
__global__ __launch_bounds__(SS_BLOCK) void po_prolong_kernel(const float* __restrict__ e, PoDims d, PoDims dc, long long voxels, float* __restrict__ x) {
    const long long v = gid();
    if (v >= voxels) return;
    const PoVoxel p = po_voxel(v, d);
    const int fine[3] = {p.i, p.j, p.k};
    int par[3], nb[3];                                           // the parent and the neighbour per axis; nb = -1: the ghost
    for (int a = 0; a < 3; ++a) {
        par[a] = fine[a] >> 1;
        nb[a] = (fine[a] & 1) ? par[a] + 1 : par[a] - 1;
        if (nb[a] >= dc.g[a]) nb[a] = -1;
    }
    const long long sy = dc.g[0], sz = (long long)dc.g[0] * dc.g[1];
    double ez[2];
    for (int kz = 0; kz < 2; ++kz) {                              // kz, ky = 0: the parent's row; 1: the neighbour's
        const int K = kz ? nb[2] : par[2];
        if (K < 0) { ez[1] = -ez[0]; continue; }
        double ey[2];
        for (int ky = 0; ky < 2; ++ky) {
            const int J = ky ? nb[1] : par[1];
            if (J < 0) { ey[1] = -ey[0]; continue; }
            const long long row = sy * J + sz * K;
            const double c = (double)e[row + par[0]];
            const double m = nb[0] < 0 ? -c : (double)e[row + nb[0]];
            ey[ky] = po::prolong_axis(c, m);
        }
        ez[kz] = po::prolong_axis(ey[0], ey[1]);
    }
    x[v] = (float)((double)x[v] + po::prolong_axis(ez[0], ez[1]));
}

// part[block] = max |residual| over the voxels the block strides over
__global__ __launch_bounds__(SS_BLOCK) void po_norm_kernel(const float* __restrict__ x, const float* __restrict__ b, PoDims d, long long voxels, double h2,
                                                           double* __restrict__ part) {
    __shared__ double sh[SS_BLOCK];
    double m = 0.0;
    for (long long v = gid(); v < voxels; v += (long long)gridDim.x * SS_BLOCK) m = fmax(m, fabs(po_residual(x, b, v, po_voxel(v, d), d, h2)));
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = SS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(SS_BLOCK) void po_norm_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    __shared__ double sh[SS_BLOCK];
    double m = 0.0;
    for (int q = threadIdx.x; q < nparts; q += SS_BLOCK) m = fmax(m, part[q]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = SS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// ---- the isovalue -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void po_terms_kernel(const float* __restrict__ xyz, const double* __restrict__ point, long long n, const float* __restrict__ chi,
                                                            PoGrid g, double* __restrict__ terms) {
    const long long i = gid();
    if (i >= n) return;
    const double s = point[2 * i];
    po::Cell c;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    if (s > 0.0 && po::cell_of(xyz + 3 * i, g.o, g.h, g.g, &c)) {
        double xp = 0.0;
        for (int code = 0; code < 8; ++code) xp = xp + po::corner_weight(c, code) * (double)chi[po::corner_voxel(c, code, g.g)];
        t[0] = s * xp;
        t[1] = s;
        t[2] = point[2 * i + 1];
        t[3] = 1.0;
    }
    for (int q = 0; q < 4; ++q) terms[q * n + i] = t[q];
}

// rcmvs_pc_moments' tree over the four planes of terms, and the minimum of plane 2 where plane 3 is set: part[q * PO_TREE + block]
__global__ __launch_bounds__(SS_BLOCK) void po_tree_kernel(const double* __restrict__ terms, long long n, double* __restrict__ part) {
    __shared__ double sh[SS_BLOCK];
    const long long lane = gid(), lanes = (long long)PO_TREE * SS_BLOCK;
    for (int q = 0; q < 5; ++q) {
        double s = q < 4 ? 0.0 : (double)INFINITY;
        if (q < 4)
            for (long long i = lane; i < n; i += lanes) s = s + terms[q * n + i];
        else
            for (long long i = lane; i < n; i += lanes)
                if (terms[3 * n + i] != 0.0) s = fmin(s, terms[2 * n + i]);
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = SS_BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] = q < 4 ? sh[threadIdx.x] + sh[threadIdx.x + o] : fmin(sh[threadIdx.x], sh[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[q * PO_TREE + blockIdx.x] = sh[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void po_iso_final_kernel(const double* __restrict__ part, double* __restrict__ stats) {
    __shared__ double r[5];
    if (threadIdx.x < 5) {
        const int q = threadIdx.x;
        double s = q < 4 ? 0.0 : (double)INFINITY;
        for (int b = 0; b < PO_TREE; ++b) s = q < 4 ? s + part[q * PO_TREE + b] : fmin(s, part[q * PO_TREE + b]);
        r[q] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] = r[1] > 0.0 ? r[0] / r[1] : 0.0;
        stats[1] = r[0];
        stats[2] = r[1];
        stats[3] = r[2];
        stats[4] = r[3];
        stats[5] = r[3] > 0.0 ? r[2] / r[3] : 0.0;
        stats[6] = r[4];
        stats[7] = 0.0;
    }
}

// ---- the field ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void po_field_kernel(const float* __restrict__ chi, const float* __restrict__ W, const double* __restrict__ stats, double trim,
                                                            PoDims d, long long voxels, float* __restrict__ dsum, float* __restrict__ wsum, long long* trimmed) {
    const long long v = gid();
    bool cut = false;
    if (v < voxels) {
        const PoVoxel p = po_voxel(v, d);
        float m = 0.0f;
        for (int dz = -1; dz <= 1; ++dz) {
            const int z = p.k + dz;
            if (z < 0 || z >= d.g[2]) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int y = p.j + dy;
                if (y < 0 || y >= d.g[1]) continue;
                const long long row = (long long)d.g[0] * ((long long)y + (long long)d.g[1] * z);
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = p.i + dx;
                    if (x < 0 || x >= d.g[0]) continue;
                    m = fmaxf(m, W[row + x]);
                }
            }
        }
        const float w = po::field_weight(m, trim);
        dsum[v] = po::field_value(chi[v], stats[0]);
        wsum[v] = w;
        cut = w == 0.0f;
    }
    const int s = __syncthreads_count(cut);
    if (threadIdx.x == 0 && s) atomicAdd(reinterpret_cast<u64*>(trimmed), (u64)s);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static int po_aligned(const char* what, const char* name, const void* p, int bytes) {
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0, "%s: %s must be %d-byte aligned", what, name, bytes);
    return 0;
}

static int po_dims(const char* what, const int* dims_host, PoDims* d, long long* voxels) {
    RCMVS_REQUIRE(dims_host, "%s: null pointer (dims_host)", what);
    for (int a = 0; a < 3; ++a) d->g[a] = dims_host[a];
    RCMVS_REQUIRE(d->g[0] >= 1 && d->g[1] >= 1 && d->g[2] >= 1 && (long long)d->g[0] * d->g[1] * d->g[2] <= RCMVS_PO_MAX_VOXELS,
                  "%s: dims_host = %d x %d x %d (every side >= 1, at most 2^27 voxels)", what, d->g[0], d->g[1], d->g[2]);
    *voxels = (long long)d->g[0] * d->g[1] * d->g[2];
    return 0;
}

static int po_grid(const char* what, const double* grid_host, const int* dims_host, PoGrid* g, long long* voxels) {
    RCMVS_REQUIRE(grid_host, "%s: null pointer (grid_host)", what);
    PoDims d;
    if (int rc = po_dims(what, dims_host, &d, voxels)) return rc;
    for (int a = 0; a < 3; ++a) { g->o[a] = grid_host[a]; g->g[a] = d.g[a]; }
    g->h = grid_host[3];
    RCMVS_REQUIRE(g->h > 0.0 && std::isfinite(g->h) && std::isfinite(g->o[0]) && std::isfinite(g->o[1]) && std::isfinite(g->o[2]),
                  "%s: grid_host = {%g, %g, %g, %g} (a finite origin and a finite voxel edge h > 0)", what, g->o[0], g->o[1], g->o[2], g->h);
    return 0;
}

static int po_n(const char* what, long long n) {
    RCMVS_REQUIRE(n >= 0 && n < (1ll << 31), "%s: n = %lld points (0 .. 2^31-1)", what, n);
    return 0;
}

// the levels of the grid: dims[l] and the voxels of each; -> their number
static int po_levels(const PoDims& d, PoDims* dims, long long* voxels) {
    int L = 1;
    dims[0] = d;
    voxels[0] = (long long)d.g[0] * d.g[1] * d.g[2];
    while (L < RCMVS_PO_MAX_LEVELS) {
        const PoDims& f = dims[L - 1];
        if ((f.g[0] | f.g[1] | f.g[2]) & 1) break;
        if (f.g[0] / 2 < 4 || f.g[1] / 2 < 4 || f.g[2] / 2 < 4) break;
        for (int a = 0; a < 3; ++a) dims[L].g[a] = f.g[a] / 2;
        voxels[L] = (long long)dims[L].g[0] * dims[L].g[1] * dims[L].g[2];
        ++L;
    }
    return L;
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_po_splat_timed(const float* xyz, const float* normals, const unsigned char* rgb, long long n, int density_weight, const double* grid_host,
                                    const int* dims_host, long long* acc, float* W, float* Vx, float* Vy, float* Vz, float* Cr, float* Cg, float* Cb, double* point,
                                    long long* counters, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "po_splat";
    if (int rc = po_n(what, n)) return rc;
    RCMVS_REQUIRE(density_weight == 0 || density_weight == 1, "%s: density_weight = %d (0 or 1)", what, density_weight);
    RCMVS_REQUIRE(phase == RCMVS_PO_PHASE_ALL || phase == RCMVS_PO_PHASE_DENSITY || phase == RCMVS_PO_PHASE_NORMAL, "%s: phase = %d (0: all, 1: density, 2: normal)", what, phase);
    PoGrid g;
    long long voxels;
    if (int rc = po_grid(what, grid_host, dims_host, &g, &voxels)) return rc;
    RCMVS_REQUIRE(acc && W && Vx && Vy && Vz && counters, "%s: null pointer (acc, W, Vx, Vy, Vz, counters)", what);
    RCMVS_REQUIRE(n == 0 || (xyz && normals && point), "%s: null pointer (xyz, normals and point hold n rows)", what);
    const bool colour = rgb != nullptr;
    RCMVS_REQUIRE((Cr != nullptr) == (Cg != nullptr) && (Cg != nullptr) == (Cb != nullptr) && (n == 0 || colour == (Cr != nullptr)),
                  "%s: rgb and the three colour planes come together", what);
    const int planes = Cr ? RCMVS_PO_ACC : 4;
    if (int rc = po_aligned(what, "xyz", xyz, 4)) return rc;
    if (int rc = po_aligned(what, "normals", normals, 4)) return rc;
    if (int rc = po_aligned(what, "acc", acc, 8)) return rc;
    if (int rc = po_aligned(what, "point", point, 8)) return rc;
    if (int rc = po_aligned(what, "counters", counters, 8)) return rc;
    {
        const void* fp[] = {W, Vx, Vy, Vz, Cr, Cg, Cb};
        for (const void* p : fp)
            if (int rc = po_aligned(what, "a plane", p, 4)) return rc;
        const size_t pl = (size_t)voxels * 4;
        const void* ptr[] = {acc, W, Vx, Vy, Vz, Cr, Cg, Cb, point, counters, xyz, normals, rgb};
        const size_t len[] = {(size_t)voxels * 8 * planes, pl, pl, pl, pl, pl, pl, pl, (size_t)n * 16, (size_t)RCMVS_PO_COUNTERS * 8, (size_t)n * 12, (size_t)n * 12, (size_t)n * 3};
        if (int rc = buffers_overlap(what, ptr, len, 10, 13)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    const bool all = phase == RCMVS_PO_PHASE_ALL, den = phase == RCMVS_PO_PHASE_DENSITY, nor = phase == RCMVS_PO_PHASE_NORMAL;
    u64* a = reinterpret_cast<u64*>(acc);
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(blocks(voxels * planes)), dim3(SS_BLOCK), 0, st, all ? e0 : none, none, a, voxels * planes);
    hipLaunchKernelGGL(zero_kernel<u64>, dim3(1), dim3(SS_BLOCK), 0, st, reinterpret_cast<u64*>(counters), (long long)RCMVS_PO_COUNTERS);
    RCMVS_LAUNCH_TIMED(po_density_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, den ? e0 : none, den ? e1 : none, xyz, normals, n, g, a, counters);
    hipLaunchKernelGGL(po_density_plane_kernel, dim3(blocks(voxels)), dim3(SS_BLOCK), 0, st, acc, voxels, W);
    RCMVS_LAUNCH_TIMED(po_normal_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, nor ? e0 : none, nor ? e1 : none, xyz, normals, rgb, n, density_weight, g, voxels, W, a,
                       point);
    RCMVS_LAUNCH_TIMED(po_planes_kernel, dim3(blocks(voxels)), dim3(SS_BLOCK), 0, st, none, all ? e1 : none, acc, voxels, Cr ? 1 : 0, Vx, Vy, Vz, Cr, Cg, Cb);
    return launch_status(what);
}

extern "C" int rcmvs_po_splat(const float* xyz, const float* normals, const unsigned char* rgb, long long n, int density_weight, const double* grid_host,
                              const int* dims_host, long long* acc, float* W, float* Vx, float* Vy, float* Vz, float* Cr, float* Cg, float* Cb, double* point,
                              long long* counters, void* stream) {
    return rcmvs_po_splat_timed(xyz, normals, rgb, n, density_weight, grid_host, dims_host, acc, W, Vx, Vy, Vz, Cr, Cg, Cb, point, counters, RCMVS_PO_PHASE_ALL, nullptr,
                                nullptr, stream);
}

extern "C" int rcmvs_po_rhs_timed(const float* Vx, const float* Vy, const float* Vz, const double* grid_host, const int* dims_host, float* b, int phase, void* ev0,
                                  void* ev1, void* stream) {
    const char* what = "po_rhs";
    RCMVS_REQUIRE(phase == RCMVS_PO_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    PoGrid g;
    long long voxels;
    if (int rc = po_grid(what, grid_host, dims_host, &g, &voxels)) return rc;
    RCMVS_REQUIRE(Vx && Vy && Vz && b, "%s: null pointer (Vx, Vy, Vz, b)", what);
    {
        const void* ptr[] = {b, Vx, Vy, Vz};
        for (const void* p : ptr)
            if (int rc = po_aligned(what, "a plane", p, 4)) return rc;
        const size_t pl = (size_t)voxels * 4;
        const size_t len[] = {pl, pl, pl, pl};
        if (int rc = buffers_overlap(what, ptr, len, 1, 4)) return rc;
    }
    PoDims d = {{g.g[0], g.g[1], g.g[2]}};
    RCMVS_LAUNCH_TIMED(po_rhs_kernel, dim3(blocks(voxels)), dim3(SS_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1), Vx, Vy, Vz,
                       d, voxels, g.h, b);
    return launch_status(what);
}

extern "C" int rcmvs_po_rhs(const float* Vx, const float* Vy, const float* Vz, const double* grid_host, const int* dims_host, float* b, void* stream) {
    return rcmvs_po_rhs_timed(Vx, Vy, Vz, grid_host, dims_host, b, RCMVS_PO_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_po_solve_timed(float* x, float* tmp, const float* b, float* coarse, const double* grid_host, const int* dims_host, int cycles, double* part,
                                    double* resid, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "po_solve";
    RCMVS_REQUIRE(cycles >= 0 && cycles <= RCMVS_PO_MAX_CYCLES, "%s: cycles = %d (0 .. %d)", what, cycles, RCMVS_PO_MAX_CYCLES);
    RCMVS_REQUIRE(phase >= RCMVS_PO_PHASE_ALL && phase <= RCMVS_PO_PHASE_PROLONG, "%s: phase = %d (0: all, 1: sweep, 2: restrict, 3: prolong)", what, phase);
    PoGrid g;
    long long voxels;
    if (int rc = po_grid(what, grid_host, dims_host, &g, &voxels)) return rc;
    PoDims dims[RCMVS_PO_MAX_LEVELS];
    long long nvox[RCMVS_PO_MAX_LEVELS], below = 0;
    const int L = po_levels(PoDims{{g.g[0], g.g[1], g.g[2]}}, dims, nvox);
    for (int l = 1; l < L; ++l) below += nvox[l];
    const bool timed = ev0 || ev1;
    RCMVS_REQUIRE(!timed || (cycles >= 1 && (L > 1 || phase <= RCMVS_PO_PHASE_SWEEP)), "%s: nothing of phase %d runs (%d cycles, %d levels)", what, phase, cycles, L);
    RCMVS_REQUIRE(x && tmp && b && part, "%s: null pointer (x, tmp, b, part)", what);
    RCMVS_REQUIRE(L == 1 || coarse, "%s: null pointer (coarse holds 3 x %lld floats)", what, below);
    RCMVS_REQUIRE(cycles == 0 || resid, "%s: null pointer (resid holds %d doubles)", what, cycles);
    if (int rc = po_aligned(what, "x", x, 4)) return rc;
    if (int rc = po_aligned(what, "tmp", tmp, 4)) return rc;
    if (int rc = po_aligned(what, "b", b, 4)) return rc;
    if (int rc = po_aligned(what, "coarse", coarse, 4)) return rc;
    if (int rc = po_aligned(what, "part", part, 8)) return rc;
    if (int rc = po_aligned(what, "resid", resid, 8)) return rc;
    {
        const void* ptr[] = {x, tmp, coarse, part, resid, b};
        const size_t len[] = {(size_t)voxels * 4, (size_t)voxels * 4, (size_t)below * 12, (size_t)RCMVS_PO_PART * 8, (size_t)cycles * 8, (size_t)voxels * 4};
        if (int rc = buffers_overlap(what, ptr, len, 5, 6)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    float* lx[RCMVS_PO_MAX_LEVELS];
    float* lt[RCMVS_PO_MAX_LEVELS];
    const float* lb[RCMVS_PO_MAX_LEVELS];
    double h2[RCMVS_PO_MAX_LEVELS];
    lx[0] = x; lt[0] = tmp; lb[0] = b;
    {
        float* p = coarse;
        double h = g.h;
        h2[0] = h * h;
        for (int l = 1; l < L; ++l) {
            lx[l] = p; lt[l] = p + nvox[l]; lb[l] = p + 2 * nvox[l];
            p += 3 * nvox[l];
            h = 2.0 * h;
            h2[l] = h * h;
        }
    }
    bool first = true;                                           // nothing launched yet: ALL's start
    int pending = phase;                                         // the phase whose first fine launch is still to come
    // the events of one launch: kind = a phase > 0 at the fine level, else 0; last = the solve's last launch
    auto events = [&](int kind, bool last, hipEvent_t* a, hipEvent_t* z) {
        *a = none; *z = none;
        if (phase == RCMVS_PO_PHASE_ALL) { if (first) *a = e0; if (last) *z = e1; }
        else if (kind == pending) { *a = e0; *z = e1; pending = -1; }
        first = false;
    };
    auto sweeps = [&](int l, int count) {
        for (int s = 0; s < count; ++s) {
            hipEvent_t a, z;
            events(l == 0 ? RCMVS_PO_PHASE_SWEEP : 0, false, &a, &z);
            const float* src = (s & 1) ? lt[l] : lx[l];
            float* dst = (s & 1) ? lx[l] : lt[l];
            RCMVS_LAUNCH_TIMED(po_sweep_kernel, dim3(blocks(nvox[l])), dim3(SS_BLOCK), 0, st, a, z, src, lb[l], dims[l], nvox[l], h2[l], dst);
        }
    };
    const int nparts = (int)(blocks(voxels) < (unsigned)RCMVS_PO_PART ? blocks(voxels) : (unsigned)RCMVS_PO_PART);
    for (int c = 0; c < cycles; ++c) {
        hipEvent_t a, z;
        for (int l = 0; l + 1 < L; ++l) {
            if (l > 0) { events(0, false, &a, &z); RCMVS_LAUNCH_TIMED(zero_kernel<int>, dim3(blocks(nvox[l])), dim3(SS_BLOCK), 0, st, a, z, reinterpret_cast<int*>(lx[l]), nvox[l]); }
            sweeps(l, 2);
            events(l == 0 ? RCMVS_PO_PHASE_RESTRICT : 0, false, &a, &z);
            RCMVS_LAUNCH_TIMED(po_restrict_kernel, dim3(blocks(nvox[l + 1])), dim3(SS_BLOCK), 0, st, a, z, lx[l], lb[l], dims[l], dims[l + 1], nvox[l + 1], h2[l],
                               const_cast<float*>(lb[l + 1]));
        }
        if (L > 1) { events(0, false, &a, &z); RCMVS_LAUNCH_TIMED(zero_kernel<int>, dim3(blocks(nvox[L - 1])), dim3(SS_BLOCK), 0, st, a, z, reinterpret_cast<int*>(lx[L - 1]), nvox[L - 1]); }
        sweeps(L - 1, RCMVS_PO_COARSEST_SWEEPS);
        for (int l = L - 2; l >= 0; --l) {
            events(l == 0 ? RCMVS_PO_PHASE_PROLONG : 0, false, &a, &z);
            RCMVS_LAUNCH_TIMED(po_prolong_kernel, dim3(blocks(nvox[l])), dim3(SS_BLOCK), 0, st, a, z, lx[l + 1], dims[l], dims[l + 1], nvox[l], lx[l]);
            sweeps(l, 2);
        }
        events(0, false, &a, &z);
        RCMVS_LAUNCH_TIMED(po_norm_kernel, dim3(nparts), dim3(SS_BLOCK), 0, st, a, z, x, b, dims[0], voxels, h2[0], part);
        events(0, c == cycles - 1, &a, &z);
        RCMVS_LAUNCH_TIMED(po_norm_final_kernel, dim3(1), dim3(SS_BLOCK), 0, st, a, z, part, nparts, resid + c);
    }
    return launch_status(what);
}

extern "C" int rcmvs_po_solve(float* x, float* tmp, const float* b, float* coarse, const double* grid_host, const int* dims_host, int cycles, double* part,
                              double* resid, void* stream) {
    return rcmvs_po_solve_timed(x, tmp, b, coarse, grid_host, dims_host, cycles, part, resid, RCMVS_PO_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_po_iso_timed(const float* xyz, const double* point, long long n, const float* chi, const double* grid_host, const int* dims_host, double* terms,
                                  double* part, double* stats, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "po_iso";
    if (int rc = po_n(what, n)) return rc;
    RCMVS_REQUIRE(phase == RCMVS_PO_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    PoGrid g;
    long long voxels;
    if (int rc = po_grid(what, grid_host, dims_host, &g, &voxels)) return rc;
    RCMVS_REQUIRE(chi && part && stats, "%s: null pointer (chi, part, stats)", what);
    RCMVS_REQUIRE(n == 0 || (xyz && point && terms), "%s: null pointer (xyz, point and terms hold n rows)", what);
    if (int rc = po_aligned(what, "xyz", xyz, 4)) return rc;
    if (int rc = po_aligned(what, "chi", chi, 4)) return rc;
    if (int rc = po_aligned(what, "point", point, 8)) return rc;
    if (int rc = po_aligned(what, "terms", terms, 8)) return rc;
    if (int rc = po_aligned(what, "part", part, 8)) return rc;
    if (int rc = po_aligned(what, "stats", stats, 8)) return rc;
    {
        const void* ptr[] = {terms, part, stats, xyz, point, chi};
        const size_t len[] = {(size_t)n * 32, (size_t)5 * PO_TREE * 8, (size_t)RCMVS_PO_STATS * 8, (size_t)n * 12, (size_t)n * 16, (size_t)voxels * 4};
        if (int rc = buffers_overlap(what, ptr, len, 3, 6)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(po_terms_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, e0, none, xyz, point, n, chi, g, terms);
    hipLaunchKernelGGL(po_tree_kernel, dim3(PO_TREE), dim3(SS_BLOCK), 0, st, terms, n, part);
    RCMVS_LAUNCH_TIMED(po_iso_final_kernel, dim3(1), dim3(64), 0, st, none, e1, part, stats);
    return launch_status(what);
}

extern "C" int rcmvs_po_iso(const float* xyz, const double* point, long long n, const float* chi, const double* grid_host, const int* dims_host, double* terms,
                            double* part, double* stats, void* stream) {
    return rcmvs_po_iso_timed(xyz, point, n, chi, grid_host, dims_host, terms, part, stats, RCMVS_PO_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_po_field_timed(const float* chi, const float* W, const double* stats, double trim, const int* dims_host, float* dsum, float* wsum,
                                    long long* trimmed, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "po_field";
    RCMVS_REQUIRE(phase == RCMVS_PO_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    RCMVS_REQUIRE(trim >= 0.0 && std::isfinite(trim), "%s: trim = %g (finite and >= 0)", what, trim);
    PoDims d;
    long long voxels;
    if (int rc = po_dims(what, dims_host, &d, &voxels)) return rc;
    RCMVS_REQUIRE(chi && W && stats && dsum && wsum && trimmed, "%s: null pointer (chi, W, stats, dsum, wsum, trimmed)", what);
    if (int rc = po_aligned(what, "stats", stats, 8)) return rc;
    if (int rc = po_aligned(what, "trimmed", trimmed, 8)) return rc;
    {
        const void* ptr[] = {dsum, wsum, trimmed, chi, W, stats};
        for (int q = 0; q < 5; ++q)
            if (q != 2)
                if (int rc = po_aligned(what, "a plane", ptr[q], 4)) return rc;
        const size_t pl = (size_t)voxels * 4;
        const size_t len[] = {pl, pl, 8, pl, pl, (size_t)RCMVS_PO_STATS * 8};
        if (int rc = buffers_overlap(what, ptr, len, 3, 6)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(SS_BLOCK), 0, st, e0, none, reinterpret_cast<u64*>(trimmed), 1ll);
    RCMVS_LAUNCH_TIMED(po_field_kernel, dim3(blocks(voxels)), dim3(SS_BLOCK), 0, st, none, e1, chi, W, stats, trim, d, voxels, dsum, wsum, trimmed);
    return launch_status(what);
}

extern "C" int rcmvs_po_field(const float* chi, const float* W, const double* stats, double trim, const int* dims_host, float* dsum, float* wsum, long long* trimmed,
                              void* stream) {
    return rcmvs_po_field_timed(chi, W, stats, trim, dims_host, dsum, wsum, trimmed, RCMVS_PO_PHASE_ALL, nullptr, nullptr, stream);
}
