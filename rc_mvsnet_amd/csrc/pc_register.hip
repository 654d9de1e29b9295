// Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py): the benchmark's python_toolbox/evaluation crops both clouds to a
// polygon prism, voxel-averages them, refines the alignment with ICP and thresholds the two nearest-neighbour distance sets.
// The bounding box, the grid and the capped nearest neighbour are pointcloud.hip's; the passes of its own are kernels here:
//
//   crop      one thread per point: optional 4x4 transform in fp64 (rounded to fp32 once), axis range + even-odd polygon test
//             (pc_register_math.h), per-block counts, pointcloud.hip's scan, ordered compaction of the transformed points.
//   voxel     63-bit voxel keys (kz, ky, kx packed on the lattice's own dims), an LSD radix sort of (key, index) pairs, 8 bits a
//             pass (scan_sort.hip's kernels, shared with mesh_decimate.hip): per-block digit histograms, one scan over the
//             digit-major (digit, block) table, a stable scatter whose in-block rank comes from wave ballots.  Stable
//             passes from index order leave every voxel's points in input order.
//             Segment heads + scan give the voxel count and the output slots; one thread per head then walks its segment and
//             adds in fp64 in that order (a long segment occupies one lane, never a block).  No array over the lattice, no
//             floating-point atomics.
//   icp       one thread per source point: s' = T s in fp64, pointcloud.hip's shell search around s' stopped at max_dist with
//             the lower target index winning ties, then the pair's 18 moments reduced wave -> block -> a fixed number of block
//             partials, finished by a second launch (fixed summation tree: two runs give the same bits).
//   hist      bins floor(d / w) counted in LDS per block, then integer atomics (order-independent).
// gfx950 only; only plain atomics, __syncthreads, ballots and shuffles (tests/emu compiles this file too).
#include <climits>

#include "common.h"
#include "pc_register.h"
#include "pc_register_math.h"
#include "pointcloud_scan.h"                                      // pc_scan
#include "scan_sort.h"                                            // radix_hist_kernel, radix_scatter_kernel

#pragma clang fp contract(off)

namespace rcmvs {

constexpr int PCR_BLOCK = 256;
constexpr int PCR_WAVES = PCR_BLOCK / WAVE;
constexpr int PCR_ICP_BLOCKS = RCMVS_PC_ICP_BLOCKS;
constexpr int PCR_NMOM = RCMVS_PC_ICP_MOMENTS;
constexpr int PCR_HIST_BLOCKS = 1024;
static_assert(PCR_BLOCK == SS_BLOCK, "the radix kernels of scan_sort.h sort blocks of PCR_BLOCK keys");

// ---- transform + crop -----------------------------------------------------------------------------------------------
struct PcrCrop {
    double u[RCMVS_PC_MAX_POLYGON], v[RCMVS_PC_MAX_POLYGON];
    double T[12];
    double amin, amax;
    int axis, m, has_T;
};

__device__ inline bool pcr_crop_point(const PcrCrop& c, const float* __restrict__ pts, long long i, float* q) {
    const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (c.has_T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = (float)pcr::xform(c.T, a, (double)x, (double)y, (double)z);
    } else {
        q[0] = x; q[1] = y; q[2] = z;
    }
    return pcr::in_crop(q[0], q[1], q[2], c.axis, c.amin, c.amax, c.u, c.v, c.m);
}

__global__ __launch_bounds__(PCR_BLOCK) void pcr_crop_count_kernel(PcrCrop c, const float* __restrict__ pts, int n,
                                                                   unsigned char* __restrict__ flags, int* __restrict__ counts) {
    const int i = blockIdx.x * PCR_BLOCK + threadIdx.x;
    bool f = false;
    float q[3];
    if (i < n) { f = pcr_crop_point(c, pts, i, q); flags[i] = f; }
    const int k = __syncthreads_count(f);
    if (threadIdx.x == 0) counts[blockIdx.x] = k;
}

__global__ __launch_bounds__(PCR_BLOCK) void pcr_crop_scatter_kernel(PcrCrop c, const float* __restrict__ pts, int n,
                                                                     const int* __restrict__ offsets, float* __restrict__ out) {
    __shared__ int wave_base[PCR_WAVES];
    const int i = blockIdx.x * PCR_BLOCK + threadIdx.x;
    float q[3] = {0.0f, 0.0f, 0.0f};
    const bool f = i < n && pcr_crop_point(c, pts, i, q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_base[wave] = __popcll(b);
    __syncthreads();
    int base = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wave_base[w];
    if (f) {
        const long long o = (long long)(base + before) * 3;
        out[o + 0] = q[0]; out[o + 1] = q[1]; out[o + 2] = q[2];
    }
}

// ---- voxel down-sample: keys, radix sort, heads, segment means ------------------------------------------------------
struct PcrLattice { double org[3]; double voxel; long long g[3]; };

__global__ __launch_bounds__(PCR_BLOCK) void pcr_voxel_key_kernel(const float* __restrict__ pts, int n, PcrLattice L,
                                                                  unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int i = blockIdx.x * PCR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long kx = pcr::voxel_coord(pts[(long long)i * 3 + 0], L.org[0], L.voxel);
    const long long ky = pcr::voxel_coord(pts[(long long)i * 3 + 1], L.org[1], L.voxel);
    const long long kz = pcr::voxel_coord(pts[(long long)i * 3 + 2], L.org[2], L.voxel);
    key[i] = (unsigned long long)((kz * L.g[1] + ky) * L.g[0] + kx);
    idx[i] = i;
}

__global__ __launch_bounds__(PCR_BLOCK) void pcr_voxel_head_kernel(const unsigned long long* __restrict__ key, int n, int* __restrict__ head) {
    const int i = blockIdx.x * PCR_BLOCK + threadIdx.x;
    if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// one thread per sorted slot; the head of a segment adds its points in fp64 in sorted (= input index) order, divides once
__global__ __launch_bounds__(PCR_BLOCK) void pcr_voxel_emit_kernel(const float* __restrict__ pts, const unsigned long long* __restrict__ key,
                                                                   const int* __restrict__ idx, const int* __restrict__ head_start, int n, int m,
                                                                   float* __restrict__ out) {
    const int i = blockIdx.x * PCR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int slot = head_start[i];
    if (head_start[i + 1] == slot || slot >= m) return;
    const unsigned long long k = key[i];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int j = i;
    for (; j < n && key[j] == k; ++j) {
        const long long p = (long long)idx[j] * 3;
        sx += (double)pts[p + 0]; sy += (double)pts[p + 1]; sz += (double)pts[p + 2];
    }
    const double c = (double)(j - i);
    out[(long long)slot * 3 + 0] = (float)(sx / c);
    out[(long long)slot * 3 + 1] = (float)(sy / c);
    out[(long long)slot * 3 + 2] = (float)(sz / c);
}

// ---- ICP step: nearest neighbour of T s with the lower index winning ties, 18 moments -------------------------------
struct PcrGrid { double o[3]; double h; int g[3]; };
struct PcrXform { double T[12]; };

__device__ inline int pcr_cell_coord(double p, double o, double h, int g) {
    const double c = floor((p - o) / h);
    return c < 0.0 ? 0 : (c >= (double)g ? g - 1 : (int)c);
}

// pointcloud.hip's pc_nn_kernel search for an fp64 query: -> the sorted slot of the nearest target with distance < cap
// (ties: the lower sorted_idx), -1 when there is none; *d2 its squared distance
__device__ inline int pcr_nearest(const double* qd, const PcrGrid& g, const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                  const int* __restrict__ sorted_idx, double cap, double* d2_out) {
    const double slack = 1e-6 * g.h;
    double gap2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = g.o[a], hi = g.o[a] + (double)g.g[a] * g.h;
        const double d = qd[a] < lo ? lo - qd[a] : (qd[a] > hi ? qd[a] - hi : 0.0);
        gap2 += d * d;
    }
    const double gap = sqrt(gap2) - slack;
    if (gap > cap) return -1;
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = pcr_cell_coord(qd[a], g.o[a], g.h, g.g[a]);
    double best2 = INFINITY;
    int best = -1, best_idx = INT_MAX;
    const double cap2 = cap * cap;
    for (int r = 0;; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = c[2] + dz;
            if (z < 0 || z >= g.g[2]) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = c[1] + dy;
                if (y < 0 || y >= g.g[1]) continue;
                const bool face = r == 0 || dz == -r || dz == r || dy == -r || dy == r;
                const int step = face ? 1 : 2 * r;
                for (int dx = -r; dx <= r; dx += step) {
                    const int x = c[0] + dx;
                    if (x < 0 || x >= g.g[0]) continue;
                    const int cc[3] = {x, y, z};
                    double lb2 = 0.0;
                    for (int a = 0; a < 3; ++a) {
                        const double lo = g.o[a] + (double)cc[a] * g.h - slack, hi = g.o[a] + (double)(cc[a] + 1) * g.h + slack;
                        const double d = qd[a] < lo ? lo - qd[a] : (qd[a] > hi ? qd[a] - hi : 0.0);
                        lb2 += d * d;
                    }
                    if (lb2 > best2 || lb2 > cap2) continue;
                    const int k = (z * g.g[1] + y) * g.g[0] + x;
                    const int e = cell_start[k + 1];
                    for (int j = cell_start[k]; j < e; ++j) {
                        const float4 t = sorted[j];
                        const double d2 = pcr::dist2(qd[0], qd[1], qd[2], t.x, t.y, t.z);
                        if (d2 > best2) continue;
                        const int id = sorted_idx[j];
                        if (d2 < best2 || id < best_idx) { best2 = d2; best = j; best_idx = id; }
                    }
                }
            }
        }
        double side = INFINITY;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) side = fmin(side, qd[a] - (g.o[a] + (double)(c[a] - r) * g.h));
            if (c[a] + r < g.g[a] - 1) side = fmin(side, (g.o[a] + (double)(c[a] + r + 1) * g.h) - qd[a]);
        }
        if (side == INFINITY) break;
        const double lb = fmax(side - slack, gap);
        if (lb > 0.0 && (lb * lb > best2 || lb > cap)) break;
    }
    if (best < 0 || !(sqrt(best2) < cap)) return -1;
    *d2_out = best2;
    return best;
}

// part[block * 18 + k]: {count, sum d^2, sum s' (3), sum t (3), sum s'_a t_b (9, a-major), sum |s'|^2} of the block's points
// (thread t takes points t, t + T, ... in that order; lanes halve down by shuffles, then the block's waves in order)
__global__ __launch_bounds__(PCR_BLOCK) void pcr_icp_step_kernel(const float* __restrict__ src, int n, PcrXform X, PcrGrid g,
                                                                 const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                                 const int* __restrict__ sorted_idx, double max_dist, int* __restrict__ corr,
                                                                 double* __restrict__ part) {
    __shared__ double sh[PCR_WAVES][PCR_NMOM];
    double acc[PCR_NMOM];
#pragma unroll
    for (int k = 0; k < PCR_NMOM; ++k) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * PCR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PCR_BLOCK) {
        const double x = (double)src[i * 3 + 0], y = (double)src[i * 3 + 1], z = (double)src[i * 3 + 2];
        double s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = pcr::xform(X.T, a, x, y, z);
        double d2 = 0.0;
        const int j = pcr_nearest(s, g, cell_start, sorted, sorted_idx, max_dist, &d2);
        if (corr) corr[i] = j >= 0 ? sorted_idx[j] : -1;
        if (j < 0) continue;
        const float4 t4 = sorted[j];
        const double t[3] = {(double)t4.x, (double)t4.y, (double)t4.z};
        acc[0] += 1.0;
        acc[1] += d2;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[2 + a] += s[a];
            acc[5 + a] += t[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += s[a] * t[b];
        }
        acc[17] += (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PCR_NMOM; ++k) {
        double v = acc[k];
        for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < PCR_NMOM) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < PCR_WAVES; ++w) v += sh[w][threadIdx.x];
        part[(long long)blockIdx.x * PCR_NMOM + threadIdx.x] = v;
    }
}

// block k sums moment k over the partials: thread t takes blocks t, t + 256, ..., then the block halves down
__global__ __launch_bounds__(PCR_BLOCK) void pcr_icp_final_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    __shared__ double sh[PCR_BLOCK];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += PCR_BLOCK) s += part[(long long)b * PCR_NMOM + k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = PCR_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = sh[0];
}

// ---- thresholded histogram ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PCR_BLOCK) void pcr_dist_hist_kernel(const double* __restrict__ d, int n, double tau, int nbins, double w,
                                                                  unsigned long long* __restrict__ counts, unsigned long long* __restrict__ below) {
    __shared__ unsigned int bins[RCMVS_PC_HIST_MAX_BINS + 1];     // the last one counts d < tau
    for (int b = threadIdx.x; b <= nbins; b += PCR_BLOCK) bins[b] = 0u;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * PCR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PCR_BLOCK) {
        const double v = d[i];
        const double b = pcr::hist_bin(v, w);
        if (b >= 0.0 && b < (double)nbins) atomicAdd(&bins[(int)b], 1u);
        if (v < tau) atomicAdd(&bins[nbins], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= nbins; b += PCR_BLOCK) {
        const unsigned int c = bins[b];
        if (c) atomicAdd(b < nbins ? &counts[b] : below, (unsigned long long)c);
    }
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_pc_crop(const float* pts, long long n, const double* transform_host, int axis, double axis_min, double axis_max,
                             const double* polygon_host, int m, unsigned char* flags, float* kept, int* work, void* stream) {
    RCMVS_REQUIRE(pts && polygon_host && flags && kept && work, "pc_crop: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_crop: n=%lld (1 .. 2^31-1)", n);
    RCMVS_REQUIRE(axis >= 0 && axis <= 2, "pc_crop: orthogonal axis %d (0, 1 or 2)", axis);
    RCMVS_REQUIRE(m >= 3 && m <= RCMVS_PC_MAX_POLYGON, "pc_crop: polygon of %d vertices (3 .. %d)", m, RCMVS_PC_MAX_POLYGON);
    RCMVS_REQUIRE(std::isfinite(axis_min) && std::isfinite(axis_max), "pc_crop: axis range %g .. %g", axis_min, axis_max);
    PcrCrop c = {};
    for (int i = 0; i < m; ++i) {
        c.u[i] = polygon_host[2 * i + 0];
        c.v[i] = polygon_host[2 * i + 1];
        RCMVS_REQUIRE(std::isfinite(c.u[i]) && std::isfinite(c.v[i]), "pc_crop: polygon vertex %d is not finite", i);
    }
    if (transform_host)
        for (int k = 0; k < 12; ++k) {
            c.T[k] = transform_host[k];
            RCMVS_REQUIRE(std::isfinite(c.T[k]), "pc_crop: transform entry %d is not finite", k);
        }
    c.amin = axis_min; c.amax = axis_max; c.axis = axis; c.m = m; c.has_T = transform_host ? 1 : 0;
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(n, PCR_BLOCK);
    int* counts = work;
    int* offsets = work + nblk;
    int* bsum = offsets + nblk + 1;
    hipLaunchKernelGGL(pcr_crop_count_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, c, pts, (int)n, flags, counts);
    pc_scan(counts, nblk, bsum, offsets, st);
    hipLaunchKernelGGL(pcr_crop_scatter_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, c, pts, (int)n, offsets, kept);
    return launch_status("pc_crop");
}

extern "C" int rcmvs_pc_voxel_sort(const float* pts, long long n, const double* lattice_host, const long long* dims_host,
                                   unsigned long long* key_a, int* idx_a, unsigned long long* key_b, int* idx_b, int* hist, int* hist_start,
                                   int* scan_work, int* head, int* head_start, void* stream) {
    RCMVS_REQUIRE(pts && lattice_host && dims_host && key_a && idx_a && key_b && idx_b && hist && hist_start && scan_work && head && head_start,
                  "pc_voxel_sort: null pointer");
    RCMVS_REQUIRE(n > 0 && n <= (1ll << 31) - 256, "pc_voxel_sort: n=%lld (1 .. 2^31-256)", n);
    PcrLattice L;
    for (int a = 0; a < 3; ++a) { L.org[a] = lattice_host[a]; L.g[a] = dims_host[a]; }
    L.voxel = lattice_host[3];
    RCMVS_REQUIRE(L.voxel > 0.0 && std::isfinite(L.voxel), "pc_voxel_sort: voxel %g", L.voxel);
    RCMVS_REQUIRE(std::isfinite(L.org[0]) && std::isfinite(L.org[1]) && std::isfinite(L.org[2]), "pc_voxel_sort: lattice origin is not finite");
    for (int a = 0; a < 3; ++a)
        RCMVS_REQUIRE(L.g[a] >= 1 && L.g[a] <= RCMVS_PC_MAX_VOXELS_PER_AXIS, "pc_voxel_sort: %lld voxels on axis %d (1 .. 2^21)", L.g[a], a);
    int bits = 0;
    for (unsigned long long top = (unsigned long long)(L.g[0] * L.g[1] * L.g[2]) - 1ull; top; top >>= 1) ++bits;
    int passes = (bits + 7) / 8;
    passes = passes < 2 ? 2 : passes + (passes & 1);             // an even count: the sorted pairs end in (key_a, idx_a)
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(n, PCR_BLOCK);
    hipLaunchKernelGGL(pcr_voxel_key_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, pts, (int)n, L, key_a, idx_a);
    for (int p = 0; p < passes; ++p) {
        const unsigned long long* kin = p & 1 ? key_b : key_a;
        const int* iin = p & 1 ? idx_b : idx_a;
        unsigned long long* kout = p & 1 ? key_a : key_b;
        int* iout = p & 1 ? idx_a : idx_b;
        hipLaunchKernelGGL(radix_hist_kernel<unsigned long long>, dim3(nblk), dim3(PCR_BLOCK), 0, st, kin, n, 8 * p, (long long)nblk, hist);
        pc_scan(hist, 256 * nblk, scan_work, hist_start, st);
        hipLaunchKernelGGL(radix_scatter_kernel<unsigned long long>, dim3(nblk), dim3(PCR_BLOCK), 0, st, kin, iin, n, 8 * p, (long long)nblk, hist_start, kout, iout);
    }
    hipLaunchKernelGGL(pcr_voxel_head_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, key_a, (int)n, head);
    pc_scan(head, (int)n, scan_work, head_start, st);
    return launch_status("pc_voxel_sort");
}

extern "C" int rcmvs_pc_voxel_emit(const float* pts, long long n, const unsigned long long* key, const int* idx, const int* head_start,
                                   long long m, float* out, void* stream) {
    RCMVS_REQUIRE(pts && key && idx && head_start && out, "pc_voxel_emit: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31) && m > 0 && m <= n, "pc_voxel_emit: n=%lld m=%lld (1 <= m <= n < 2^31)", n, m);
    hipLaunchKernelGGL(pcr_voxel_emit_kernel, dim3((int)cdiv(n, PCR_BLOCK)), dim3(PCR_BLOCK), 0, as_stream(stream), pts, key, idx, head_start,
                       (int)n, (int)m, out);
    return launch_status("pc_voxel_emit");
}

extern "C" int rcmvs_pc_icp_step(const float* src, long long n, const double* transform_host, const double* grid_host, const int* dims_host,
                                 const int* cell_start, const float* sorted, const int* sorted_idx, long long n_to, double max_dist, int* corr,
                                 double* part, double* out, void* stream) {
    RCMVS_REQUIRE(src && transform_host && cell_start && sorted && sorted_idx && part && out, "pc_icp_step: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31) && n_to > 0 && n_to < (1ll << 31), "pc_icp_step: n=%lld n_to=%lld (1 .. 2^31-1)", n, n_to);
    RCMVS_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist), "pc_icp_step: max_dist %g", max_dist);
    RCMVS_REQUIRE(grid_host && dims_host, "pc_icp_step: null grid description");
    PcrGrid g;
    for (int a = 0; a < 3; ++a) { g.o[a] = grid_host[a]; g.g[a] = dims_host[a]; }
    g.h = grid_host[3];
    RCMVS_REQUIRE(g.h > 0.0 && std::isfinite(g.h), "pc_icp_step: cell edge %g", g.h);
    RCMVS_REQUIRE(g.g[0] >= 1 && g.g[1] >= 1 && g.g[2] >= 1 && (long long)g.g[0] * g.g[1] * g.g[2] <= RCMVS_PC_MAX_CELLS,
                  "pc_icp_step: grid %d x %d x %d (at most %d cells)", g.g[0], g.g[1], g.g[2], RCMVS_PC_MAX_CELLS);
    PcrXform X;
    for (int k = 0; k < 12; ++k) {
        X.T[k] = transform_host[k];
        RCMVS_REQUIRE(std::isfinite(X.T[k]), "pc_icp_step: transform entry %d is not finite", k);
    }
    hipStream_t st = as_stream(stream);
    const int nblk = (int)min(cdiv(n, PCR_BLOCK), (long long)PCR_ICP_BLOCKS);
    hipLaunchKernelGGL(pcr_icp_step_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, src, (int)n, X, g, cell_start,
                       reinterpret_cast<const float4*>(sorted), sorted_idx, max_dist, corr, part);
    hipLaunchKernelGGL(pcr_icp_final_kernel, dim3(PCR_NMOM), dim3(PCR_BLOCK), 0, st, part, nblk, out);
    return launch_status("pc_icp_step");
}

extern "C" int rcmvs_pc_dist_hist(const double* d, long long n, double tau, int nbins, double w, unsigned long long* counts,
                                  unsigned long long* below, void* stream) {
    RCMVS_REQUIRE(d && counts && below, "pc_dist_hist: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_dist_hist: n=%lld (1 .. 2^31-1)", n);
    RCMVS_REQUIRE(nbins >= 1 && nbins <= RCMVS_PC_HIST_MAX_BINS, "pc_dist_hist: %d bins (1 .. %d)", nbins, RCMVS_PC_HIST_MAX_BINS);
    RCMVS_REQUIRE(w > 0.0 && std::isfinite(w) && std::isfinite(tau), "pc_dist_hist: bin width %g, tau %g", w, tau);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(counts, 0, sizeof(unsigned long long) * nbins, st) != hipSuccess) return launch_status("pc_dist_hist: memset");
    if (hipMemsetAsync(below, 0, sizeof(unsigned long long), st) != hipSuccess) return launch_status("pc_dist_hist: memset");
    const int nblk = (int)min(cdiv(n, PCR_BLOCK), (long long)PCR_HIST_BLOCKS);
    hipLaunchKernelGGL(pcr_dist_hist_kernel, dim3(nblk), dim3(PCR_BLOCK), 0, st, d, (int)n, tau, nbins, w, counts, below);
    return launch_status("pc_dist_hist");
}
