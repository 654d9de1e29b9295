// Point-cloud clean-up: the finite filter, k nearest neighbours, the radius count, the statistical rule, normals from the
// neighbourhoods and the ordered compaction (rc_mvsnet_amd/cloud_clean.py; contract in cloud_knn.h, the per-element rules in
// cloud_knn_math.h).
//
//   finite    one thread per point: the flag, and the block's count by one integer atomic.
//   walk      ck_walk, shared by knn and radius: the shells of cells around the query's cell as pc_nn_kernel walks them (the same
//             lower bounds and slack), cells farther than the visitor's bound skipped, stop when the lower bound of everything
//             unvisited, squared, exceeds the bound.  Thread i takes SORTED slot i, so the lanes of a wave walk the same cells.
//   knn       the visitor keeps the k best (d2, input index) as a sorted list in LDS, [slot][lane]: a lane's column is its own, so
//             there is no synchronisation, and the 8-byte reads of a 32-lane half fall on distinct banks.  The worst stays in
//             registers: a candidate is compared with it before LDS or sorted_idx is touched.
//   radius    the visitor counts d2 <= r2 up to cap.
//   stat      valid flags -> scan3 -> the valid means in input order -> rcmvs_pc_moments -> keep flags and {n, mu, sigma, bound}.
//   normals   one thread per point in input order: two passes over its neighbours (mean, covariance), Jacobi, orientation.
//   compact   scan3 of the keep bytes, then one thread per point scatters its row.
// Counters are integer adds.  No kernel waits for another workgroup, and there are no floating-point atomics.
// gfx950 only; __syncthreads, shuffles, plain loads and stores and integer atomics (tests/emu compiles this file too).
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "cloud_knn.h"
#include "cloud_knn_math.h"
#include "scan_sort.h"                                            // gid, blocks, the overlap checks, scan3, zero_kernel

#pragma clang fp contract(off)

namespace rcmvs {

static_assert(ck::MAX_K == RCMVS_CK_MAX_K && ck::MAX_SWEEPS == RCMVS_CK_MAX_SWEEPS && ck::ORIENTED < RCMVS_CK_COUNTERS, "the constants of cloud_knn.h");

using u64 = unsigned long long;

struct CkGrid { double o[3]; double h; int g[3]; };

__device__ inline int ck_cell_coord(float p, double o, double h, int g) {      // pc_cell_coord of pointcloud.hip: the build's rule
    const int c = (int)floor(((double)p - o) / h);
    return c < 0 ? 0 : (c >= g ? g - 1 : c);
}

// the sum of v over the wave's lanes, in lane 0
__device__ inline unsigned ck_wave_sum(unsigned v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// ---- the finite filter --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void ck_finite_kernel(const float* __restrict__ pts, long long n, unsigned char* __restrict__ flags, int* __restrict__ count) {
    const long long i = gid();
    bool ok = false;
    if (i < n) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        ok = fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f;
        flags[i] = ok ? 1 : 0;
    }
    const int c = __syncthreads_count(ok);
    if (threadIdx.x == 0 && c) atomicAdd(count, c);
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
// V: bound2() -> candidates and cells with a squared distance above it cannot matter; done() -> stop now; visit(slot, d2) for every
// point of a visited cell but `self`.  cells / tested count what was read.
template <class V>
__device__ inline void ck_walk(const CkGrid& g, const int* __restrict__ cell_start, const float4* __restrict__ sorted, int self, V& v, unsigned* cells,
                               unsigned* tested) {
    const float4 q = sorted[self];
    const double qd[3] = {(double)q.x, (double)q.y, (double)q.z};
    const double slack = 1e-6 * g.h;
    int c[3];
    c[0] = ck_cell_coord(q.x, g.o[0], g.h, g.g[0]);
    c[1] = ck_cell_coord(q.y, g.o[1], g.h, g.g[1]);
    c[2] = ck_cell_coord(q.z, g.o[2], g.h, g.g[2]);
    for (int r = 0; !v.done(); ++r) {
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
                    double lb2 = 0.0;                            // the cell's box (widened by slack) to q
                    for (int a = 0; a < 3; ++a) {
                        const double lo = g.o[a] + (double)cc[a] * g.h - slack, hi = g.o[a] + (double)(cc[a] + 1) * g.h + slack;
                        const double d = qd[a] < lo ? lo - qd[a] : (qd[a] > hi ? qd[a] - hi : 0.0);
                        lb2 += d * d;
                    }
                    if (lb2 > v.bound2()) continue;
                    const int cell = (z * g.g[1] + y) * g.g[0] + x;
                    const int e = cell_start[cell + 1];
                    ++*cells;
                    for (int j = cell_start[cell]; j < e; ++j) {
                        if (j == self) continue;
                        const float4 t = sorted[j];
                        ++*tested;
                        v.visit(j, pc::dist2(q.x, q.y, q.z, t.x, t.y, t.z));
                    }
                }
            }
        }
        // every point not yet visited lies in the grid's box and outside the searched cube on some side still open
        double side = INFINITY;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) side = fmin(side, qd[a] - (g.o[a] + (double)(c[a] - r) * g.h));
            if (c[a] + r < g.g[a] - 1) side = fmin(side, (g.o[a] + (double)(c[a] + r + 1) * g.h) - qd[a]);
        }
        if (side == INFINITY) break;                             // the whole grid has been searched
        const double lb = side - slack;
        if (lb > 0.0 && lb * lb > v.bound2()) break;
    }
}

// ---- k nearest ----------------------------------------------------------------------------------------------------------------------
// the k best of one lane: column `lane` of two LDS arrays, ascending by (d2, input index); empty slots hold (+inf, INT_MAX)
template <int B>
struct CkBest {
    double* d2;                                                  // &list_d2[0][lane]; slot s at d2[s * B]
    int* idx;
    const int* __restrict__ sorted_idx;
    int k;
    double worst_d2;
    int worst_idx;
    __device__ double bound2() const { return worst_d2; }
    __device__ bool done() const { return false; }
    __device__ void visit(int slot, double cd2) {
        if (cd2 > worst_d2) return;
        const int ci = sorted_idx[slot];
        if (!ck::before(cd2, ci, worst_d2, worst_idx)) return;
        int s = k - 1;                                           // the worst falls out; entries after the candidate move down one slot
        for (; s > 0; --s) {
            const double pd = d2[(s - 1) * B];
            const int pi = idx[(s - 1) * B];
            if (!ck::before(cd2, ci, pd, pi)) break;
            d2[s * B] = pd;
            idx[s * B] = pi;
        }
        d2[s * B] = cd2;
        idx[s * B] = ci;
        worst_d2 = d2[(k - 1) * B];
        worst_idx = idx[(k - 1) * B];
    }
};

template <int K, int B>
__global__ __launch_bounds__(B) void ck_knn_kernel(int n, int k, CkGrid g, const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                   const int* __restrict__ sorted_idx, int* __restrict__ out_idx, double* __restrict__ out_d2,
                                                   double* __restrict__ out_mean, u64* counters) {
    __shared__ double list_d2[K][B];
    __shared__ int list_idx[K][B];
    const long long i = (long long)blockIdx.x * B + threadIdx.x;
    unsigned cells = 0, tested = 0;
    if (i < n) {
        CkBest<B> best;
        best.d2 = &list_d2[0][threadIdx.x];
        best.idx = &list_idx[0][threadIdx.x];
        best.sorted_idx = sorted_idx;
        best.k = k;
        best.worst_d2 = INFINITY;
        best.worst_idx = INT_MAX;
        for (int s = 0; s < k; ++s) {
            best.d2[s * B] = INFINITY;
            best.idx[s * B] = INT_MAX;
        }
        ck_walk(g, cell_start, sorted, (int)i, best, &cells, &tested);
        const long long row = (long long)sorted_idx[i] * k;
        double sum = 0.0;
        bool missing = false;
        for (int s = 0; s < k; ++s) {
            const double d = best.d2[s * B];
            const int j = best.idx[s * B];
            missing = missing || j == INT_MAX;
            sum = sum + sqrt(d);
            if (out_idx) out_idx[row + s] = j == INT_MAX ? -1 : j;
            if (out_d2) out_d2[row + s] = d;
        }
        if (out_mean) out_mean[sorted_idx[i]] = missing ? (double)NAN : sum / (double)k;
    }
    if (counters) {                                              // uniform: every lane of the block takes the branch
        const unsigned c = ck_wave_sum(cells), t = ck_wave_sum(tested);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            atomicAdd(&counters[0], (u64)c);
            atomicAdd(&counters[1], (u64)t);
        }
    }
}

// ---- radius count -------------------------------------------------------------------------------------------------------------------
struct CkCount {
    double r2;
    int cap, count;
    __device__ double bound2() const { return r2; }
    __device__ bool done() const { return count >= cap; }
    __device__ void visit(int, double d2) { if (d2 <= r2 && count < cap) ++count; }
};

__global__ __launch_bounds__(SS_BLOCK) void ck_radius_kernel(int n, double r2, int cap, CkGrid g, const int* __restrict__ cell_start,
                                                             const float4* __restrict__ sorted, const int* __restrict__ sorted_idx, int* __restrict__ count,
                                                             unsigned char* __restrict__ keep) {
    const long long i = gid();
    if (i >= n) return;
    CkCount v = {r2, cap, 0};
    unsigned cells = 0, tested = 0;
    ck_walk(g, cell_start, sorted, (int)i, v, &cells, &tested);
    count[sorted_idx[i]] = v.count;
    if (keep) keep[sorted_idx[i]] = v.count >= cap ? 1 : 0;
}

// ---- the statistical rule -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void ck_valid_kernel(const double* __restrict__ mean, long long n, unsigned char* __restrict__ flags) {
    const long long i = gid();
    if (i < n) { const double m = mean[i]; flags[i] = m == m ? 1 : 0; }
}

__global__ __launch_bounds__(SS_BLOCK) void ck_gather_valid_kernel(const double* __restrict__ mean, long long n, const unsigned char* __restrict__ flags,
                                                                   const int* __restrict__ offsets, double* __restrict__ valid_mean) {
    const long long i = gid();
    if (i >= n || !flags[i]) return;
    const long long dst = offsets[i];
    if (dst >= 0 && dst < n) valid_mean[dst] = mean[i];
}

// moments = rcmvs_pc_moments' {n, mean, variance}, read by every thread; stats = {n, mu, sigma, bound}, another place, written by one
__global__ __launch_bounds__(SS_BLOCK) void ck_keep_kernel(const double* __restrict__ mean, long long n, const unsigned char* __restrict__ flags,
                                                           const double* __restrict__ moments, double ratio, unsigned char* __restrict__ keep,
                                                           double* __restrict__ stats) {
    const long long i = gid();
    const double mu = moments[1], sigma = sqrt(moments[2]);
    const double bound = ck::threshold(mu, sigma, ratio);
    if (i == 0) { stats[0] = moments[0]; stats[1] = mu; stats[2] = sigma; stats[3] = bound; stats[7] = 0.0; }
    if (i < n) keep[i] = flags[i] && mean[i] <= bound ? 1 : 0;
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void ck_normals_kernel(const float* __restrict__ pts, long long n, int k, const int* __restrict__ idx,
                                                              const int* __restrict__ view, const double* __restrict__ centres, int nc,
                                                              float* __restrict__ normals, long long* counters) {
    const long long i = gid();
    int what = -1, how = -1;                                     // what: WITH_NORMAL, TOO_FEW or DEGENERATE_N; how: UNORIENTED, FLIPPED or ORIENTED
    bool unconverged = false;
    if (i < n) {
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        double s[3] = {(double)px, (double)py, (double)pz};
        int m = 1;
        for (int q = 0; q < k; ++q) {
            const int j = idx[i * k + q];
            if ((unsigned)j >= (unsigned long long)n) continue;
            s[0] = s[0] + (double)pts[3 * (long long)j];
            s[1] = s[1] + (double)pts[3 * (long long)j + 1];
            s[2] = s[2] + (double)pts[3 * (long long)j + 2];
            ++m;
        }
        double nrm[3] = {0.0, 0.0, 0.0};
        if (m < 3) what = ck::TOO_FEW;
        else {
            const double mean[3] = {s[0] / (double)m, s[1] / (double)m, s[2] / (double)m};
            ck::Sym3 c = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            ck::cov_add(mean, px, py, pz, &c);
            for (int q = 0; q < k; ++q) {
                const int j = idx[i * k + q];
                if ((unsigned)j >= (unsigned long long)n) continue;
                ck::cov_add(mean, pts[3 * (long long)j], pts[3 * (long long)j + 1], pts[3 * (long long)j + 2], &c);
            }
            ck::cov_finish(&c, m);
            bool converged;
            what = ck::normal_of(c, nrm, &converged);
            unconverged = !converged;
            if (what == ck::WITH_NORMAL && view) {
                const int w = view[i];
                if ((unsigned)w >= (unsigned)nc) how = ck::UNORIENTED;
                else how = ck::orient(nrm, px, py, pz, centres + 3 * (long long)w) ? ck::FLIPPED : ck::ORIENTED;
            }
        }
        normals[3 * i] = (float)nrm[0];
        normals[3 * i + 1] = (float)nrm[1];
        normals[3 * i + 2] = (float)nrm[2];
    }
    for (int c = 0; c < RCMVS_CK_COUNTERS - 1; ++c) {
        const int hit = c == ck::UNCONVERGED ? unconverged : (c == what || c == how);
        const int s = __syncthreads_count(hit);
        if (threadIdx.x == 0 && s) atomicAdd(reinterpret_cast<u64*>(counters) + c, (u64)s);
    }
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_BLOCK) void ck_scatter_kernel(const unsigned char* __restrict__ keep, const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                              const int* __restrict__ view, long long n, const int* __restrict__ offsets, float* __restrict__ out_xyz,
                                                              unsigned char* __restrict__ out_rgb, int* __restrict__ out_view, int* __restrict__ out_index) {
    const long long i = gid();
    if (i >= n || !keep[i]) return;
    const long long d = offsets[i];
    if (d < 0 || d >= n) return;                                 // keep bytes other than 0 and 1 are a caller's error: never an address
    for (int a = 0; a < 3; ++a) out_xyz[3 * d + a] = xyz[3 * i + a];
    if (rgb)
        for (int a = 0; a < 3; ++a) out_rgb[3 * d + a] = rgb[3 * i + a];
    if (view) out_view[d] = view[i];
    out_index[d] = (int)i;
}

static int ck_n(const char* what, long long n) {
    RCMVS_REQUIRE(n >= 0 && n < (1ll << 31), "%s: n = %lld points (0 .. 2^31-1)", what, n);
    return 0;
}

static int ck_phase(const char* what, int phase) {
    RCMVS_REQUIRE(phase == RCMVS_CK_PHASE_ALL, "%s: phase = %d (0: all)", what, phase);
    return 0;
}

static int ck_aligned(const char* what, const char* name, const void* p, int bytes) {
    RCMVS_REQUIRE((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0, "%s: %s must be %d-byte aligned", what, name, bytes);
    return 0;
}

static int ck_grid(const char* what, const double* grid_host, const int* dims_host, CkGrid* g, long long* cells) {
    RCMVS_REQUIRE(grid_host && dims_host, "%s: null pointer (grid_host, dims_host)", what);
    for (int a = 0; a < 3; ++a) { g->o[a] = grid_host[a]; g->g[a] = dims_host[a]; }
    g->h = grid_host[3];
    RCMVS_REQUIRE(g->h > 0.0 && std::isfinite(g->h) && std::isfinite(g->o[0]) && std::isfinite(g->o[1]) && std::isfinite(g->o[2]),
                  "%s: grid_host = {%g, %g, %g, %g} (a finite origin and a finite cell edge > 0)", what, g->o[0], g->o[1], g->o[2], g->h);
    RCMVS_REQUIRE(g->g[0] >= 1 && g->g[1] >= 1 && g->g[2] >= 1 && (long long)g->g[0] * g->g[1] * g->g[2] <= RCMVS_PC_MAX_CELLS,
                  "%s: dims_host = %d x %d x %d (at most %d cells)", what, g->g[0], g->g[1], g->g[2], RCMVS_PC_MAX_CELLS);
    *cells = (long long)g->g[0] * g->g[1] * g->g[2];
    return 0;
}

template <int K, int B>
static void ck_knn_launch(long long n, int k, const CkGrid& g, const int* cell_start, const float* sorted, const int* sorted_idx, int* idx, double* d2, double* mean,
                          u64* counters, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    auto kernel = &ck_knn_kernel<K, B>;
    RCMVS_LAUNCH_TIMED(kernel, dim3((unsigned)cdiv(n, B)), dim3(B), 0, st, e0, e1, (int)n, k, g, cell_start, reinterpret_cast<const float4*>(sorted),
                       sorted_idx, idx, d2, mean, counters);
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_ck_finite_timed(const float* pts, long long n, unsigned char* flags, int* count, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "ck_finite";
    if (int rc = ck_n(what, n)) return rc;
    if (int rc = ck_phase(what, phase)) return rc;
    RCMVS_REQUIRE(count, "%s: null pointer (count)", what);
    RCMVS_REQUIRE(n == 0 || (pts && flags), "%s: null pointer (pts and flags hold n rows)", what);
    if (int rc = ck_aligned(what, "pts", pts, 4)) return rc;
    if (int rc = ck_aligned(what, "count", count, 4)) return rc;
    {
        const void* ptr[] = {flags, count, pts};
        const size_t len[] = {(size_t)n, 4, (size_t)n * 12};
        if (int rc = buffers_overlap(what, ptr, len, 2, 3)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<int>, dim3(1), dim3(SS_BLOCK), 0, st, e0, none, count, 1ll);
    RCMVS_LAUNCH_TIMED(ck_finite_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, none, e1, pts, n, flags, count);
    return launch_status(what);
}

extern "C" int rcmvs_ck_finite(const float* pts, long long n, unsigned char* flags, int* count, void* stream) {
    return rcmvs_ck_finite_timed(pts, n, flags, count, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ck_knn_timed(long long n, int k, const double* grid_host, const int* dims_host, const int* cell_start, const float* sorted,
                                  const int* sorted_idx, int* idx, double* d2, double* mean, u64* counters, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "ck_knn";
    if (int rc = ck_n(what, n)) return rc;
    RCMVS_REQUIRE(k >= 1 && k <= RCMVS_CK_MAX_K, "%s: k = %d (1 .. %d)", what, k, RCMVS_CK_MAX_K);
    RCMVS_REQUIRE(n * k <= RCMVS_CK_MAX_NK, "%s: n k = %lld (at most 2^31-256)", what, n * k);
    if (int rc = ck_phase(what, phase)) return rc;
    if (int rc = ck_aligned(what, "idx", idx, 4)) return rc;
    if (int rc = ck_aligned(what, "d2", d2, 8)) return rc;
    if (int rc = ck_aligned(what, "mean", mean, 8)) return rc;
    if (int rc = ck_aligned(what, "counters", counters, 8)) return rc;
    if (n == 0) return 0;
    CkGrid g;
    long long cells;
    if (int rc = ck_grid(what, grid_host, dims_host, &g, &cells)) return rc;
    RCMVS_REQUIRE(cell_start && sorted && sorted_idx, "%s: null pointer (cell_start, sorted, sorted_idx)", what);
    if (int rc = ck_aligned(what, "sorted", sorted, 16)) return rc;
    if (int rc = ck_aligned(what, "cell_start", cell_start, 4)) return rc;
    if (int rc = ck_aligned(what, "sorted_idx", sorted_idx, 4)) return rc;
    {
        const void* ptr[] = {idx, d2, mean, counters, cell_start, sorted, sorted_idx};
        const size_t len[] = {(size_t)(n * k) * 4, (size_t)(n * k) * 8, (size_t)n * 8, 16, (size_t)(cells + 1) * 4, (size_t)n * 16, (size_t)n * 4};
        if (int rc = buffers_overlap(what, ptr, len, 4, 7)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    if (k <= 8) ck_knn_launch<8, 256>(n, k, g, cell_start, sorted, sorted_idx, idx, d2, mean, counters, st, e0, e1);
    else if (k <= 16) ck_knn_launch<16, 256>(n, k, g, cell_start, sorted, sorted_idx, idx, d2, mean, counters, st, e0, e1);
    else ck_knn_launch<32, 128>(n, k, g, cell_start, sorted, sorted_idx, idx, d2, mean, counters, st, e0, e1);
    return launch_status(what);
}

extern "C" int rcmvs_ck_knn(long long n, int k, const double* grid_host, const int* dims_host, const int* cell_start, const float* sorted,
                            const int* sorted_idx, int* idx, double* d2, double* mean, u64* counters, void* stream) {
    return rcmvs_ck_knn_timed(n, k, grid_host, dims_host, cell_start, sorted, sorted_idx, idx, d2, mean, counters, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ck_radius_timed(long long n, double r2, int cap, const double* grid_host, const int* dims_host, const int* cell_start,
                                     const float* sorted, const int* sorted_idx, int* count, unsigned char* keep, int phase, void* ev0, void* ev1,
                                     void* stream) {
    const char* what = "ck_radius";
    if (int rc = ck_n(what, n)) return rc;
    RCMVS_REQUIRE(r2 >= 0.0, "%s: r2 = %g (>= 0; +inf is allowed)", what, r2);
    RCMVS_REQUIRE(cap >= 0, "%s: cap = %d (>= 0)", what, cap);
    if (int rc = ck_phase(what, phase)) return rc;
    if (n == 0) return 0;
    CkGrid g;
    long long cells;
    if (int rc = ck_grid(what, grid_host, dims_host, &g, &cells)) return rc;
    RCMVS_REQUIRE(cell_start && sorted && sorted_idx && count, "%s: null pointer (cell_start, sorted, sorted_idx, count)", what);
    if (int rc = ck_aligned(what, "sorted", sorted, 16)) return rc;
    if (int rc = ck_aligned(what, "count", count, 4)) return rc;
    if (int rc = ck_aligned(what, "cell_start", cell_start, 4)) return rc;
    if (int rc = ck_aligned(what, "sorted_idx", sorted_idx, 4)) return rc;
    {
        const void* ptr[] = {count, keep, cell_start, sorted, sorted_idx};
        const size_t len[] = {(size_t)n * 4, (size_t)n, (size_t)(cells + 1) * 4, (size_t)n * 16, (size_t)n * 4};
        if (int rc = buffers_overlap(what, ptr, len, 2, 5)) return rc;
    }
    RCMVS_LAUNCH_TIMED(ck_radius_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, as_stream(stream), static_cast<hipEvent_t>(ev0), static_cast<hipEvent_t>(ev1), (int)n, r2,
                       cap, g, cell_start, reinterpret_cast<const float4*>(sorted), sorted_idx, count, keep);
    return launch_status(what);
}

extern "C" int rcmvs_ck_radius(long long n, double r2, int cap, const double* grid_host, const int* dims_host, const int* cell_start,
                               const float* sorted, const int* sorted_idx, int* count, unsigned char* keep, void* stream) {
    return rcmvs_ck_radius_timed(n, r2, cap, grid_host, dims_host, cell_start, sorted, sorted_idx, count, keep, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ck_stat_timed(const double* mean, long long n, double ratio, unsigned char* flags, int* offsets, int* scan_work, double* valid_mean,
                                   double* part, double* stats, unsigned char* keep, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "ck_stat";
    if (int rc = ck_n(what, n)) return rc;
    RCMVS_REQUIRE(ratio >= 0.0, "%s: ratio = %g (>= 0; +inf is allowed)", what, ratio);
    if (int rc = ck_phase(what, phase)) return rc;
    RCMVS_REQUIRE(offsets && part && stats, "%s: null pointer (offsets, part, stats)", what);
    RCMVS_REQUIRE(n == 0 || (mean && flags && valid_mean && keep), "%s: null pointer (mean, flags, valid_mean and keep hold n elements)", what);
    if (int rc = scan_work_check(what, scan_work)) return rc;
    if (int rc = ck_aligned(what, "mean", mean, 8)) return rc;
    if (int rc = ck_aligned(what, "valid_mean", valid_mean, 8)) return rc;
    if (int rc = ck_aligned(what, "part", part, 8)) return rc;
    if (int rc = ck_aligned(what, "stats", stats, 8)) return rc;
    if (int rc = ck_aligned(what, "offsets", offsets, 4)) return rc;
    {
        const void* ptr[] = {flags, offsets, valid_mean, part, stats, keep, mean};
        const size_t len[] = {(size_t)n, (size_t)(n + 1) * 4, (size_t)n * 8, (size_t)RCMVS_PC_MOMENT_BLOCKS * 8, 64, (size_t)n, (size_t)n * 8};
        if (int rc = buffers_overlap(what, ptr, len, 6, 7)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(ck_valid_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, e0, none, mean, n, flags);
    scan3<unsigned char>(flags, n, offsets, scan_work, nullptr, st, none, none);
    hipLaunchKernelGGL(ck_gather_valid_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, mean, n, flags, offsets, valid_mean);
    if (int rc = rcmvs_pc_moments(valid_mean ? valid_mean : part, offsets + n, part, stats + 4, stream)) return rc;
    RCMVS_LAUNCH_TIMED(ck_keep_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, none, e1, mean, n, flags, stats + 4, ratio, keep, stats);
    return launch_status(what);
}

extern "C" int rcmvs_ck_stat(const double* mean, long long n, double ratio, unsigned char* flags, int* offsets, int* scan_work, double* valid_mean, double* part,
                             double* stats, unsigned char* keep, void* stream) {
    return rcmvs_ck_stat_timed(mean, n, ratio, flags, offsets, scan_work, valid_mean, part, stats, keep, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ck_normals_timed(const float* pts, long long n, int k, const int* idx, const int* view, const double* centres, int nc, float* normals,
                                      long long* counters, int phase, void* ev0, void* ev1, void* stream) {
    const char* what = "ck_normals";
    if (int rc = ck_n(what, n)) return rc;
    RCMVS_REQUIRE(k >= 1 && k <= RCMVS_CK_MAX_K, "%s: k = %d (1 .. %d)", what, k, RCMVS_CK_MAX_K);
    RCMVS_REQUIRE(n * k <= RCMVS_CK_MAX_NK, "%s: n k = %lld (at most 2^31-256)", what, n * k);
    RCMVS_REQUIRE(nc >= 0, "%s: nc = %d centres (>= 0)", what, nc);
    if (int rc = ck_phase(what, phase)) return rc;
    RCMVS_REQUIRE(counters, "%s: null pointer (counters)", what);
    RCMVS_REQUIRE(n == 0 || (pts && idx && normals), "%s: null pointer (pts, idx and normals hold n rows)", what);
    RCMVS_REQUIRE(n == 0 || (view ? centres || nc == 0 : !centres), "%s: view and centres come together", what);
    if (int rc = ck_aligned(what, "counters", counters, 8)) return rc;
    if (int rc = ck_aligned(what, "centres", centres, 8)) return rc;
    if (int rc = ck_aligned(what, "normals", normals, 4)) return rc;
    if (int rc = ck_aligned(what, "idx", idx, 4)) return rc;
    if (int rc = ck_aligned(what, "view", view, 4)) return rc;
    {
        const void* ptr[] = {normals, counters, pts, idx, view, centres};
        const size_t len[] = {(size_t)n * 12, (size_t)RCMVS_CK_COUNTERS * 8, (size_t)n * 12, (size_t)(n * k) * 4, view ? (size_t)n * 4 : 0, (size_t)nc * 24};
        if (int rc = buffers_overlap(what, ptr, len, 2, 6)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    RCMVS_LAUNCH_TIMED(zero_kernel<u64>, dim3(1), dim3(SS_BLOCK), 0, st, e0, none, reinterpret_cast<u64*>(counters), (long long)RCMVS_CK_COUNTERS);
    RCMVS_LAUNCH_TIMED(ck_normals_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, none, e1, pts, n, k, idx, view, centres, nc, normals, counters);
    return launch_status(what);
}

extern "C" int rcmvs_ck_normals(const float* pts, long long n, int k, const int* idx, const int* view, const double* centres, int nc, float* normals,
                                long long* counters, void* stream) {
    return rcmvs_ck_normals_timed(pts, n, k, idx, view, centres, nc, normals, counters, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}

extern "C" int rcmvs_ck_compact_timed(const unsigned char* keep, const float* xyz, const unsigned char* rgb, const int* view, long long n, int* offsets,
                                      int* scan_work, float* out_xyz, unsigned char* out_rgb, int* out_view, int* out_index, u64* total, int phase, void* ev0,
                                      void* ev1, void* stream) {
    const char* what = "ck_compact";
    if (int rc = ck_n(what, n)) return rc;
    if (int rc = ck_phase(what, phase)) return rc;
    RCMVS_REQUIRE(offsets && total, "%s: null pointer (offsets, total)", what);
    RCMVS_REQUIRE(n == 0 || (keep && xyz && out_xyz && out_index), "%s: null pointer (keep, xyz, out_xyz and out_index hold n rows)", what);
    RCMVS_REQUIRE(n == 0 || ((rgb != nullptr) == (out_rgb != nullptr) && (view != nullptr) == (out_view != nullptr)),
                  "%s: rgb and out_rgb, view and out_view come together", what);
    if (int rc = scan_work_check(what, scan_work)) return rc;
    if (int rc = ck_aligned(what, "total", total, 8)) return rc;
    if (int rc = ck_aligned(what, "offsets", offsets, 4)) return rc;
    if (int rc = ck_aligned(what, "out_xyz", out_xyz, 4)) return rc;
    if (int rc = ck_aligned(what, "out_view", out_view, 4)) return rc;
    if (int rc = ck_aligned(what, "out_index", out_index, 4)) return rc;
    {
        const void* ptr[] = {offsets, out_xyz, out_rgb, out_view, out_index, total, keep, xyz, rgb, view};
        const size_t len[] = {(size_t)(n + 1) * 4, (size_t)n * 12, out_rgb ? (size_t)n * 3 : 0, out_view ? (size_t)n * 4 : 0, (size_t)n * 4, 8, (size_t)n, (size_t)n * 12,
                              rgb ? (size_t)n * 3 : 0, view ? (size_t)n * 4 : 0};
        if (int rc = buffers_overlap(what, ptr, len, 6, 10)) return rc;
    }
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1), none = nullptr;
    scan3<unsigned char>(keep, n, offsets, scan_work, total, st, e0, none);
    RCMVS_LAUNCH_TIMED(ck_scatter_kernel, dim3(blocks(n)), dim3(SS_BLOCK), 0, st, none, e1, keep, xyz, rgb, view, n, offsets, out_xyz, out_rgb, out_view, out_index);
    return launch_status(what);
}

extern "C" int rcmvs_ck_compact(const unsigned char* keep, const float* xyz, const unsigned char* rgb, const int* view, long long n, int* offsets, int* scan_work,
                                float* out_xyz, unsigned char* out_rgb, int* out_view, int* out_index, u64* total, void* stream) {
    return rcmvs_ck_compact_timed(keep, xyz, rgb, view, n, offsets, scan_work, out_xyz, out_rgb, out_view, out_index, total, RCMVS_CK_PHASE_ALL, nullptr, nullptr, stream);
}
