// DTU point-cloud scorer (rc_mvsnet_amd/dtu_eval.py): the reference scores a fused cloud only in MATLAB
// (matlab_eval/PointCompareMain.m: reducePts_haa.m's 0.2 mm density reduction, MaxDistCP.m's two nearest-neighbour passes in
// 60 mm blocks, the ObsMask / ground-plane tests; then ComputeStat_web_pt.m).  Here every per-point pass is a kernel:
//
//   grid      a dense uniform grid over the target cloud's box: bounding box (two launches), cell keys + histogram
//             (atomics), exclusive scan of the cell counts (block reduce -> scan of the block sums -> add; no inter-block
//             flags), scatter into cell order (a counting sort).  The cell edge comes from the extent (<= RCMVS_PC_MAX_CELLS).
//   nn        one thread per query: shells of cells outward from the query's (clamped) cell, cells whose box is farther
//             than the best distance so far skipped, stop when the unsearched region's lower bound passes the best
//             distance or the cap.  Candidates in fp64 (pointcloud_math.h).
//   reduce    the sequential greedy of reducePts_haa as rounds: a point becomes KEPT when every earlier-ranked neighbour
//             within dst is REMOVED, REMOVED when one of them is KEPT; states are double-buffered, so a round reads only
//             the previous round's states and the result does not depend on block scheduling.  A device counter of the
//             points still undecided ends the host's loop.
//   select    DataInMask / StlAbovePlane and the outlier threshold, compacted in point order, then fp64 moments
//             (two passes, fixed summation tree).
//   mesh      MeshSupSamp (the 'Surfaces' input): one thread per face counts its non-empty rows, one thread per row its
//             points (binary searches, pointcloud_math.h), int64 totals for the host's 2^31 check; the scans of both give the
//             output slots, and one thread per output point finds its row and face by binary search (narrowed to the block's
//             range) and writes the vertices, then the samples, through LDS as contiguous dwords.
// gfx950 only; only plain atomics, __syncthreads, ballots and shuffles (tests/emu compiles this file too).
#include <climits>

#include "common.h"
#include "pointcloud_math.h"
#include "pointcloud_scan.h"                                      // pc_scan, defined here

namespace rcmvs {

constexpr int PC_BLOCK = 256;
constexpr int PC_SCAN_TILE = RCMVS_PC_SCAN_TILE;              // ints per block of the multi-block scan (8 per thread)
constexpr int PC_BBOX_BLOCKS = RCMVS_PC_BBOX_BLOCKS;
constexpr int PC_MOMENT_BLOCKS = RCMVS_PC_MOMENT_BLOCKS;

struct PcGrid { double o[3]; double h; int g[3]; };
struct PcLattice { double lo[3], hi[3]; };

__device__ inline int pc_cell_coord(float p, double o, double h, int g) {
    const int c = (int)floor(((double)p - o) / h);
    return c < 0 ? 0 : (c >= g ? g - 1 : c);
}

// ---- bounding box ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void pc_bbox_kernel(const float* __restrict__ p, int n, float* __restrict__ part) {
    __shared__ float s[6][PC_BLOCK];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += gridDim.x * PC_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float x = p[(long long)i * 3 + a]; v[a] = fminf(v[a], x); v[3 + a] = fmaxf(v[3 + a], x); }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) s[a][threadIdx.x] = v[a];
    __syncthreads();
    for (int o = PC_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fminf(s[a][threadIdx.x], s[a][threadIdx.x + o]);
                s[3 + a][threadIdx.x] = fmaxf(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + o]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void pc_bbox_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out) {
    const int a = threadIdx.x;
    if (a >= 6) return;
    float v = part[a];
    for (int b = 1; b < nblk; ++b) v = a < 3 ? fminf(v, part[b * 6 + a]) : fmaxf(v, part[b * 6 + a]);
    out[a] = v;
}

// ---- exclusive scan of n ints: in[0..n) -> out[0..n), out[n] = total --------------------------------------------------
__device__ inline int pc_block_exclusive(int v, int* sh) {      // exclusive prefix of v over the block; sh: PC_BLOCK ints
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < PC_BLOCK; o <<= 1) {
        const int t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const int r = sh[threadIdx.x] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(PC_BLOCK) void pc_scan_reduce_kernel(const int* __restrict__ in, int n, int* __restrict__ bsum) {
    constexpr int PER = PC_SCAN_TILE / PC_BLOCK;
    const long long base = (long long)blockIdx.x * PC_SCAN_TILE + threadIdx.x * PER;
    int s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) s += base + k < n ? in[base + k] : 0;
    __shared__ int sh[PC_BLOCK];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = PC_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}

// in place: bsum[0..nb) -> exclusive prefix sums, bsum[nb] = total.  One block of 1024 threads.
__global__ __launch_bounds__(1024) void pc_scan_bsums_kernel(int* __restrict__ bsum, int nb) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int chunk = (nb + 1023) / 1024;
    const int lo = min(t * chunk, nb), hi = min(lo + chunk, nb);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += bsum[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) { const int c = bsum[i]; bsum[i] = run; run += c; }
    if (t == 1023) bsum[nb] = part[1023];
}

__global__ __launch_bounds__(PC_BLOCK) void pc_scan_add_kernel(const int* __restrict__ in, int n, const int* __restrict__ bsum, int nb,
                                                               int* __restrict__ out) {
    constexpr int PER = PC_SCAN_TILE / PC_BLOCK;
    __shared__ int sh[PC_BLOCK];
    const long long base = (long long)blockIdx.x * PC_SCAN_TILE + threadIdx.x * PER;
    int v[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { v[k] = base + k < n ? in[base + k] : 0; s += v[k]; }
    int run = pc_block_exclusive(s, sh) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PER; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

void pc_scan(const int* in, int n, int* bsum, int* out, hipStream_t st) {
    const int nb = (int)cdiv(n, PC_SCAN_TILE);
    hipLaunchKernelGGL(pc_scan_reduce_kernel, dim3(nb), dim3(PC_BLOCK), 0, st, in, n, bsum);
    hipLaunchKernelGGL(pc_scan_bsums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb);
    hipLaunchKernelGGL(pc_scan_add_kernel, dim3(nb), dim3(PC_BLOCK), 0, st, in, n, bsum, nb, out);
}

// ---- grid build (counting sort) -------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void pc_key_kernel(const float* __restrict__ p, int n, PcGrid g, int* __restrict__ key,
                                                          int* __restrict__ count) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int cx = pc_cell_coord(p[(long long)i * 3 + 0], g.o[0], g.h, g.g[0]);
    const int cy = pc_cell_coord(p[(long long)i * 3 + 1], g.o[1], g.h, g.g[1]);
    const int cz = pc_cell_coord(p[(long long)i * 3 + 2], g.o[2], g.h, g.g[2]);
    const int k = (cz * g.g[1] + cy) * g.g[0] + cx;
    key[i] = k;
    atomicAdd(&count[k], 1);
}

// count[] runs down to 0 here: a cell is filled from its end, so the order inside a cell is the atomics' (no result depends on it)
__global__ __launch_bounds__(PC_BLOCK) void pc_scatter_kernel(const float* __restrict__ p, int n, const int* __restrict__ key,
                                                              const int* __restrict__ cell_start, int* __restrict__ count,
                                                              float4* __restrict__ sorted, int* __restrict__ sorted_idx) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int k = key[i];
    const int slot = cell_start[k] + atomicAdd(&count[k], -1) - 1;
    sorted[slot] = make_float4(p[(long long)i * 3 + 0], p[(long long)i * 3 + 1], p[(long long)i * 3 + 2], 0.0f);
    sorted_idx[slot] = i;
}

// ---- capped nearest neighbour ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void pc_nn_kernel(const float* __restrict__ q, int nq, PcGrid g, const int* __restrict__ cell_start,
                                                         const float4* __restrict__ sorted, int n_to, double cap, int use_lattice,
                                                         PcLattice lat, double* __restrict__ out) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= nq) return;
    const float qx = q[(long long)i * 3 + 0], qy = q[(long long)i * 3 + 1], qz = q[(long long)i * 3 + 2];
    if (n_to == 0 || (use_lattice && !pc::in_lattice(qx, qy, qz, lat.lo, lat.hi))) { out[i] = cap; return; }
    const double qd[3] = {(double)qx, (double)qy, (double)qz};
    const double slack = 1e-6 * g.h;
    double gap2 = 0.0;                                           // squared distance from q to the grid's box
    for (int a = 0; a < 3; ++a) {
        const double lo = g.o[a], hi = g.o[a] + (double)g.g[a] * g.h;
        const double d = qd[a] < lo ? lo - qd[a] : (qd[a] > hi ? qd[a] - hi : 0.0);
        gap2 += d * d;
    }
    const double gap = sqrt(gap2) - slack;
    if (gap > cap) { out[i] = cap; return; }
    int c[3];
    c[0] = pc_cell_coord(qx, g.o[0], g.h, g.g[0]);
    c[1] = pc_cell_coord(qy, g.o[1], g.h, g.g[1]);
    c[2] = pc_cell_coord(qz, g.o[2], g.h, g.g[2]);
    double best2 = INFINITY;
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
                    double lb2 = 0.0;                            // the cell's box (widened by slack) to q
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
                        const double d2 = pc::dist2(qx, qy, qz, t.x, t.y, t.z);
                        best2 = d2 < best2 ? d2 : best2;
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
        const double lb = fmax(side - slack, gap);
        if (lb > 0.0 && (lb * lb > best2 || lb > cap)) break;
    }
    const double d = sqrt(best2);
    out[i] = d < cap ? d : cap;
}

// ---- greedy reduction in rounds -------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLOCK) void pc_rank_kernel(const long long* __restrict__ order, const int* __restrict__ sorted_idx, int n,
                                                           int* __restrict__ rank, int* __restrict__ sorted_rank, int phase) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (phase == 0) {
        const long long o = order[i];
        if (o >= 0 && o < n) rank[o] = i;                        // order is checked to be a permutation on the host side
    } else {
        sorted_rank[i] = rank[sorted_idx[i]];
    }
}

__global__ __launch_bounds__(PC_BLOCK) void pc_reduce_round_kernel(PcGrid g, const int* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                                   const int* __restrict__ sorted_rank, const unsigned char* __restrict__ s_in,
                                                                   unsigned char* __restrict__ s_out, int n, double dst, int* __restrict__ undecided) {
    const int j = blockIdx.x * PC_BLOCK + threadIdx.x;
    bool open = false;
    if (j < n) {
        const unsigned char s = s_in[j];
        if (s != pc::UNDECIDED) {
            s_out[j] = s;
        } else {
            const float4 p = sorted[j];
            const int rj = sorted_rank[j];
            const int cx = pc_cell_coord(p.x, g.o[0], g.h, g.g[0]);
            const int cy = pc_cell_coord(p.y, g.o[1], g.h, g.g[1]);
            const int cz = pc_cell_coord(p.z, g.o[2], g.h, g.g[2]);
            bool removed = false, pending = false;
            for (int z = max(cz - 1, 0); z <= min(cz + 1, g.g[2] - 1) && !removed; ++z)
                for (int y = max(cy - 1, 0); y <= min(cy + 1, g.g[1] - 1) && !removed; ++y)
                    for (int x = max(cx - 1, 0); x <= min(cx + 1, g.g[0] - 1) && !removed; ++x) {
                        const int k = (z * g.g[1] + y) * g.g[0] + x;
                        const int e = cell_start[k + 1];
                        for (int m = cell_start[k]; m < e; ++m) {
                            if (sorted_rank[m] >= rj) continue;
                            const unsigned char sm = s_in[m];
                            if (sm == pc::REMOVED) continue;
                            const float4 t = sorted[m];
                            if (!pc::within(p.x, p.y, p.z, t.x, t.y, t.z, dst)) continue;
                            if (sm == pc::KEPT) { removed = true; break; }
                            pending = true;
                        }
                    }
            const unsigned char r = removed ? pc::REMOVED : (pending ? pc::UNDECIDED : pc::KEPT);
            s_out[j] = r;
            open = r == pc::UNDECIDED;
        }
    }
    const int c = __syncthreads_count(open);
    if (threadIdx.x == 0 && c) atomicAdd(undecided, c);
}

__global__ __launch_bounds__(PC_BLOCK) void pc_reduce_finish_kernel(const unsigned char* __restrict__ state, const int* __restrict__ sorted_idx,
                                                                    int n, unsigned char* __restrict__ kept) {
    const int j = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (j < n) kept[sorted_idx[j]] = state[j] == pc::KEPT;
}

// ---- mask / plane / threshold, ordered compaction, moments ----------------------------------------------------------
struct PcSelect { double prm[4]; int mode; int s[3]; };          // mode 0: DataInMask (prm = BB(1,:), Res), 1: StlAbovePlane (prm = P)

__device__ inline bool pc_selected(const PcSelect& sel, const float* __restrict__ pts, const double* __restrict__ d,
                                   const unsigned char* __restrict__ obs, long long i, double thresh, bool* flag) {
    const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    *flag = sel.mode == 0 ? pc::in_mask(x, y, z, sel.prm, sel.prm[3], obs, sel.s[0], sel.s[1], sel.s[2]) : pc::above_plane(x, y, z, sel.prm);
    return *flag && d[i] < thresh;
}

__global__ __launch_bounds__(PC_BLOCK) void pc_select_count_kernel(PcSelect sel, const float* __restrict__ pts, const double* __restrict__ d,
                                                                   const unsigned char* __restrict__ obs, int n, double thresh,
                                                                   unsigned char* __restrict__ flags, int* __restrict__ counts) {
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    bool f = false, s = false;
    if (i < n) { s = pc_selected(sel, pts, d, obs, i, thresh, &f); flags[i] = f; }
    const int c = __syncthreads_count(s);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(PC_BLOCK) void pc_select_scatter_kernel(PcSelect sel, const float* __restrict__ pts, const double* __restrict__ d,
                                                                     const unsigned char* __restrict__ obs, int n, double thresh,
                                                                     const int* __restrict__ offsets, double* __restrict__ out) {
    __shared__ int wave_base[PC_BLOCK / WAVE];
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    bool f = false;
    const bool s = i < n && pc_selected(sel, pts, d, obs, i, thresh, &f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(s);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_base[wave] = __popcll(b);
    __syncthreads();
    int base = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wave_base[w];
    if (s) out[base + before] = d[i];
}

// sum over a fixed tree: thread t takes x[t], x[t + T], ... (T = all threads of the launch), then the block halves down
__device__ inline double pc_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = PC_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// pass 0: sum of x; pass 1: sum of (x - mean)^2, mean = stats[1].  n = *count (on the device: no host round trip).
__global__ __launch_bounds__(PC_BLOCK) void pc_moment_kernel(const double* __restrict__ x, const int* __restrict__ count,
                                                             const double* __restrict__ stats, int pass, double* __restrict__ part) {
    __shared__ double sh[PC_BLOCK];
    const int n = *count;
    const double mean = pass ? stats[1] : 0.0;
    double s = 0.0;
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += PC_MOMENT_BLOCKS * PC_BLOCK) {
        const double v = pass ? (x[i] - mean) * (x[i] - mean) : x[i];
        s += v;
    }
    const double b = pc_block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

// stats = {n, mean, var (N - 1)}: MATLAB's mean / var, NaN for an empty set, var = 0 for one value
__global__ __launch_bounds__(64) void pc_moment_final_kernel(const double* __restrict__ part, const int* __restrict__ count, int pass,
                                                             double* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < PC_MOMENT_BLOCKS; ++b) s += part[b];
    const int n = *count;
    if (pass == 0) {
        stats[0] = (double)n;
        stats[1] = n > 0 ? s / (double)n : NAN;
    } else {
        stats[2] = n > 1 ? s / (double)(n - 1) : (n == 1 ? 0.0 : NAN);
    }
}


// ---- mesh super-sampling (MeshSupSamp) ------------------------------------------------------------------------------
constexpr int MS_BLOCK = 256;

// face t's triangle; false when an index lies outside 0 .. nv-1
__device__ inline bool ms_face(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int t, double dst, pc::SubTri* tri) {
    const int a = faces[(long long)t * 3 + 0], b = faces[(long long)t * 3 + 1], c = faces[(long long)t * 3 + 2];
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) return false;
    pc::subtri_setup(verts + (long long)a * 3, verts + (long long)b * 3, verts + (long long)c * 3, dst, tri);
    return true;
}

// *total += the block's sum of v (one atomic per block)
__device__ inline void ms_block_add(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = MS_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) atomicAdd(total, sh[0]);
}

// the last i in [lo, hi) with start[i] <= x (start non-decreasing, start[lo] <= x)
__device__ inline int ms_locate(const int* __restrict__ start, int lo, int hi, int x) {
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// tri_rows[t] = non-empty rows of face t (saturated to INT_MAX); totals[0] += the rows (each capped at 2^31), totals[1] += bad faces
__global__ __launch_bounds__(MS_BLOCK) void pc_mesh_rows_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int m,
                                                                double dst, int* __restrict__ tri_rows, unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long sh[MS_BLOCK];
    const int t = blockIdx.x * MS_BLOCK + threadIdx.x;
    long long rows = 0;
    bool bad = false;
    if (t < m) {
        pc::SubTri tri;
        if (ms_face(verts, nv, faces, t, dst, &tri)) rows = pc::subtri_rows(tri.n1, tri.n2);
        else bad = true;
        tri_rows[t] = (int)min(rows, (long long)INT_MAX);
    }
    const int nbad = __syncthreads_count(bad);
    ms_block_add((unsigned long long)rows, sh, &totals[0]);
    if (threadIdx.x == 0 && nbad) atomicAdd(&totals[1], (unsigned long long)nbad);
}

// row r (of face t = the last with tri_row_start[t] <= r, c1 = r - tri_row_start[t]): row_len[r] = its points; *total += them
__global__ __launch_bounds__(MS_BLOCK) void pc_mesh_row_len_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int m,
                                                                   double dst, const int* __restrict__ tri_row_start, int nrows,
                                                                   int* __restrict__ row_len, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long sh[MS_BLOCK];
    __shared__ int range[2];
    const int r0 = blockIdx.x * MS_BLOCK;
    const int r = r0 + threadIdx.x;
    if (threadIdx.x < 2) {
        const int x = threadIdx.x == 0 ? r0 : (int)min((long long)r0 + MS_BLOCK, (long long)nrows) - 1;
        range[threadIdx.x] = ms_locate(tri_row_start, 0, m, x);
    }
    __syncthreads();
    long long len = 0;
    if (r < nrows) {
        const int t = ms_locate(tri_row_start, range[0], range[1] + 1, r);
        pc::SubTri tri;
        if (ms_face(verts, nv, faces, t, dst, &tri)) len = pc::subtri_row_len((double)(r - tri_row_start[t]), tri.n1, tri.n2);
        row_len[r] = (int)min(len, (long long)INT_MAX);
    }
    ms_block_add((unsigned long long)len, sh, total);
}

// output point o < n_out: the vertex o, or sample s = o - nv of row r (the last with row_start[r] <= s, c2 = s - row_start[r])
__global__ __launch_bounds__(MS_BLOCK) void pc_mesh_emit_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int m,
                                                                double dst, const int* __restrict__ tri_row_start, const int* __restrict__ row_start,
                                                                int nrows, int n_out, float* __restrict__ out) {
    __shared__ int range[4];                                     // the block's first / last row, then their faces
    __shared__ float stage[3 * MS_BLOCK];
    const int o0 = blockIdx.x * MS_BLOCK;
    const int last = (int)min((long long)o0 + MS_BLOCK, (long long)n_out) - 1;
    const int o = o0 + threadIdx.x;
    if (threadIdx.x < 2 && last >= nv) {
        const int s = threadIdx.x == 0 ? max(o0 - nv, 0) : last - nv;
        const int r = ms_locate(row_start, 0, nrows, s);
        range[threadIdx.x] = r;
        range[2 + threadIdx.x] = ms_locate(tri_row_start, 0, m, r);
    }
    __syncthreads();
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (o <= last) {
        if (o < nv) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = verts[(long long)o * 3 + k];
        } else {
            const int s = o - nv;
            const int r = ms_locate(row_start, range[0], range[1] + 1, s);
            const int t = ms_locate(tri_row_start, range[2], range[3] + 1, r);
            pc::SubTri tri;
            if (ms_face(verts, nv, faces, t, dst, &tri)) {
                const double c1 = (double)(r - tri_row_start[t]), c2 = (double)(s - row_start[r]);
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = (float)pc::subtri_coord(tri, c1, c2, k);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = NAN;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) stage[threadIdx.x * 3 + k] = p[k];
    __syncthreads();
    const int nf = (last - o0 + 1) * 3;
    for (int i = threadIdx.x; i < nf; i += MS_BLOCK) out[(long long)o0 * 3 + i] = stage[i];
}

}  // namespace rcmvs

using namespace rcmvs;

extern "C" int rcmvs_pc_bbox(const float* pts, long long n, float* part, float* out, void* stream) {
    RCMVS_REQUIRE(pts && part && out, "pc_bbox: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_bbox: n=%lld (1 .. 2^31-1)", n);
    hipStream_t st = as_stream(stream);
    const int nblk = (int)min(cdiv(n, PC_BLOCK), (long long)PC_BBOX_BLOCKS);
    hipLaunchKernelGGL(pc_bbox_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, pts, (int)n, part);
    hipLaunchKernelGGL(pc_bbox_final_kernel, dim3(1), dim3(64), 0, st, part, nblk, out);
    return launch_status("pc_bbox");
}

static int pc_grid_from_host(const double* grid_host, const int* dims_host, PcGrid* g, const char* who) {
    RCMVS_REQUIRE(grid_host && dims_host, "%s: null grid description", who);
    for (int a = 0; a < 3; ++a) { g->o[a] = grid_host[a]; g->g[a] = dims_host[a]; }
    g->h = grid_host[3];
    RCMVS_REQUIRE(g->h > 0.0 && std::isfinite(g->h), "%s: cell edge %g", who, g->h);
    RCMVS_REQUIRE(g->g[0] >= 1 && g->g[1] >= 1 && g->g[2] >= 1 && (long long)g->g[0] * g->g[1] * g->g[2] <= RCMVS_PC_MAX_CELLS,
                  "%s: grid %d x %d x %d (at most %d cells)", who, g->g[0], g->g[1], g->g[2], RCMVS_PC_MAX_CELLS);
    return 0;
}

extern "C" int rcmvs_pc_grid_build(const float* pts, long long n, const double* grid_host, const int* dims_host, int* key, int* count,
                                   int* scan_work, int* cell_start, float* sorted, int* sorted_idx, void* stream) {
    RCMVS_REQUIRE(pts && key && count && scan_work && cell_start && sorted && sorted_idx, "pc_grid_build: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_grid_build: n=%lld (1 .. 2^31-1)", n);
    PcGrid g;
    if (int rc = pc_grid_from_host(grid_host, dims_host, &g, "pc_grid_build")) return rc;
    const int ncell = g.g[0] * g.g[1] * g.g[2];
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(n, PC_BLOCK);
    if (hipMemsetAsync(count, 0, sizeof(int) * ncell, st) != hipSuccess) return launch_status("pc_grid_build: memset");
    hipLaunchKernelGGL(pc_key_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, pts, (int)n, g, key, count);
    pc_scan(count, ncell, scan_work, cell_start, st);
    hipLaunchKernelGGL(pc_scatter_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, pts, (int)n, key, cell_start, count,
                       reinterpret_cast<float4*>(sorted), sorted_idx);
    return launch_status("pc_grid_build");
}

extern "C" int rcmvs_pc_nearest(const float* q, long long nq, const double* grid_host, const int* dims_host, const int* cell_start,
                                const float* sorted, long long n_to, double cap, const double* lattice_host, double* out, void* stream) {
    RCMVS_REQUIRE(q && out, "pc_nearest: null pointer");
    RCMVS_REQUIRE(nq > 0 && nq < (1ll << 31) && n_to >= 0 && n_to < (1ll << 31), "pc_nearest: nq=%lld n_to=%lld (below 2^31)", nq, n_to);
    RCMVS_REQUIRE(cap > 0.0 && std::isfinite(cap), "pc_nearest: cap %g", cap);
    PcGrid g = {};
    if (n_to > 0) {
        RCMVS_REQUIRE(cell_start && sorted, "pc_nearest: null grid");
        if (int rc = pc_grid_from_host(grid_host, dims_host, &g, "pc_nearest")) return rc;
    }
    PcLattice lat = {};
    if (lattice_host)
        for (int a = 0; a < 3; ++a) { lat.lo[a] = lattice_host[a]; lat.hi[a] = lattice_host[3 + a]; }
    hipLaunchKernelGGL(pc_nn_kernel, dim3((int)cdiv(nq, PC_BLOCK)), dim3(PC_BLOCK), 0, as_stream(stream), q, (int)nq, g, cell_start,
                       reinterpret_cast<const float4*>(sorted), (int)n_to, cap, lattice_host ? 1 : 0, lat, out);
    return launch_status("pc_nearest");
}

extern "C" int rcmvs_pc_reduce_init(const long long* order, const int* sorted_idx, long long n, int* rank, int* sorted_rank,
                                    unsigned char* state, void* stream) {
    RCMVS_REQUIRE(order && sorted_idx && rank && sorted_rank && state, "pc_reduce_init: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_reduce_init: n=%lld (1 .. 2^31-1)", n);
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(n, PC_BLOCK);
    hipLaunchKernelGGL(pc_rank_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, order, sorted_idx, (int)n, rank, sorted_rank, 0);
    hipLaunchKernelGGL(pc_rank_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, order, sorted_idx, (int)n, rank, sorted_rank, 1);
    if (hipMemsetAsync(state, pc::UNDECIDED, (size_t)n, st) != hipSuccess) return launch_status("pc_reduce_init: memset");
    return launch_status("pc_reduce_init");
}

extern "C" int rcmvs_pc_reduce_round(const double* grid_host, const int* dims_host, const int* cell_start, const float* sorted,
                                     const int* sorted_rank, const unsigned char* s_in, unsigned char* s_out, long long n, double dst,
                                     int* undecided, void* stream) {
    RCMVS_REQUIRE(cell_start && sorted && sorted_rank && s_in && s_out && undecided, "pc_reduce_round: null pointer");
    RCMVS_REQUIRE(s_in != s_out, "pc_reduce_round: the two state buffers must differ");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_reduce_round: n=%lld (1 .. 2^31-1)", n);
    PcGrid g;
    if (int rc = pc_grid_from_host(grid_host, dims_host, &g, "pc_reduce_round")) return rc;
    RCMVS_REQUIRE(dst > 0.0 && g.h >= dst, "pc_reduce_round: dst %g must be positive and at most the cell edge %g", dst, g.h);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(undecided, 0, sizeof(int), st) != hipSuccess) return launch_status("pc_reduce_round: memset");
    hipLaunchKernelGGL(pc_reduce_round_kernel, dim3((int)cdiv(n, PC_BLOCK)), dim3(PC_BLOCK), 0, st, g, cell_start,
                       reinterpret_cast<const float4*>(sorted), sorted_rank, s_in, s_out, (int)n, dst, undecided);
    return launch_status("pc_reduce_round");
}

extern "C" int rcmvs_pc_reduce_finish(const unsigned char* state, const int* sorted_idx, long long n, unsigned char* kept, void* stream) {
    RCMVS_REQUIRE(state && sorted_idx && kept, "pc_reduce_finish: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_reduce_finish: n=%lld (1 .. 2^31-1)", n);
    hipLaunchKernelGGL(pc_reduce_finish_kernel, dim3((int)cdiv(n, PC_BLOCK)), dim3(PC_BLOCK), 0, as_stream(stream), state, sorted_idx, (int)n, kept);
    return launch_status("pc_reduce_finish");
}

extern "C" int rcmvs_pc_select(const float* pts, const double* d, long long n, int mode, const double* params_host,
                               const unsigned char* obs_mask, int s1, int s2, int s3, double thresh, unsigned char* flags,
                               double* out, int* work, void* stream) {
    RCMVS_REQUIRE(pts && d && params_host && flags && out && work, "pc_select: null pointer");
    RCMVS_REQUIRE(n > 0 && n < (1ll << 31), "pc_select: n=%lld (1 .. 2^31-1)", n);
    RCMVS_REQUIRE(mode == 0 || mode == 1, "pc_select: mode %d (0 = DataInMask, 1 = StlAbovePlane)", mode);
    RCMVS_REQUIRE(mode == 1 || (obs_mask && s1 > 0 && s2 > 0 && s3 > 0 && params_host[3] > 0.0),
                  "pc_select: DataInMask needs the mask (%d x %d x %d) and Res > 0", s1, s2, s3);
    PcSelect sel = {};
    for (int k = 0; k < 4; ++k) sel.prm[k] = params_host[k];
    sel.mode = mode; sel.s[0] = s1; sel.s[1] = s2; sel.s[2] = s3;
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(n, PC_BLOCK);
    int* counts = work;
    int* offsets = work + nblk;
    int* bsum = offsets + nblk + 1;
    hipLaunchKernelGGL(pc_select_count_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, sel, pts, d, obs_mask, (int)n, thresh, flags, counts);
    pc_scan(counts, nblk, bsum, offsets, st);
    hipLaunchKernelGGL(pc_select_scatter_kernel, dim3(nblk), dim3(PC_BLOCK), 0, st, sel, pts, d, obs_mask, (int)n, thresh, offsets, out);
    return launch_status("pc_select");
}

extern "C" int rcmvs_pc_moments(const double* x, const int* count, double* part, double* stats, void* stream) {
    RCMVS_REQUIRE(x && count && part && stats, "pc_moments: null pointer");
    hipStream_t st = as_stream(stream);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(pc_moment_kernel, dim3(PC_MOMENT_BLOCKS), dim3(PC_BLOCK), 0, st, x, count, stats, pass, part);
        hipLaunchKernelGGL(pc_moment_final_kernel, dim3(1), dim3(64), 0, st, part, count, pass, stats);
    }
    return launch_status("pc_moments");
}

static int pc_mesh_args(const float* verts, long long nv, const int* faces, long long m, double dst, const char* who) {
    RCMVS_REQUIRE(verts && faces, "%s: null pointer", who);
    RCMVS_REQUIRE(nv > 0 && nv < (1ll << 31) && m > 0 && m < (1ll << 31), "%s: nv=%lld m=%lld (1 .. 2^31-1)", who, nv, m);
    RCMVS_REQUIRE(dst > 0.0 && std::isfinite(dst), "%s: dst %g", who, dst);
    return 0;
}

extern "C" int rcmvs_pc_mesh_rows(const float* verts, long long nv, const int* faces, long long m, double dst, int* tri_rows,
                                  unsigned long long* totals, void* stream) {
    if (int rc = pc_mesh_args(verts, nv, faces, m, dst, "pc_mesh_rows")) return rc;
    RCMVS_REQUIRE(tri_rows && totals, "pc_mesh_rows: null pointer");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(totals, 0, 3 * sizeof(unsigned long long), st) != hipSuccess) return launch_status("pc_mesh_rows: memset");
    hipLaunchKernelGGL(pc_mesh_rows_kernel, dim3((int)cdiv(m, MS_BLOCK)), dim3(MS_BLOCK), 0, st, verts, (int)nv, faces, (int)m, dst, tri_rows, totals);
    return launch_status("pc_mesh_rows");
}

extern "C" int rcmvs_pc_mesh_count(const float* verts, long long nv, const int* faces, long long m, double dst, const int* tri_rows,
                                   long long nrows, int* scan_work, int* tri_row_start, int* row_len, unsigned long long* totals,
                                   void* stream) {
    if (int rc = pc_mesh_args(verts, nv, faces, m, dst, "pc_mesh_count")) return rc;
    RCMVS_REQUIRE(tri_rows && scan_work && tri_row_start && row_len && totals, "pc_mesh_count: null pointer");
    RCMVS_REQUIRE(nrows > 0 && nv + nrows < (1ll << 31), "pc_mesh_count: %lld rows for %lld vertices (1 .. 2^31-1 points)", nrows, nv);
    hipStream_t st = as_stream(stream);
    pc_scan(tri_rows, (int)m, scan_work, tri_row_start, st);
    hipLaunchKernelGGL(pc_mesh_row_len_kernel, dim3((int)cdiv(nrows, MS_BLOCK)), dim3(MS_BLOCK), 0, st, verts, (int)nv, faces, (int)m, dst,
                       tri_row_start, (int)nrows, row_len, &totals[2]);
    return launch_status("pc_mesh_count");
}

extern "C" int rcmvs_pc_mesh_emit(const float* verts, long long nv, const int* faces, long long m, double dst, const int* tri_row_start,
                                  const int* row_len, long long nrows, long long n_samples, int* scan_work, int* row_start, float* out,
                                  void* stream) {
    if (int rc = pc_mesh_args(verts, nv, faces, m, dst, "pc_mesh_emit")) return rc;
    RCMVS_REQUIRE(tri_row_start && row_len && scan_work && row_start && out, "pc_mesh_emit: null pointer");
    RCMVS_REQUIRE(nrows > 0 && n_samples >= nrows && nv + n_samples < (1ll << 31),
                  "pc_mesh_emit: %lld samples in %lld rows for %lld vertices (at most 2^31-1 points)", n_samples, nrows, nv);
    hipStream_t st = as_stream(stream);
    pc_scan(row_len, (int)nrows, scan_work, row_start, st);
    const long long n_out = nv + n_samples;
    hipLaunchKernelGGL(pc_mesh_emit_kernel, dim3((int)cdiv(n_out, MS_BLOCK)), dim3(MS_BLOCK), 0, st, verts, (int)nv, faces, (int)m, dst,
                       tri_row_start, row_start, (int)nrows, (int)n_out, out);
    return launch_status("pc_mesh_emit");
}
