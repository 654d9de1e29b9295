/* C ABI of the block-sparse TSDF volume in librcmvs_hip.so (an extension header of include/rcmvs.h like tsdf_mesh.h, whose
 * conventions and per-voxel contract it keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*). */
#ifndef RCMVS_TSDF_SPARSE_H
#define RCMVS_TSDF_SPARSE_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- depth maps -> triangle mesh of a large scene (rc_mvsnet_amd/tsdf_mesh.py SparseTsdfVolume; csrc/tsdf_sparse.hip; additive,
 * RCMVS_VERSION stays 106) ----
 * The virtual grid: grid_host = {ox, oy, oz, h} (HOST, 4 doubles), bdims_host = {bx, by, bz} (HOST, 3 ints) counts blocks of
 * RCMVS_TSDF_SP_BLOCK^3 voxels, bx * by * bz <= RCMVS_TSDF_SP_MAX_BLOCKS; block (X, Y, Z) has the number B = X + bx * (Y + by * Z);
 * voxel (i, j, k) of the 8 bx x 8 by x 8 bz voxels has the centre o + (idx + 0.5) * h, exactly as in the dense grid of tsdf_mesh.h.
 * Only marked blocks are allocated: mark sets flags, build turns them into a bit mask with ranks, and a block's slot is
 * word_rank[B >> 5] + popcount(mask_words[B >> 5] & lower bits) -- no hash table.  Allocated voxel number: slot * 512 + lx + 8 *
 * (ly + 8 * lz).  The planes (dsum, wsum, optionally three colour sums) hold n_active * 512 fp32 each, zero-filled by the caller.
 * Per voxel everything is csrc/tsdf_mesh_math.h's arithmetic: a voxel's planes equal the dense kernel's planes of the same voxel in
 * a dense grid of 8 * bdims in every bit, and with no skipped pixel the mesh is the dense mesh in another order (the covering
 * argument is in DESIGN.md).  The marking rule is csrc/tsdf_sparse_math.h's; tests/tsdf_sparse_oracle.py restates it. */
#define RCMVS_TSDF_SP_BLOCK 8
#define RCMVS_TSDF_SP_MAX_BLOCKS (1 << 27)
#define RCMVS_TSDF_SP_MAX_ACTIVE (1 << 19)
#define RCMVS_TSDF_SP_MARK_SPAN 4
#define RCMVS_TSDF_SP_SCAN_TILE 2048

/* Marks the blocks that the truncation slabs of n views' depth pixels touch (1 .. RCMVS_TSDF_MAX_VIEWS per call; any number of
 * calls).  depth: DEVICE (n, H, W) fp32, cams_host as in rcmvs_tsdf_integrate.  Per pixel (column i, row j), fp64 in this order:
 * d finite and > 0 or nothing is marked; z0 = max(d - trunc, 0) (0 unless > 0), z1 = d + trunc; the eight corners z in {z0, z1},
 * a = i -+ 0.5, b = j -+ 0.5: xc = ((a - cx) / fx) * z, yc = ((b - cy) / fy) * z, q = (xc - t0, yc - t1, z - t2), world w_k =
 * (R[0][k] q0 + R[1][k] q1) + R[2][k] q2; lo_k = min - h, hi_k = max + h; any of them not finite: the pixel is skipped and counted;
 * bl_k = floor((lo_k - o_k) / (8 h)), bh_k likewise, compared in fp64; a range wholly outside [0, bdim_k) marks nothing (not
 * counted); else clamped; longer than RCMVS_TSDF_SP_MARK_SPAN on an axis: skipped and counted; else every block of the range gets
 * flags[B] = 1 (a plain byte store; every writer stores the same value).  flags: DEVICE, bx * by * bz bytes, zero-filled by the
 * caller before the first call.  skipped: DEVICE, one uint64 that accumulates over calls.  No input makes the kernel write outside
 * flags.  H, W, trunc, grid and cameras as rcmvs_tsdf_integrate demands them. */
int rcmvs_tsdf_sp_mark(const float* depth, int n, int H, int W, const double* cams_host, double trunc, const double* grid_host,
                       const int* bdims_host, unsigned char* flags, unsigned long long* skipped, void* stream);
int rcmvs_tsdf_sp_mark_timed(const float* depth, int n, int H, int W, const double* cams_host, double trunc, const double* grid_host,
                             const int* bdims_host, unsigned char* flags, unsigned long long* skipped, void* ev0, void* ev1, void* stream);

/* flags (non-zero = active) -> mask_words (DEVICE, words = ceil(blocks / 32) uint32, bit B & 31 of word B >> 5), word_rank (DEVICE,
 * words + 1 uint32: the number of set bits before each word, and the total last) and active (DEVICE, the numbers of the set blocks
 * ascending; only the first active_capacity are written).  scan_work: DEVICE, ceil(words / RCMVS_TSDF_SP_SCAN_TILE) ints.  The
 * caller reads the total and refuses 0 and more than RCMVS_TSDF_SP_MAX_ACTIVE before it allocates the planes. */
int rcmvs_tsdf_sp_build(const unsigned char* flags, const int* bdims_host, unsigned int* mask_words, unsigned int* word_rank, int* active,
                        int active_capacity, int* scan_work, void* stream);
int rcmvs_tsdf_sp_build_timed(const unsigned char* flags, const int* bdims_host, unsigned int* mask_words, unsigned int* word_rank, int* active,
                              int active_capacity, int* scan_work, void* ev0, void* ev1, void* stream);

/* rcmvs_tsdf_integrate on the allocated voxels: one workgroup per active block, the state in registers, one fp32 add per view in
 * view order, no atomics; chunking the views over calls does not change a bit.  active: DEVICE, n_active block numbers as build
 * wrote them (1 .. RCMVS_TSDF_SP_MAX_ACTIVE); an entry outside the grid is ignored. */
int rcmvs_tsdf_sp_integrate(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                            const double* grid_host, const int* bdims_host, const int* active, int n_active, float* dsum, float* wsum,
                            float* csum_r, float* csum_g, float* csum_b, void* stream);
int rcmvs_tsdf_sp_integrate_timed(const float* depth, const unsigned char* rgb, int n, int H, int W, const double* cams_host, double trunc,
                                  const double* grid_host, const int* bdims_host, const int* active, int n_active, float* dsum, float* wsum,
                                  float* csum_r, float* csum_g, float* csum_b, void* ev0, void* ev1, void* stream);

/* rcmvs_tsdf_mesh_count read through the block table: a voxel in an inactive block or beyond the grid is unobserved.  edge_mask,
 * tri_count (DEVICE bytes), vert_start, tri_start (DEVICE ints, + 1) are indexed by the allocated voxel number, n_active * 512 of
 * them; totals = {vertices, triangles} (DEVICE, 2 uint64, exact).  scan_work: DEVICE, 1024 + 2 * n_active ints, 8-byte aligned (a
 * two-level scan of the blocks' sums: tiles of RCMVS_TSDF_SP_SCAN_TILE blocks, at most 256 tile sums in 64 bits). */
int rcmvs_tsdf_sp_mesh_count(const float* dsum, const float* wsum, const int* bdims_host, const unsigned int* mask_words,
                             const unsigned int* word_rank, const int* active, int n_active, int min_weight, unsigned char* edge_mask,
                             unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals, void* stream);
int rcmvs_tsdf_sp_mesh_count_timed(const float* dsum, const float* wsum, const int* bdims_host, const unsigned int* mask_words,
                                   const unsigned int* word_rank, const int* active, int n_active, int min_weight, unsigned char* edge_mask,
                                   unsigned char* tri_count, int* scan_work, int* vert_start, int* tri_start, unsigned long long* totals,
                                   void* ev0, void* ev1, void* stream);

/* rcmvs_tsdf_mesh_emit read through the block table.  Vertices are ordered by (allocated voxel number, edge code), faces by
 * (allocated number of the cube's voxel, tetrahedron, triangle); a face finds a vertex through its owner's allocated number, and
 * the owner may sit in a neighbouring block.  Positions, colours and orientation as in the dense contract. */
int rcmvs_tsdf_sp_mesh_emit(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                            const double* grid_host, const int* bdims_host, const unsigned int* mask_words, const unsigned int* word_rank,
                            const int* active, int n_active, int min_weight, const unsigned char* edge_mask, const unsigned char* tri_count,
                            const int* vert_start, const int* tri_start, long long nv, long long nf, float* verts, unsigned char* vert_rgb,
                            int* faces, void* stream);
int rcmvs_tsdf_sp_mesh_emit_timed(const float* dsum, const float* wsum, const float* csum_r, const float* csum_g, const float* csum_b,
                                  const double* grid_host, const int* bdims_host, const unsigned int* mask_words, const unsigned int* word_rank,
                                  const int* active, int n_active, int min_weight, const unsigned char* edge_mask, const unsigned char* tri_count,
                                  const int* vert_start, const int* tri_start, long long nv, long long nf, float* verts, unsigned char* vert_rgb,
                                  int* faces, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_TSDF_SPARSE_H */
