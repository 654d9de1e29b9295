/* C ABI of mesh decimation in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_clean.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, *_timed twins whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop, refusals that write nothing; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_DECIMATE_H
#define RCMVS_MESH_DECIMATE_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> a coarser one by vertex clustering on a regular lattice, one vertex per occupied cell placed by the
 * cluster's quadric (Lindstrom's out-of-core simplification) or at the members' mean (rc_mvsnet_amd/mesh_decimate.py;
 * csrc/mesh_decimate.hip; the per-element rules and their operation order are csrc/mesh_decimate_math.h's, restated by
 * tests/mesh_decimate_oracle.py) ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE; 0 <= nv <= RCMVS_MD_MAX_ELEMENTS,
 * 0 <= 3 nf <= RCMVS_MD_MAX_ELEMENTS, and a pointer to an array of no elements may be NULL.  A face is VALID by mesh_clean.h's
 * rule (indices in [0, nv), distinct); no index of an invalid face is used as an address.  Every output is a function of the
 * inputs alone: the sorts are stable LSD radix sorts, the fp64 sums run in a fixed order in one thread, and atomics only add
 * integers, take integer minima / maxima, or claim slots of a hash table whose contents do not reach any output (DESIGN.md,
 * "Mesh decimation").  There are no floating-point atomics.
 * Scans run in three levels over tiles of RCMVS_MD_SCAN_TILE elements.  scan_work: DEVICE, 8-byte aligned,
 * RCMVS_MD_SCAN_WORK + ceil(n / RCMVS_MD_SCAN_TILE) + 1 ints for the longest array n the call scans.
 * A radix sort of n (key, index) pairs takes 8 bits a pass over blocks of RCMVS_MD_SORT_BLOCK pairs, between two key buffers and
 * two index buffers of n entries each (either may hold the result; the entry points copy what they return out of them), with
 * hist and hist_start: DEVICE 256 * ceil(n / RCMVS_MD_SORT_BLOCK) and one more ints, and a scan_work for that length. */
#define RCMVS_MD_SCAN_TILE 2048
#define RCMVS_MD_SCAN_WORK 2048
#define RCMVS_MD_SORT_BLOCK 256
#define RCMVS_MD_MAX_ELEMENTS 2147483392
#define RCMVS_MD_MAX_CELLS_PER_AXIS (1 << 21)
/* face_class values, the first rule that applies */
#define RCMVS_MD_FACE_KEPT 0
#define RCMVS_MD_FACE_INVALID 1
#define RCMVS_MD_FACE_UNCLUSTERED 2
#define RCMVS_MD_FACE_COLLAPSED 3
#define RCMVS_MD_FACE_DUPLICATE 4
/* placement, and how a cluster's position was chosen (via) */
#define RCMVS_MD_PLACE_QUADRIC 0
#define RCMVS_MD_PLACE_MEAN 1
#define RCMVS_MD_VIA_QUADRIC 0
#define RCMVS_MD_VIA_NO_FACES 1
#define RCMVS_MD_VIA_SINGULAR 2
#define RCMVS_MD_VIA_OUTSIDE 3
#define RCMVS_MD_VIA_MEAN 4

/* The bounding box of the vertices whose three coordinates are finite.  bounds: DEVICE 8 uint32 = {min x, y, z, max x, y, z as
 * md::ordered keys (integer-ordered, -0.0 below +0.0; 0xffffffff / 0 where there is no such vertex), the number of such
 * vertices, 0}. */
int rcmvs_md_bounds(const float* verts, int nv, unsigned* bounds, void* stream);
int rcmvs_md_bounds_timed(const float* verts, int nv, unsigned* bounds, void* ev0, void* ev1, void* stream);

/* The lattice of a box, on the HOST (no launch): lohi_host = {min x, y, z, max x, y, z} fp32, all finite, min <= max;
 * cell > 0 finite.  lattice_host: 4 doubles = {origin x, y, z = (double)min - cell / 2, cell}; dims_host: 3 long long,
 * g = floor(((double)max - origin) / cell) + 1.  Refused, naming the axis, when a g is not in 1 .. RCMVS_MD_MAX_CELLS_PER_AXIS. */
int rcmvs_md_lattice(const float* lohi_host, double cell, double* lattice_host, long long* dims_host);

/* Clusters.  A vertex is CLUSTERED when its coordinates are finite and its cell k = floor(((double)p - origin) / cell) lies in
 * [0, g) on every axis (every finite vertex, for the lattice of the vertices' own box); its key is (kz gy + ky) gx + kx.  The
 * clusters are the occupied cells, numbered in ascending key order; unclustered vertices sort behind them under the key
 * gx gy gz.  The sort takes ceil(bits(gx gy gz) / 8) passes, at least one.
 * cluster: DEVICE nv ints, the vertex's cluster or -1.  order: DEVICE nv ints, the vertices sorted by (key, vertex number).
 * cluster_start: DEVICE nv + 1 ints, cluster r's members are order[cluster_start[r] .. cluster_start[r + 1]), ascending vertex
 * numbers; entries 0 .. m are written.  cluster_key: DEVICE nv uint64, entries 0 .. m - 1 are written.  head: DEVICE nv bytes,
 * head_rank: DEVICE nv + 1 ints (work).  totals: DEVICE 2 uint64 = {m, the number of clustered vertices}. */
int rcmvs_md_cluster(const float* verts, int nv, const double* lattice_host, const long long* dims_host, unsigned long long* key_a, int* idx_a,
                     unsigned long long* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, unsigned char* head, int* head_rank,
                     int* cluster, int* order, int* cluster_start, unsigned long long* cluster_key, unsigned long long* totals, void* stream);
int rcmvs_md_cluster_timed(const float* verts, int nv, const double* lattice_host, const long long* dims_host, unsigned long long* key_a,
                           int* idx_a, unsigned long long* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, unsigned char* head,
                           int* head_rank, int* cluster, int* order, int* cluster_start, unsigned long long* cluster_key,
                           unsigned long long* totals, void* ev0, void* ev1, void* stream);

/* Faces.  cface: DEVICE nf * 3 ints, the clusters (ca, cb, cc) of a valid face's vertices, (-1, -1, -1) for an invalid face.
 * face_class: DEVICE nf bytes: INVALID; else UNCLUSTERED when one of the three is -1; else COLLAPSED when two of them are equal;
 * else DUPLICATE when a face of lower number, itself neither of these, maps to the same triple up to rotation ((a, b, c) and
 * (a, c, b) differ); else KEPT.  counts: DEVICE 4 uint64 = {invalid, unclustered, collapsed, duplicate}.
 * table: DEVICE table_capacity ints (work), table_capacity a power of two > nf: an open-addressing hash table of face numbers
 * keyed by the rotated triple.  A triple always ends in the one slot its probe sequence reaches first, whatever the order of
 * the insertions, and that slot ends with the smallest face number of the triple (atomicMin). */
int rcmvs_md_classify_faces(const int* faces, int nv, int nf, const int* cluster, int* cface, unsigned char* face_class, int* table,
                            long long table_capacity, unsigned long long* counts, void* stream);
int rcmvs_md_classify_faces_timed(const int* faces, int nv, int nf, const int* cluster, int* cface, unsigned char* face_class, int* table,
                                  long long table_capacity, unsigned long long* counts, void* ev0, void* ev1, void* stream);

/* Cluster quadrics.  Every corner e = 3 f + c of every valid face whose three vertices are clustered (collapsed and duplicate
 * faces included) contributes md::add_corner of the face, taken in the frame of cluster[faces[e]] (centre = origin + (k + 0.5)
 * cell, units of the cell), to that cluster.  quad: DEVICE m * 9 doubles = {A00 A01 A02 A11 A12 A22 b0 b1 b2} per cluster, the
 * fp64 sums of its corners' contributions from 0.0 in ascending e: a stable sort of the 3 nf (cluster, e) pairs (32-bit keys,
 * ceil(bits(m) / 8) passes, other corners behind under the key m) and one thread per cluster walking its segment.
 * m: the number of clusters, 1 <= m <= nv.  ckey_a / ckey_b: DEVICE 3 nf uint32, cidx_a / cidx_b: DEVICE 3 nf ints, hist /
 * hist_start / scan_work for 3 nf pairs; seg: DEVICE 2 m ints (work). */
int rcmvs_md_quadrics(const float* verts, const int* faces, int nv, int nf, const int* cluster, const unsigned long long* cluster_key, int m,
                      const double* lattice_host, const long long* dims_host, unsigned* ckey_a, int* cidx_a, unsigned* ckey_b, int* cidx_b,
                      int* hist, int* hist_start, int* scan_work, int* seg, double* quad, void* stream);
int rcmvs_md_quadrics_timed(const float* verts, const int* faces, int nv, int nf, const int* cluster, const unsigned long long* cluster_key,
                            int m, const double* lattice_host, const long long* dims_host, unsigned* ckey_a, int* cidx_a, unsigned* ckey_b,
                            int* cidx_b, int* hist, int* hist_start, int* scan_work, int* seg, double* quad, void* ev0, void* ev1,
                            void* stream);

/* Positions and colours, one thread per cluster.  mean = the members' md::local coordinates added from 0.0 in ascending vertex
 * order, divided once by their number.  placement QUADRIC: md::solve(quad, mean, reg) and, when it answers VIA_QUADRIC,
 * out_verts = md::world(centre, cell, x); otherwise, and always under placement MEAN (quad may be NULL), the mean is taken:
 * md::world(centre, cell, mean), except that a cluster of ONE member takes that member's coordinates in every bit (a copy, no
 * arithmetic).  via: DEVICE m bytes, the RCMVS_MD_VIA_* value.  out_rgb (with rgb, or both NULL): md::colour of the members'
 * integer channel sums.  counts: DEVICE 3 uint64 = {VIA_NO_FACES, VIA_SINGULAR, VIA_OUTSIDE clusters}.  A cluster whose segment
 * does not lie inside order, or with a member outside [0, nv), is not written.  reg >= 0 finite. */
int rcmvs_md_place(const float* verts, const unsigned char* rgb, int nv, const int* order, const int* cluster_start,
                   const unsigned long long* cluster_key, int m, const double* lattice_host, const long long* dims_host, const double* quad,
                   int placement, double reg, float* out_verts, unsigned char* out_rgb, unsigned char* via, unsigned long long* counts,
                   void* stream);
int rcmvs_md_place_timed(const float* verts, const unsigned char* rgb, int nv, const int* order, const int* cluster_start,
                         const unsigned long long* cluster_key, int m, const double* lattice_host, const long long* dims_host,
                         const double* quad, int placement, double reg, float* out_verts, unsigned char* out_rgb, unsigned char* via,
                         unsigned long long* counts, void* ev0, void* ev1, void* stream);

/* What the output keeps, in the form rcmvs_mc_gather takes (mesh_clean.h; called with cface as the faces and the m cluster
 * vertices): face_keep: DEVICE nf bytes, 1 for a KEPT face; vert_keep: DEVICE m bytes, 1 for a cluster a kept face uses
 * (drop_unreferenced != 0) or for every cluster (== 0); face_rank / vert_rank: DEVICE nf + 1 / m + 1 ints, their exclusive prefix
 * sums, the totals last.  totals: DEVICE 2 uint64 = {faces kept, clusters kept}. */
int rcmvs_md_select(const int* cface, const unsigned char* face_class, int m, int nf, int drop_unreferenced, unsigned char* face_keep,
                    unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, unsigned long long* totals, void* stream);
int rcmvs_md_select_timed(const int* cface, const unsigned char* face_class, int m, int nf, int drop_unreferenced, unsigned char* face_keep,
                          unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, unsigned long long* totals, void* ev0,
                          void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_DECIMATE_H */
