/* C ABI of the mesh clean-up pass in librcmvs_hip.so (an extension header of include/rcmvs.h like tsdf_sparse.h, whose conventions
 * it keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, *_timed twins whose ev0 / ev1 receive
 * the first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_CLEAN_H
#define RCMVS_MESH_CLEAN_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> its connected components, a compacted copy, its 1-ring, Taubin smoothing (rc_mvsnet_amd/mesh_clean.py;
 * csrc/mesh_clean.hip; the per-element rules are csrc/mesh_clean_math.h's, restated by tests/mesh_clean_oracle.py) ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE, as TsdfVolume.extract returns
 * them; 0 <= nv, nf < 2^31, and a pointer to an array of no elements may be NULL.  A face is VALID when its three indices lie in
 * [0, nv) and differ; every kernel tests this itself and uses no index of an invalid face as an address, so no faces array makes
 * a kernel read or write outside its buffers.  Every output is a function of the inputs alone: atomics only add integers, take
 * integer maxima, hand out slots of a segment that is sorted afterwards, or link union-find roots whose final minimum does not
 * depend on the order ("Mesh clean-up").
 * Scans run in three levels over tiles of RCMVS_MC_SCAN_TILE elements.  scan_work: DEVICE, 8-byte aligned,
 * RCMVS_MC_SCAN_WORK + ceil(n / RCMVS_MC_SCAN_TILE) + 1 ints for the longest array n the call scans. */
#define RCMVS_MC_SCAN_TILE 2048
#define RCMVS_MC_SCAN_WORK 2048
#define RCMVS_MC_SORT_LIMIT 48
#define RCMVS_MC_MAX_ENTRIES 2147483647

/* Validation and connected components.  Two vertices are connected when a valid face holds both.  label: DEVICE nv ints,
 * label[v] = the smallest vertex number of v's component (v itself for a vertex no valid face uses).  face_ok: DEVICE nf bytes,
 * 1 = valid.  comp_faces: DEVICE nv ints, at a label the number of valid faces whose FIRST index carries that label, 0 elsewhere.
 * counts: DEVICE 4 uint64 = {invalid faces, 0, 0, 0}.  Union-find on label[]: hooking by atomicCAS of the larger root under the
 * smaller, path halving, then a flatten pass. */
int rcmvs_mc_components(const int* faces, int nv, int nf, int* label, unsigned char* face_ok, int* comp_faces, unsigned long long* counts,
                        void* stream);
int rcmvs_mc_components_timed(const int* faces, int nv, int nf, int* label, unsigned char* face_ok, int* comp_faces,
                              unsigned long long* counts, void* ev0, void* ev1, void* stream);

/* The components that own at least one valid face, one row {label, faces} each, ascending by label: table, DEVICE capacity * 2 ints
 * (only the first `capacity` rows are written; min(nv, nf) always suffices).  flags: DEVICE nv bytes, rank: DEVICE nv + 1 ints (work).
 * totals: DEVICE 2 uint64 = {rows, the largest faces value}. */
int rcmvs_mc_component_table(const int* label, const int* comp_faces, int nv, unsigned char* flags, int* rank, int* scan_work, int* table,
                             int capacity, unsigned long long* totals, void* stream);
int rcmvs_mc_component_table_timed(const int* label, const int* comp_faces, int nv, unsigned char* flags, int* rank, int* scan_work,
                                   int* table, int capacity, unsigned long long* totals, void* ev0, void* ev1, void* stream);

/* Selection.  A component of faces_c faces and label l is kept when faces_c >= min_faces, (double)faces_c >= min_fraction *
 * (double)max_faces, and, with keep_largest > 0, faces_c > k_faces or (faces_c == k_faces and l <= k_label): (k_faces, k_label) is
 * the keep_largest-th row of the table ordered by (faces descending, label ascending), which the caller reads from the table.
 * face_keep: DEVICE nf bytes, 1 for a valid face whose first index's component is kept.  vert_keep: DEVICE nv bytes, 1 for a vertex
 * of a kept face (drop_unreferenced != 0) or for every vertex (== 0).  face_rank / vert_rank: DEVICE nf + 1 / nv + 1 ints, the
 * exclusive prefix sums of the two, the totals last.  totals: DEVICE 3 uint64 = {faces kept, vertices kept, components kept}.
 * min_faces, keep_largest >= 0; min_fraction finite. */
int rcmvs_mc_select(const int* faces, const unsigned char* face_ok, const int* label, const int* comp_faces, int nv, int nf, int min_faces,
                    double min_fraction, int max_faces, int keep_largest, int k_faces, int k_label, int drop_unreferenced,
                    unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work,
                    unsigned long long* totals, void* stream);
int rcmvs_mc_select_timed(const int* faces, const unsigned char* face_ok, const int* label, const int* comp_faces, int nv, int nf,
                          int min_faces, double min_fraction, int max_faces, int keep_largest, int k_faces, int k_label,
                          int drop_unreferenced, unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank,
                          int* scan_work, unsigned long long* totals, void* ev0, void* ev1, void* stream);

/* Compaction: kept vertices and kept faces in input order; out_verts / out_rgb (nv_out rows, out_rgb with rgb or both NULL) are
 * copies in every bit, out_faces (nf_out rows) holds vert_rank of the old indices.  A rank outside the output is not written. */
int rcmvs_mc_gather(const float* verts, const unsigned char* rgb, const int* faces, const unsigned char* face_keep, const int* face_rank,
                    const unsigned char* vert_keep, const int* vert_rank, int nv, int nf, int nv_out, int nf_out, float* out_verts,
                    unsigned char* out_rgb, int* out_faces, void* stream);
int rcmvs_mc_gather_timed(const float* verts, const unsigned char* rgb, const int* faces, const unsigned char* face_keep,
                          const int* face_rank, const unsigned char* vert_keep, const int* vert_rank, int nv, int nf, int nv_out, int nf_out,
                          float* out_verts, unsigned char* out_rgb, int* out_faces, void* ev0, void* ev1, void* stream);

/* The 1-ring in CSR form, without a global sort.  Every valid face (a, b, c) contributes the six directed entries a->b, a->c,
 * b->a, b->c, c->a, c->b; 6 * nf <= RCMVS_MC_MAX_ENTRIES.  row_start: DEVICE nv + 1 ints, the exclusive prefix sums of the entry
 * counts.  Vertex v's segment nbr[row_start[v] .. row_start[v + 1]) (DEVICE 6 * nf ints) holds its row_len[v] (DEVICE nv ints)
 * distinct neighbours ascending, then -1; mult (DEVICE 6 * nf ints) holds next to each neighbour w the number of valid faces on the
 * edge {v, w}, then 0.  on_boundary: DEVICE nv bytes, 1 when an edge at v has multiplicity 1.  A segment of at most
 * RCMVS_MC_SORT_LIMIT entries is sorted by one lane in LDS; a longer one by a workgroup (odd-even transposition, any length).
 * cursor: DEVICE nv ints (work).  heavy: DEVICE heavy_capacity ints (work), heavy_capacity >= 6 * nf / (RCMVS_MC_SORT_LIMIT + 1) + 1.
 * stats: DEVICE 6 uint64 = {undirected edges, edges of multiplicity 1, edges of multiplicity > 2, vertices with a neighbour,
 * segments on the long path, entries}. */
int rcmvs_mc_adjacency(const int* faces, int nv, int nf, int* row_start, int* row_len, int* nbr, int* mult, unsigned char* on_boundary,
                       int* cursor, int* heavy, int heavy_capacity, int* scan_work, unsigned long long* stats, void* stream);
int rcmvs_mc_adjacency_timed(const int* faces, int nv, int nf, int* row_start, int* row_len, int* nbr, int* mult, unsigned char* on_boundary,
                             int* cursor, int* heavy, int heavy_capacity, int* scan_work, unsigned long long* stats, void* ev0, void* ev1,
                             void* stream);

/* One Jacobi step of Taubin smoothing with the factor f (lambda or mu): dst[v] = src[v] in every bit for a vertex with
 * row_len[v] < 1 or pinned[v] != 0 (pinned may be NULL: nothing pinned); otherwise per coordinate in fp64 s = 0.0 + the
 * neighbours' coordinates in segment order, m = s / row_len[v], dst = (float)((double)src + f * (m - (double)src)).  NaN and
 * infinities propagate by IEEE rules; no branch looks at a coordinate.  entries: the length of nbr; a segment that does not lie
 * inside it, or a neighbour outside [0, nv), leaves the vertex unchanged.  src and dst (DEVICE nv * 3 fp32) must not overlap.
 * f finite. */
int rcmvs_mc_taubin_step(const float* src, float* dst, int nv, const int* row_start, const int* row_len, const int* nbr, long long entries,
                         const unsigned char* pinned, double f, void* stream);
int rcmvs_mc_taubin_step_timed(const float* src, float* dst, int nv, const int* row_start, const int* row_len, const int* nbr,
                               long long entries, const unsigned char* pinned, double f, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_CLEAN_H */
