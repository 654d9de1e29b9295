/* C ABI of mesh simplification in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_decimate.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, *_timed twins whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop, refusals that write nothing; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_SIMPLIFY_H
#define RCMVS_MESH_SIMPLIFY_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> a coarser one by quadric edge collapse, one independent set of edges a round (rc_mvsnet_amd/
 * mesh_simplify.py; csrc/mesh_simplify.hip; the per-element rules and their operation order are csrc/mesh_simplify_math.h's,
 * restated by tests/mesh_simplify_oracle.py; the rule and the independence argument: DESIGN.md, "Mesh simplification") ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE; 0 <= nv, 6 nf <=
 * RCMVS_MC_MAX_ENTRIES and 3 nf <= RCMVS_MS_MAX_CORNERS, and a pointer to an array of no elements may be NULL.  A face is VALID by
 * mesh_clean.h's rule (indices in [0, nv), distinct); no index of an invalid face is used as an address.  Every output is a
 * function of the inputs alone: the sorts are stable LSD radix sorts, every fp64 sum runs in a fixed order in one thread, the set
 * of edges a round collapses is decided by integer minima that one lane takes over a sorted segment, and atomics only add
 * integers or take an integer maximum.  There are no floating-point atomics.
 * One lane serves an edge, and one lane walks a vertex's ring or its corners: a vertex of very high valence is slow, not wrong.
 * Vertices on the rim, on non-manifold edges and with non-finite coordinates are LOCKED: they keep their position in every bit
 * and are never removed, so those parts of a mesh stay at full resolution.  A colour is the mean of the merged vertices'
 * colours, not an attribute of the quadric.
 * Work areas as in mesh_decimate.h: scan_work holds RCMVS_MS_SCAN_WORK + ceil(n / RCMVS_MS_SCAN_TILE) + 1 ints for the longest
 * array the call scans (6 nf flags, nv counts, or the sort's 256 ceil(3 nf / RCMVS_MS_SORT_BLOCK) table), 8-byte aligned; key_a /
 * key_b: 3 nf uint32, idx_a / idx_b: 3 nf ints, hist / hist_start: 256 ceil(3 nf / RCMVS_MS_SORT_BLOCK) and one more ints. */
#define RCMVS_MS_SCAN_TILE 2048
#define RCMVS_MS_SCAN_WORK 2048
#define RCMVS_MS_SORT_BLOCK 256
#define RCMVS_MS_MAX_CORNERS 2147483392
#define RCMVS_MS_QUADRIC_DOUBLES 10
/* how an edge's target was chosen */
#define RCMVS_MS_PATH_LOCKED 0
#define RCMVS_MS_PATH_QUADRIC 1
#define RCMVS_MS_PATH_MIDPOINT 2
#define RCMVS_MS_PATH_END_U 3
#define RCMVS_MS_PATH_END_V 4
/* an edge's state: a candidate, the first reason that rejects it, or no candidate at all */
#define RCMVS_MS_EDGE_OK 0
#define RCMVS_MS_EDGE_COST 1
#define RCMVS_MS_EDGE_LINK 2
#define RCMVS_MS_EDGE_FLIP 3
#define RCMVS_MS_EDGE_NONE 255
/* the counters of a round */
#define RCMVS_MS_COUNTS 16
#define RCMVS_MS_COUNT_LOCKED 0
#define RCMVS_MS_COUNT_CANDIDATES 1
#define RCMVS_MS_COUNT_REJECT_COST 2
#define RCMVS_MS_COUNT_REJECT_LINK 3
#define RCMVS_MS_COUNT_REJECT_FLIP 4
#define RCMVS_MS_COUNT_PATH 5
#define RCMVS_MS_COUNT_SELECTED 10
#define RCMVS_MS_COUNT_APPLIED 11
#define RCMVS_MS_COUNT_MAX_COST 12
#define RCMVS_MS_COUNT_LIVE 13
#define RCMVS_MS_COUNT_LIVE_BEFORE 14

/* The state a call carries from round to round.  frame_host: HOST 4 doubles = {centre x, y, z, side} of ms::centre / ms::side over
 * the box of rcmvs_md_bounds; side > 0, all finite.  quad: DEVICE nv * 10 doubles = {A00 A01 A02 A11 A12 A22 b0 b1 b2 c} per
 * vertex: the fp64 sum from 0.0, in ascending 3 face + corner, of ms::add_corner over the vertex's corners in the valid faces whose
 * nine coordinates are finite (the face's plane weighted by four times its squared area, frame coordinates).  members: DEVICE nv
 * ints = 1.  csum (with rgb, or both NULL): DEVICE nv * 3 uint64 = the vertex's colour.  live: DEVICE 1 uint64 = the valid faces.
 * stats: DEVICE 4 uint64 = {valid faces with a non-finite coordinate, vertices with one, valid faces, 0}.  seg: DEVICE 2 nv ints
 * (work). */
int rcmvs_ms_init(const float* verts, const int* faces, const unsigned char* rgb, int nv, int nf, const double* frame_host, unsigned* key_a,
                  int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, double* quad, int* members,
                  unsigned long long* csum, unsigned long long* live, unsigned long long* stats, void* stream);
int rcmvs_ms_init_timed(const float* verts, const int* faces, const unsigned char* rgb, int nv, int nf, const double* frame_host,
                        unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg,
                        double* quad, int* members, unsigned long long* csum, unsigned long long* live, unsigned long long* stats,
                        void* ev0, void* ev1, void* stream);

/* One round over faces_in, all on the stream.
 * Topology: rcmvs_mc_adjacency of faces_in (row_start, row_len, nbr, mult, on_boundary, cursor, heavy, heavy_capacity, adj_stats as
 * mesh_clean.h sizes them) and the corners of every vertex in ascending 3 face + corner (a stable sort of the valid faces'
 * corners by vertex; seg: DEVICE 2 nv ints).  locked: DEVICE nv bytes, 1 for a vertex with a non-finite coordinate or with an
 * edge of multiplicity != 2.
 * Candidates, one lane per CSR entry i of u -> v with u < v: multiplicity 2 and not both ends locked.  edge: DEVICE 6 nf bytes,
 * RCMVS_MS_EDGE_NONE for an entry that is no candidate, else the first of COST (!(cost <= max_error)), LINK (ms::link_ok over the
 * two rings) and FLIP (ms::keeps_side fails for a face at u or v that does not hold the other) that applies, else OK.  The target is
 * ms::place's, rounded once to fp32 (md::world) or an endpoint's bits; the cost is ms::cost at the fp32 target taken back into the
 * frame, and the flip test moves the corner there.  key: DEVICE 6 nf uint64, ms::key(cost, i) at the entry of an OK edge AND at
 * its mirror entry v -> u, ms::NO_KEY at every other entry.
 * Independent set: best1: DEVICE nv uint64, the smallest key in the vertex's segment; best2: DEVICE nv uint64, the smallest best1
 * over the vertex and its ring.  selected: DEVICE 6 nf bytes, 1 at the entry of an OK edge with key == best2[u] == best2[v].
 * Budget: rank: DEVICE 6 nf + 1 ints, the exclusive prefix sums of selected; applied: DEVICE 6 nf bytes, selected and rank <
 * ms::budget(live, target_faces).
 * Apply, one lane per applied edge: the survivor s is u unless v is locked, the other end g is gone; verts[s] = the target,
 * quad[s] = ms::add(quad[u], quad[v]), members[s] and csum[s] = the sums, members[g] = 0, remap[g] = s; remap: DEVICE nv ints, the
 * identity elsewhere.  faces_out: DEVICE nf * 3 ints = faces_in with every index in [0, nv) taken through remap; it must not
 * overlap faces_in.  live: in, the valid faces of faces_in; out, those of faces_out.
 * counts: DEVICE RCMVS_MS_COUNTS uint64 by RCMVS_MS_COUNT_*: locked vertices, candidates, the three rejections, candidates by
 * path (5 from RCMVS_MS_COUNT_PATH), selected, applied, the largest applied cost as md::ordered bits of its fp32 value (0: none),
 * live after and before.  target_faces >= 0; max_error >= 0 or +inf, not NaN. */
int rcmvs_ms_round(float* verts, const int* faces_in, int* faces_out, int nv, int nf, const double* frame_host, double* quad, int* members,
                   unsigned long long* csum, long long target_faces, double max_error, int* row_start, int* row_len, int* nbr, int* mult,
                   unsigned char* on_boundary, int* cursor, int* heavy, int heavy_capacity, unsigned long long* adj_stats, unsigned* key_a,
                   int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start, int* scan_work, int* seg, unsigned char* locked,
                   unsigned char* edge, unsigned long long* key, unsigned long long* best1, unsigned long long* best2,
                   unsigned char* selected, int* rank, unsigned char* applied, int* remap, unsigned long long* live,
                   unsigned long long* counts, void* stream);
int rcmvs_ms_round_timed(float* verts, const int* faces_in, int* faces_out, int nv, int nf, const double* frame_host, double* quad,
                         int* members, unsigned long long* csum, long long target_faces, double max_error, int* row_start, int* row_len,
                         int* nbr, int* mult, unsigned char* on_boundary, int* cursor, int* heavy, int heavy_capacity,
                         unsigned long long* adj_stats, unsigned* key_a, int* idx_a, unsigned* key_b, int* idx_b, int* hist, int* hist_start,
                         int* scan_work, int* seg, unsigned char* locked, unsigned char* edge, unsigned long long* key,
                         unsigned long long* best1, unsigned long long* best2, unsigned char* selected, int* rank, unsigned char* applied,
                         int* remap, unsigned long long* live, unsigned long long* counts, int phase, void* ev0, void* ev1, void* stream);
/* phase of the _timed twin: which launches ev0 / ev1 bracket (every launch runs in every phase) */
#define RCMVS_MS_PHASE_ALL 0
#define RCMVS_MS_PHASE_TOPOLOGY 1
#define RCMVS_MS_PHASE_CANDIDATES 2
#define RCMVS_MS_PHASE_SELECTION 3
#define RCMVS_MS_PHASE_APPLY 4

/* What the output keeps, in the form rcmvs_mc_gather takes: face_keep: DEVICE nf bytes, 1 for a valid face; vert_keep: DEVICE nv
 * bytes, 1 for a vertex a valid face uses (drop_unreferenced != 0) or for every vertex with members > 0 (== 0); face_rank /
 * vert_rank: DEVICE nf + 1 / nv + 1 ints, their exclusive prefix sums; totals: DEVICE 2 uint64 = {faces kept, vertices kept}.
 * out_rgb (with csum, or both NULL): DEVICE nv * 3 bytes, md::colour(csum, members) for a vertex with members > 0. */
int rcmvs_ms_finish(const int* faces, int nv, int nf, const int* members, const unsigned long long* csum, int drop_unreferenced,
                    unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work, unsigned char* out_rgb,
                    unsigned long long* totals, void* stream);
int rcmvs_ms_finish_timed(const int* faces, int nv, int nf, const int* members, const unsigned long long* csum, int drop_unreferenced,
                          unsigned char* face_keep, unsigned char* vert_keep, int* face_rank, int* vert_rank, int* scan_work,
                          unsigned char* out_rgb, unsigned long long* totals, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_SIMPLIFY_H */
