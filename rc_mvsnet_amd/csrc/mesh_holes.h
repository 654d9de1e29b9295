/* C ABI of the hole-filling pass in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_clean.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, *_timed twins whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_HOLES_H
#define RCMVS_MESH_HOLES_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh -> its boundary loops, the short ones closed (rc_mvsnet_amd/mesh_holes.py; csrc/mesh_holes.hip; the
 * per-element rules are csrc/mesh_holes_math.h's, restated by tests/mesh_holes_oracle.py) ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE; 0 <= nv, nf < 2^31, and a
 * pointer to an array of no elements may be NULL.  Validity of a face is mesh_clean.h's (three indices in [0, nv) that differ);
 * every kernel tests it before an index is used as an address.
 *
 * THE RULE.  A valid face (a, b, c) has the half-edges a->b, b->c, c->a.  A half-edge v->w is a BOUNDARY half-edge when the
 * undirected edge {v, w} has multiplicity 1 in the 1-ring of the same faces (rcmvs_mc_adjacency).  out[v] / in[v] count the
 * boundary half-edges that leave / arrive at v.  v is SIMPLE when out[v] == in[v] == 1, COMPLEX when out[v] + in[v] > 0 and it is
 * not simple (bow-ties, fans on non-manifold edges, neighbours of inconsistent orientation).  succ[v] / pred[v] are the head of the
 * one boundary half-edge that leaves a simple v / the tail of the one that arrives; -1 for every other vertex.
 * A LOOP is a cycle u0 -> u1 -> ... -> u(L-1) -> u0 of succ in which every vertex is simple; u0, its LEADER, is its smallest
 * vertex number; L >= 3.  A chain that reaches a vertex that is not simple is no loop.  A loop is FILLED when L <= max_edges,
 * 3 <= max_edges <= RCMVS_MH_MAX_EDGES.  Loops are handled in ascending leader order:
 *   L == 3  one face (u0, u2, u1), no new vertex.
 *   L > 3   one new vertex c = per coordinate (float)(s / (double)L), s = 0.0 + the members' coordinates in loop order from u0, in
 *           fp64 without contraction; no position is compared, NaN and infinities go through the arithmetic.  Its colour is per
 *           channel (2 * sum + L) / (2 * L) in integers (the members' mean rounded half up, mesh_decimate's rule).  L faces:
 *           face i = (u((i + 1) mod L), u(i), c), the reverse of the boundary half-edge it closes.
 * Output vertices: the input vertices in every bit, then the new ones in ascending leader order.  Output faces: the input faces
 * in every bit and in order, invalid ones included, then each filled loop's faces in ascending leader order, inside a loop in
 * loop order.  Every output is a function of the inputs alone: atomics only add integers or take an integer maximum, the one plain
 * store that can race (succ / pred at a complex vertex) is overwritten with -1 by the next launch, and ranks come from scans.
 * No kernel reads a cell that another workgroup of the same launch writes.
 * Scans run in three levels over tiles of RCMVS_MH_SCAN_TILE elements.  scan_work: DEVICE, 8-byte aligned,
 * RCMVS_MH_SCAN_WORK + ceil(nv / RCMVS_MH_SCAN_TILE) + 1 ints. */
#define RCMVS_MH_MAX_EDGES 4096
#define RCMVS_MH_SCAN_TILE 2048
#define RCMVS_MH_SCAN_WORK 2048
#define RCMVS_MH_NONE 0
#define RCMVS_MH_SIMPLE 1
#define RCMVS_MH_COMPLEX 2

/* Boundary half-edges.  row_start (nv + 1), row_len (nv), nbr and mult (entries, 0 <= entries < 2^31) are rcmvs_mc_adjacency's
 * of the SAME faces; a segment that does not lie inside nbr, or a head that its tail's segment does not hold, gives no boundary
 * half-edge.  out_count, in_count, succ, pred: DEVICE nv ints; flags: DEVICE nv bytes (RCMVS_MH_NONE / _SIMPLE / _COMPLEX).
 * counts: DEVICE 2 uint64 = {boundary half-edges (= edges of multiplicity 1), complex vertices}.  One thread per face corner finds
 * the multiplicity by bisection in the tail's sorted segment. */
int rcmvs_mh_boundary(const int* faces, int nv, int nf, const int* row_start, const int* row_len, const int* nbr, const int* mult, long long entries,
                      int* out_count, int* in_count, int* succ, int* pred, unsigned char* flags, unsigned long long* counts, void* stream);
int rcmvs_mh_boundary_timed(const int* faces, int nv, int nf, const int* row_start, const int* row_len, const int* nbr, const int* mult, long long entries,
                            int* out_count, int* in_count, int* succ, int* pred, unsigned char* flags, unsigned long long* counts, void* ev0,
                            void* ev1, void* stream);

/* Leaders and ranks.  A vertex with succ[v] > v and pred[v] > v walks succ (finished by an earlier call: this launch writes
 * neither) and gives up at the first vertex smaller than itself, at a value outside [0, nv), or after max_edges steps; it is a
 * leader when it arrives back at itself, after L steps.  loop_len: DEVICE nv ints, L at the leader of a filled loop, 0 elsewhere.
 * vert_count (DEVICE nv bytes) / face_count (DEVICE nv ints): the vertices (0 or 1) and faces (0, 1 or L) the vertex's loop adds;
 * vert_rank / face_rank: DEVICE nv + 1 ints, their exclusive prefix sums, the totals last.
 * totals: DEVICE 5 uint64 = {vertices added, faces added, loops filled, loops filled by one face, the longest filled loop}. */
int rcmvs_mh_leaders(const int* succ, const int* pred, int nv, int max_edges, int* loop_len, unsigned char* vert_count, int* face_count, int* vert_rank,
                     int* face_rank, int* scan_work, unsigned long long* totals, void* stream);
int rcmvs_mh_leaders_timed(const int* succ, const int* pred, int nv, int max_edges, int* loop_len, unsigned char* vert_count, int* face_count,
                           int* vert_rank, int* face_rank, int* scan_work, unsigned long long* totals, void* ev0, void* ev1, void* stream);

/* The filled mesh.  out_verts (nv_out, 3) / out_rgb (nv_out, 3; with rgb or both NULL) / out_faces (nf_out, 3): the input copied
 * in every bit, then one lane per leader walks its loop once more and writes the loop's vertex at nv + vert_rank[leader] and its
 * faces from nf + face_rank[leader].  nv <= nv_out, nf <= nf_out (both below 2^31 as ints: the caller refuses a mesh whose counts
 * would reach 2^31); a rank outside the output is not written, and a walk that leaves [0, nv) stops.  The outputs must not
 * overlap the inputs. */
int rcmvs_mh_emit(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, const int* succ, const int* loop_len,
                  const int* vert_rank, const int* face_rank, int nv_out, int nf_out, float* out_verts, unsigned char* out_rgb, int* out_faces,
                  void* stream);
int rcmvs_mh_emit_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, const int* succ, const int* loop_len,
                        const int* vert_rank, const int* face_rank, int nv_out, int nf_out, float* out_verts, unsigned char* out_rgb,
                        int* out_faces, void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_HOLES_H */
