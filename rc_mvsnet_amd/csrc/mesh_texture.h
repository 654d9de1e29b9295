/* C ABI of the mesh texturing in librcmvs_hip.so (an extension header of include/rcmvs.h like mesh_normals.h, whose conventions it
 * keeps: status-returning entry points, rcmvs_last_error_string, a HIP stream as void*, a *_timed twin whose ev0 / ev1 receive the
 * first launch's start and the last launch's stop; additive, RCMVS_VERSION stays 106). */
#ifndef RCMVS_MESH_TEXTURE_H
#define RCMVS_MESH_TEXTURE_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- triangle mesh + the images of V views -> a texture atlas, per-corner texel coordinates and textured renders
 * (rc_mvsnet_amd/mesh_texture.py; csrc/mesh_texture.hip; the per-element rules are csrc/mesh_texture_math.h's, restated by
 * tests/mesh_texture_oracle.py) ----
 * A mesh is verts (nv, 3) fp32, faces (nf, 3) int32 and optionally rgb (nv, 3) uint8, all DEVICE; 0 <= nv < 2^31,
 * 0 <= nf <= RCMVS_MT_MAX_FACES, and a pointer to an array of no elements may be NULL.  Validity of a face is mesh_clean.h's; every
 * kernel tests it before an index is used as an address.  Views are H x W, 1 <= H, W <= 16384, cameras are rows of 16 doubles
 * (mesh_render.h's layout, pixel centres at integers).  No output or work buffer may overlap another buffer.
 *
 * VOTE.  rcmvs_mt_vote takes n views' face images (n, H, W) int32 as rcmvs_mr_render wrote them and the views' cameras on the HOST;
 * the views are numbered first_view .. first_view + n - 1.  reset != 0 zeroes best first.  Per view, in order: count (nf ints, work)
 * is zeroed; a thread per pixel adds 1 to count[f] for f in [0, nf) (the only atomic: an integer add); a thread per face projects
 * its vertices by mesh_render_math.h and, when the view is eligible (the face valid, the three vertices usable and inside the sample
 * rectangle 0 <= X <= 256 (W - 1), 0 <= Y <= 256 (H - 1)) and count > 0, sets best[f] = max(best[f], count << 32 | 0xFFFFFFFF - view).
 * best: DEVICE nf uint64; 0 = unseen.  Calls over chunks of the views give the bits of one call over all of them.
 *
 * LAYOUT.  rcmvs_mt_layout takes best, the V cameras on the DEVICE (cams_dev) and shift in [0, RCMVS_MT_MAX_SHIFT].  A face is SEEN
 * when best names a view below V in which it is eligible.  klass[f] (DEVICE nf ints): for a seen face the smallest k in
 * [RCMVS_MT_MIN_CLASS, RCMVS_MT_MAX_CLASS] with ((2^k - 3) << (8 + shift))^2 >= the largest squared lattice length of its edges in its
 * view, RCMVS_MT_MAX_CLASS and counted as capped when none reaches it; RCMVS_MT_MIN_CLASS for an unseen valid face; 0 for an invalid
 * one.  The faces are sorted by descending class with one stable 8-bit pass of scan_sort.hip's radix sort on the key
 * RCMVS_MT_MAX_CLASS - k (255 for an invalid face): order (DEVICE nf ints) is the sorted list of face numbers, key_a / idx_a / key_b
 * (nf each), hist (256 ceil(nf / 256) ints), hist_start (one more) and scan_work (mesh_clean.h's, for max(256 ceil(nf / 256), nf)
 * elements) are work.  table: DEVICE RCMVS_MT_TABLE int64 = per class k at 4 k {start in the sorted order, faces, cells =
 * ceil(faces / 2), Morton base = sum over j > k of cells_j 4^j}, then at 44 {total, m, S = 2^m, Sy}: the atlas is S wide and Sy
 * high, 4^m >= total, Sy = S / 2 when S >= 2 and 2 total <= S^2.  texel: DEVICE (nf, 3, 2) int32, the texel centres (x, y) of the
 * corners a, b, c; zeros for an invalid face.  The face at sorted position start_k + r has cell r >> 1 and half r & 1 of its class;
 * mesh_texture_math.h states the rest.  stats: DEVICE RCMVS_MT_STATS uint64 = {faces seen, unseen, invalid, capped, texels from an
 * image, texels from vertex colours (unseen faces), texels of projection fallback, 0, faces of class 0 .. 10, 0 ...}; the call zeroes
 * all of it and fills the faces' counters.  The _timed twin brackets every launch (RCMVS_MT_PHASE_ALL).
 *
 * FILL.  rcmvs_mt_fill takes what layout produced, S and Sy as the host read them from the table (a table that states another size
 * leaves the atlas background), the images (V, H, W, 3) uint8 DEVICE and cams_dev.  One thread per Morton index below S Sy: atlas
 * (Sy, S, 3) uint8 and owner (Sy, S) int32 (the face, -1 for background).  A texel of a seen face is the bilinear sample of its
 * view's image at the projection of its surface point, of an unseen face or when the projection fails the vertex colours under the
 * texel's weights (white without rgb).  The call zeroes and fills the three texel counters of stats.
 *
 * SHADE.  rcmvs_mt_shade is shaped like rcmvs_mn_shade (cameras on the HOST): tex_rgb (n, H, W, 3) uint8 is the bilinear sample of
 * the atlas at the perspective-correct texel position of each pixel whose face number is in [0, nf), whose face is valid and usable
 * with area2 != 0; background (r | g << 8 | b << 16) elsewhere. */
#define RCMVS_MT_MIN_CLASS 2
#define RCMVS_MT_MAX_CLASS 10
#define RCMVS_MT_MAX_SHIFT 8
#define RCMVS_MT_MAX_ATLAS 16384
#define RCMVS_MT_MAX_FACES 1073741568
#define RCMVS_MT_STATS 24
#define RCMVS_MT_TABLE 48
#define RCMVS_MT_SORT_BLOCK 256
#define RCMVS_MT_PHASE_ALL 0

int rcmvs_mt_vote(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z, const int* face_image,
                  int first_view, int reset, int* count, unsigned long long* best, void* stream);
int rcmvs_mt_vote_timed(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z,
                        const int* face_image, int first_view, int reset, int* count, unsigned long long* best, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_mt_layout(const float* verts, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev, double near_z,
                    const unsigned long long* best, int shift, int* klass, unsigned* key_a, int* idx_a, unsigned* key_b, int* order, int* hist,
                    int* hist_start, int* scan_work, long long* table, int* texel, unsigned long long* stats, void* stream);
int rcmvs_mt_layout_timed(const float* verts, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev, double near_z,
                          const unsigned long long* best, int shift, int* klass, unsigned* key_a, int* idx_a, unsigned* key_b, int* order, int* hist,
                          int* hist_start, int* scan_work, long long* table, int* texel, unsigned long long* stats, int phase, void* ev0, void* ev1,
                          void* stream);

int rcmvs_mt_fill(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev, double near_z,
                  const unsigned char* images, const unsigned long long* best, const int* order, const long long* table, int S, int Sy, int background,
                  unsigned char* atlas, int* owner, unsigned long long* stats, void* stream);
int rcmvs_mt_fill_timed(const float* verts, const unsigned char* rgb, const int* faces, int nv, int nf, int V, int H, int W, const double* cams_dev,
                        double near_z, const unsigned char* images, const unsigned long long* best, const int* order, const long long* table, int S, int Sy,
                        int background, unsigned char* atlas, int* owner, unsigned long long* stats, int phase, void* ev0, void* ev1, void* stream);

int rcmvs_mt_shade(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z, const int* face_image,
                   const int* texel, const unsigned char* atlas, int S, int Sy, int background, unsigned char* tex_rgb, void* stream);
int rcmvs_mt_shade_timed(const float* verts, const int* faces, int nv, int nf, int n, int H, int W, const double* cams_host, double near_z,
                         const int* face_image, const int* texel, const unsigned char* atlas, int S, int Sy, int background, unsigned char* tex_rgb, int phase,
                         void* ev0, void* ev1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCMVS_MESH_TEXTURE_H */
