// The per-element rules of the mesh texturing (rc_mvsnet_amd/mesh_texture.py; contract in mesh_texture.h): a face's vote for a view,
// its size class, the Morton atlas (the per-class table, a cell's origin, the corners' texels, the owner of a texel), a texel's
// colour from the chosen view's image and a pixel's colour from the atlas.  Plain C++ shared by mesh_texture.hip and host code,
// restated by tests/mesh_texture_oracle.py with the same operation order: this header is normative for that order.  Decisions are
// integers (int64); floating point is fp64 under `fp contract(off)`: every expression is evaluated as written, one rounding per
// operation.  A vertex is projected by mesh_render_math.h's camera() and project() wherever a lattice coordinate is needed.
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_render_math.h"                                     // mr::camera, mr::project, mr::area2, mr::face, mr::weights

namespace rcmvs {
namespace mt {

using u64 = unsigned long long;

constexpr int MIN_CLASS = 2, MAX_CLASS = 10, MAX_SHIFT = 8;       // a cell's side is 2^k texels, k in [MIN_CLASS, MAX_CLASS]
constexpr int CLASSES = MAX_CLASS + 1;                            // the tables have a row per k in [0, MAX_CLASS]; rows below MIN_CLASS stay empty
constexpr unsigned SENTINEL = 255;                                // the sort key of an invalid face: last
// the counters (RCMVS_MT_STATS uint64)
constexpr int SEEN = 0, UNSEEN = 1, INVALID = 2, CAPPED = 3, TEX_IMAGE = 4, TEX_VERTEX = 5, TEX_FALLBACK = 6, PER_CLASS = 8;
// the table (RCMVS_MT_TABLE int64): four entries per class k at 4 k, then the totals
constexpr int T_START = 0, T_COUNT = 1, T_CELLS = 2, T_BASE = 3, T_TOTAL = 4 * CLASSES, T_M = T_TOTAL + 1, T_S = T_TOTAL + 2, T_SY = T_TOTAL + 3;
constexpr double F64_MAX = 1.7976931348623157e308;

#pragma clang fp contract(off)

// ---- vote ---------------------------------------------------------------------------------------------------------------------------
// A view is eligible for a valid face when its three vertices are usable and lie in the image's sample rectangle
// 0 <= X <= 256 (W - 1), 0 <= Y <= 256 (H - 1): every point of the face then projects inside the image.
RCMVS_HD bool in_rect(const mr::Proj& p, int H, int W) {
    return p.usable && p.X >= 0 && p.X <= mr::SUB * (W - 1) && p.Y >= 0 && p.Y <= mr::SUB * (H - 1);
}
RCMVS_HD bool eligible(const mr::Proj& a, const mr::Proj& b, const mr::Proj& c, int H, int W) { return in_rect(a, H, W) && in_rect(b, H, W) && in_rect(c, H, W); }
// the maximum over the views is the most samples, then the smallest view number; 0 is no view
RCMVS_HD u64 vote_key(unsigned count, unsigned view) { return ((u64)count << 32) | (u64)(0xFFFFFFFFu - view); }
// the view a key names; false for 0 and for a view number that is not below V (a key is never trusted as an address)
RCMVS_HD bool chosen_view(u64 best, int V, int* view) {
    if (best == 0) return false;
    const u64 v = 0xFFFFFFFFull - (best & 0xFFFFFFFFull);
    if (v >= (u64)V) return false;
    *view = (int)v;
    return true;
}

// ---- size class ---------------------------------------------------------------------------------------------------------------------
// Lattice coordinates of an eligible view lie in [0, 2^22]: a difference is below 2^22 + 1, the sum of two squares below 2^46.
RCMVS_HD long long edge2(const mr::Proj& p, const mr::Proj& q) {
    const long long dx = (long long)(q.X - p.X), dy = (long long)(q.Y - p.Y);
    return dx * dx + dy * dy;
}
RCMVS_HD long long longest_edge2(const mr::Proj& a, const mr::Proj& b, const mr::Proj& c) {
    const long long ab = edge2(a, b), bc = edge2(b, c), ca = edge2(c, a);
    const long long m = ab > bc ? ab : bc;
    return m > ca ? m : ca;
}
// the smallest k whose legs (2^k - 3 texels, 256 << shift lattice steps each) reach the longest edge: ((2^k - 3) << (8 + shift))^2 >= e2;
// at most 1021 << 16 < 2^26, squared below 2^52.  No class reaches it: MAX_CLASS, capped.
RCMVS_HD int size_class(long long e2, int shift, int* capped) {
    *capped = 0;
    for (int k = MIN_CLASS; k <= MAX_CLASS; ++k) {
        const long long side = (long long)((1 << k) - 3) << (8 + shift);
        if (side * side >= e2) return k;
    }
    *capped = 1;
    return MAX_CLASS;
}

// ---- Morton order -------------------------------------------------------------------------------------------------------------------
// x from the even bits, y from the odd bits
RCMVS_HD unsigned compact_even(u64 x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (unsigned)x;
}
RCMVS_HD int morton_x(long long m) { return (int)compact_even((u64)m); }
RCMVS_HD int morton_y(long long m) { return (int)compact_even((u64)m >> 1); }

// ---- the table ----------------------------------------------------------------------------------------------------------------------
// per_class[k]: the valid faces of class k.  In descending class order: start_k (the class's first position in the sorted order),
// cells_k = ceil(n_k / 2), base_k = the sum of cells_j 4^j over j > k (a multiple of 4^k).  total = the sum of cells_k 4^k; the atlas
// is S x Sy, S = 2^m with the smallest m whose 4^m >= total, Sy = S / 2 when S >= 2 and 2 total <= S^2 (the top Morton bit is a y
// bit), else S.  nf < 2^30 faces of class 10 give a total below 2^49.
RCMVS_HD void layout_table(const u64* per_class, long long* table) {
    long long start = 0, base = 0;
    for (int k = MAX_CLASS; k >= 0; --k) {
        const long long n = (long long)per_class[k], cells = (n + 1) >> 1;
        table[4 * k + T_START] = start;
        table[4 * k + T_COUNT] = n;
        table[4 * k + T_CELLS] = cells;
        table[4 * k + T_BASE] = base;
        start += n;
        base += cells << (2 * k);
    }
    int m = 0;
    while ((1ll << (2 * m)) < base) ++m;
    const long long S = 1ll << m;
    table[T_TOTAL] = base;
    table[T_M] = m;
    table[T_S] = S;
    table[T_SY] = (S >= 2 && 2 * base <= S * S) ? S / 2 : S;
}

// The texel centres of the corners a, b, c of the face at rank r of class k (cell r >> 1, half r & 1), x then y per corner.
// Half 0: a -> (0, 0), b -> (L, 0), c -> (0, L) from the cell's origin, L = 2^k - 3.  Half 1: the same read through
// i' = s - 1 - i, j' = s - 1 - j (a half turn: the orientation is kept).
RCMVS_HD void corner_texels(long long base_k, long long r, int k, int* t) {
    const int s = 1 << k, L = s - 3;
    const long long m = base_k + ((r >> 1) << (2 * k));
    const int ox = morton_x(m), oy = morton_y(m);
    if ((r & 1) == 0) {
        t[0] = ox;     t[1] = oy;
        t[2] = ox + L; t[3] = oy;
        t[4] = ox;     t[5] = oy + L;
    } else {
        const int X = ox + s - 1, Y = oy + s - 1;
        t[0] = X;     t[1] = Y;
        t[2] = X - L; t[3] = Y;
        t[4] = X;     t[5] = Y - L;
    }
}

// The texel at Morton index m: its class (bases ascend as classes descend), its cell, its local (i, j), its half (half 0 owns
// i + j <= s - 2, the diagonal i + j = s - 2 being its gutter; half 1 owns the rest), the coordinates (ip, jp) in its half's frame
// and its face's position in the sorted order; pos = -1 for an odd class's missing partner.  false at or beyond the total.
struct Texel {
    int k, half, ip, jp;
    long long pos;
};
RCMVS_HD bool locate(const long long* table, long long m, Texel* t) {
    if (m < 0 || m >= table[T_TOTAL]) return false;
    for (int k = MIN_CLASS; k <= MAX_CLASS; ++k) {
        const long long base = table[4 * k + T_BASE], cells = table[4 * k + T_CELLS];
        if (cells <= 0 || m < base || m >= base + (cells << (2 * k))) continue;
        const long long rel = m - base, cell = rel >> (2 * k), loc = rel & ((1ll << (2 * k)) - 1);
        const int s = 1 << k, i = morton_x(loc), j = morton_y(loc);
        t->k = k;
        t->half = i + j <= s - 2 ? 0 : 1;
        t->ip = t->half ? s - 1 - i : i;
        t->jp = t->half ? s - 1 - j : j;
        const long long r = 2 * cell + t->half;
        t->pos = r < table[4 * k + T_COUNT] ? table[4 * k + T_START] + r : -1;
        return true;
    }
    return false;
}

// ---- colour -------------------------------------------------------------------------------------------------------------------------
// wb = i' / L, wc = j' / L, wa = (1 - wb) - wc: slightly negative in a gutter, which extrapolates
struct Weights {
    double a, b, c;
};
RCMVS_HD Weights texel_weights(int ip, int jp, int L) {
    Weights w;
    w.b = (double)ip / (double)L;
    w.c = (double)jp / (double)L;
    w.a = (1.0 - w.b) - w.c;
    return w;
}
RCMVS_HD double mix(const Weights& w, double A, double B, double C) { return (w.a * A + w.b * B) + w.c * C; }

// mr::camera on fp64 inputs, the same order of operations
RCMVS_HD mr::Point camera_d(const double* c, double x, double y, double z) {
    mr::Point p;
    p.x = ((c[0] * x + c[1] * y) + c[2] * z) + c[9];
    p.y = ((c[3] * x + c[4] * y) + c[5] * z) + c[10];
    p.z = ((c[6] * x + c[7] * y) + c[8] * z) + c[11];
    return p;
}

RCMVS_HD double clamp_to(double x, double hi) { return x < 0.0 ? 0.0 : (x > hi ? hi : x); }

// u = fx (xc / zc) + cx, v likewise; false unless zc >= near and u, v are finite; then clamped to [0, W - 1] x [0, H - 1]
RCMVS_HD bool image_position(const double* c, double near_z, mr::Point p, int H, int W, double* u, double* v) {
    if (!(p.z >= near_z)) return false;
    const double pu = c[12] * (p.x / p.z) + c[14];
    const double pv = c[13] * (p.y / p.z) + c[15];
    if (!(fabs(pu) <= F64_MAX && fabs(pv) <= F64_MAX)) return false;
    *u = clamp_to(pu, (double)(W - 1));
    *v = clamp_to(pv, (double)(H - 1));
    return true;
}

RCMVS_HD unsigned char byte_of(double x) { return (unsigned char)(int)(x >= 255.0 ? 255.0 : (x >= 0.0 ? x : 0.0)); }

// One channel of an (H, W, 3) byte image at (u, v) in [0, W - 1] x [0, H - 1]: x0 = min(floor(u), W - 2), 0 when W == 1,
// x1 = min(x0 + 1, W - 1), fx = u - x0, rows likewise; top = (1 - fx) p(y0, x0) + fx p(y0, x1), bottom on y1 likewise,
// floor(((1 - fy) top + fy bottom) + 0.5).
struct Tap {
    int x0, x1, y0, y1;
    double fx, fy;
};
RCMVS_HD Tap tap(double u, double v, int H, int W) {
    Tap t;
    t.x0 = (int)floor(u);
    if (t.x0 > W - 2) t.x0 = W - 2;
    if (t.x0 < 0) t.x0 = 0;
    t.x1 = t.x0 + 1 < W - 1 ? t.x0 + 1 : W - 1;
    t.y0 = (int)floor(v);
    if (t.y0 > H - 2) t.y0 = H - 2;
    if (t.y0 < 0) t.y0 = 0;
    t.y1 = t.y0 + 1 < H - 1 ? t.y0 + 1 : H - 1;
    t.fx = u - (double)t.x0;
    t.fy = v - (double)t.y0;
    return t;
}
RCMVS_HD unsigned char bilinear(const unsigned char* img, int W, const Tap& t, int ch) {
    const double p00 = (double)img[3 * ((size_t)t.y0 * W + t.x0) + ch], p01 = (double)img[3 * ((size_t)t.y0 * W + t.x1) + ch];
    const double p10 = (double)img[3 * ((size_t)t.y1 * W + t.x0) + ch], p11 = (double)img[3 * ((size_t)t.y1 * W + t.x1) + ch];
    const double top = (1.0 - t.fx) * p00 + t.fx * p01;
    const double bottom = (1.0 - t.fx) * p10 + t.fx * p11;
    return byte_of(floor(((1.0 - t.fy) * top + t.fy * bottom) + 0.5));
}

// a texel of a face that has no image: the vertex colours under the texel's weights
RCMVS_HD unsigned char vertex_colour(const Weights& w, int ca, int cb, int cc) { return byte_of(floor(mix(w, (double)ca, (double)cb, (double)cc) + 0.5)); }

// ---- a pixel of a textured view -----------------------------------------------------------------------------------------------------
// The pixel (px, py) sees the face f whose corners' texels are t: the weights of mr::weights, q_i = (double)w_i iz_i, the position
// ((q0 Ta + q1 Tb) + q2 Tc) / ((q0 + q1) + q2) per axis; false unless both are finite; then clamped to the atlas.
RCMVS_HD bool atlas_position(const mr::Face& f, int px, int py, const int* t, int Sy, int S, double* tx, double* ty) {
    long long w[3];
    mr::weights(f, px, py, w);
    const double q0 = (double)w[0] * f.iz[0], q1 = (double)w[1] * f.iz[1], q2 = (double)w[2] * f.iz[2];
    const double den = (q0 + q1) + q2;
    const double x = ((q0 * (double)t[0] + q1 * (double)t[2]) + q2 * (double)t[4]) / den;
    const double y = ((q0 * (double)t[1] + q1 * (double)t[3]) + q2 * (double)t[5]) / den;
    if (!(fabs(x) <= F64_MAX && fabs(y) <= F64_MAX)) return false;
    *tx = clamp_to(x, (double)(S - 1));
    *ty = clamp_to(y, (double)(Sy - 1));
    return true;
}

}  // namespace mt
}  // namespace rcmvs
