// Stand-alone host program over csrc/fusion_dyn_math.h for tests/test_fusion_dyn_cpu.py, which compiles it with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off and runs it as its own process: the header's per-pixel
// function on hostile numbers (NaN, +-Inf, 0, 1e30 as reference and source depths, a point at z = 0 in the source camera, positions
// beyond the far guard), with every debug output asked for.  Prints "ok <checks>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "fusion_dyn_math.h"

using namespace rcmvs::fu;

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

static void identity_mats(std::vector<double>& m, int N, const double* tx, const double* tz) {
    m.assign(REF_MATS + SRC_MATS * N, 0.0);
    auto eye3 = [&](int o) { m[o] = m[o + 4] = m[o + 8] = 1.0; };
    auto eye34 = [&](int o, double x, double z) { m[o] = m[o + 5] = m[o + 10] = 1.0; m[o + 3] = x; m[o + 11] = z; };
    eye3(0); eye3(9); eye34(18, 0.0, 0.0);
    for (int n = 0; n < N; ++n) {
        const int o = REF_MATS + n * SRC_MATS;
        eye34(o, tx[n], tz[n]); eye3(o + 12); eye3(o + 21); eye34(o + 30, -tx[n], -tz[n]);
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int H = 5, W = 7, N = 6, V = N + 1, plane = H * W;
    const float hostile[] = {nan, inf, -inf, 0.0f, 1e30f, -600.0f, 1e-30f, 3e38f, 1.0f, 1.25f};
    const int nh = (int)(sizeof(hostile) / sizeof(hostile[0]));
    // source shifts: none, half a pixel, a whole image, beyond the far guard both ways, and z = -1 (the point lands at z = 0 for depth 1)
    const double tx[N] = {0.0, 0.5, (double)W, 1e8, -4e7, 0.0}, tz[N] = {0.0, 0.0, 0.0, 0.0, 0.0, -1.0};
    std::vector<double> mats;
    identity_mats(mats, N, tx, tz);
    std::vector<int> src(N);
    for (int n = 0; n < N; ++n) src[n] = n + 1;
    std::vector<float> depth((size_t)V * plane), dbg_d((size_t)N * plane), dbg_xy((size_t)N * plane * 2);
    std::vector<unsigned char> dbg_l((size_t)N * plane);
    for (int ref_kind = 0; ref_kind < nh; ++ref_kind) {
        for (int src_kind = 0; src_kind < nh; ++src_kind) {
            for (int i = 0; i < plane; ++i) depth[i] = (i % 3 == 0) ? hostile[ref_kind] : 1.0f;
            for (int v = 1; v < V; ++v)
                for (int i = 0; i < plane; ++i) depth[(size_t)v * plane + i] = ((i + v) % 4 == 0) ? hostile[src_kind] : 1.0f + (float)((i * v) % 5) / 1024.0f;
            for (int lo = 1; lo <= 16; lo += 5) {
                for (int hi = lo; hi <= 16; hi += 3) {
                    const Levels L = levels(lo, hi, 0.25, 1.0f / 1300.0f);
                    for (int y = 0; y < H; ++y) {
                        for (int x = 0; x < W; ++x) {
                            const float d_ref = depth[y * W + x];
                            const Pixel px = fuse_pixel(mats.data(), depth.data(), src.data(), N, L, H, W, x, y, d_ref, dbg_d.data(), dbg_l.data(), dbg_xy.data());
                            CHECK(px.level == 0 || (px.level >= lo && px.level <= hi));
                            CHECK(px.level <= N && px.count_hi >= 0 && px.count_hi <= N && (px.hi_bits >> N) == 0);
                            int bits = 0;
                            for (int n = 0; n < N; ++n) {
                                const size_t at = (size_t)n * plane + y * W + x;
                                const bool on = (px.hi_bits >> n) & 1u;
                                bits += on;
                                CHECK(on || (dbg_d[at] == 0.0f && !std::signbit(dbg_d[at])));
                                CHECK(dbg_l[at] == 0 || (dbg_l[at] >= lo && dbg_l[at] <= hi));
                                CHECK(!on || dbg_l[at] != 0);
                                int mx = -1, my = -1;
                                const bool in = mark_pixel(dbg_xy[at * 2], dbg_xy[at * 2 + 1], H, W, &mx, &my);
                                CHECK(!in || (mx >= 0 && mx < W && my >= 0 && my < H));
                                if (n >= 3 && n <= 4) CHECK(!in || !std::isfinite(d_ref) || std::fabs(d_ref) > 1e6f || d_ref == 0.0f);   // beyond the far guard
                            }
                            CHECK(bits == px.count_hi);
                            double w[3];
                            world_point(mats.data(), x, y, px.avg, w);
                            CHECK(!std::isfinite(px.avg) || w[2] == px.avg);
                        }
                    }
                }
            }
        }
    }
    // the rounding of a mark and its guards, one by one
    int mx = 0, my = 0;
    CHECK(mark_pixel(0.5f, 1.5f, H, W, &mx, &my) && mx == 0 && my == 2);              // ties to even
    CHECK(mark_pixel(2.5f, 2.5f, H, W, &mx, &my) && mx == 2 && my == 2);
    CHECK(mark_pixel(-0.5f, 0.0f, H, W, &mx, &my) && mx == 0);                        // -0.5 rounds to -0: inside
    CHECK(mark_pixel(W - 0.5f, 0.0f, H, W, &mx, &my) && mx == W - 1);                 // W odd: W - 0.5 rounds to the even W - 1
    CHECK(!mark_pixel(-0.51f, 0.0f, H, W, &mx, &my) && !mark_pixel((float)W, 0.0f, H, W, &mx, &my) && !mark_pixel(0.0f, (float)H - 0.49f, H, W, &mx, &my));
    CHECK(!mark_pixel(1e8f, 0.0f, H, W, &mx, &my) && !mark_pixel(0.0f, -1e8f, H, W, &mx, &my) && !mark_pixel(3.2e7f, 0.0f, H, W, &mx, &my));
    CHECK(!mark_pixel(nan, 0.0f, H, W, &mx, &my) && !mark_pixel(0.0f, nan, H, W, &mx, &my) && !mark_pixel(inf, 0.0f, H, W, &mx, &my) && !mark_pixel(0.0f, -inf, H, W, &mx, &my));
    // levels: each product rounded once, NaN and negative bases pass nothing, an infinite base passes every finite distance
    const Levels L = levels(1, 16, 0.1, 0.1f);
    for (int n = 1; n <= 16; ++n) CHECK(L.dist_t[n - 1] == (double)n * 0.1 && L.rel_t[n - 1] == (float)n * 0.1f);
    CHECK(pass_bits(L, 0.0, 0.0f) == 0xffffu && pass_bits(L, (double)nan, 0.0f) == 0 && pass_bits(L, 0.0, nan) == 0 && pass_bits(L, 0.25, 0.0f) == 0xfffcu);
    CHECK(pass_bits(levels(3, 5, 0.1, 0.1f), 0.0, 0.0f) == 0x1cu && lowest_level(0x1cu) == 3 && lowest_level(0) == 0 && lowest_level(0x8000u) == 16);
    CHECK(pass_bits(levels(1, 16, (double)nan, 0.1f), 0.0, 0.0f) == 0 && pass_bits(levels(1, 16, -1.0, 0.1f), 0.0, 0.0f) == 0);
    CHECK(pass_bits(levels(1, 16, (double)inf, inf), 1e300, 3e38f) == 0xffffu && pass_bits(levels(1, 16, (double)inf, inf), (double)inf, 0.0f) == 0);
    // the packed counts: sixteen sources passing every level give 16 in every byte, and no byte carries into its neighbour
    Counts c = {{0u, 0u, 0u, 0u}};
    for (int i = 0; i < 16; ++i) count_add(c, 0xffffu);
    for (int i = 0; i < 16; ++i) count_add(c, 0x8421u);
    for (int n = 1; n <= 16; ++n) CHECK(count_of(c, n) == (((0x8421u >> (n - 1)) & 1u) ? 32 : 16));
    std::printf("ok %d\n", checks);
    return 0;
}
