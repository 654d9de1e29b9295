// A stand-alone host program over csrc/mesh_simplify_math.h: the header's rules are plain C++, so they can run under
// -fsanitize=address,undefined on the CPU (tests/test_mesh_simplify_cpu.py builds and runs this).  It walks every function over
// ordinary, degenerate and hostile values (NaN, infinities, the largest and the smallest fp32, empty rings) and checks the answers
// that are known exactly.  It prints "ok" and the number of checks; any failed check or sanitizer report ends it with a status != 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mesh_simplify_math.h"

using namespace rcmvs;

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static void corners(ms::Quadric& Q, const double (*p)[3], const int (*f)[3], int nf) {
    for (int i = 0; i < nf; ++i)
        for (int k = 0; k < 3; ++k) ms::add_corner(Q, p[f[i][0]], p[f[i][1]], p[f[i][2]]);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the frame
    {
        const float lo[3] = {-0.0f, 1.0f, -3.4e38f}, hi[3] = {0.0f, 1.0f, 3.4e38f}, flat[3] = {2.0f, 2.0f, 2.0f};
        CHECK(ms::centre(lo[0], hi[0]) == 0.0 && ms::centre(lo[1], hi[1]) == 1.0 && ms::centre(lo[2], hi[2]) == 0.0);
        CHECK(ms::side(lo, hi) == 2.0 * (double)3.4e38f && ms::side(flat, flat) == 1.0);
        CHECK(md::world(0.5, 1.0, -0.5) == 0.0f && !std::signbit(md::world(0.5, 1.0, -0.5)));
    }
    // a plane z = 0 (dyadic): singular, every point of it costs exactly 0, the midpoint wins the tie
    {
        const double p[4][3] = {{0, 0, 0}, {0.5, 0, 0}, {0, 0.5, 0}, {0.5, 0.5, 0}};
        const int f[2][3] = {{0, 1, 2}, {1, 3, 2}};
        ms::Quadric Q = ms::zero();
        corners(Q, p, f, 2);
        double x[3] = {7, 7, 7};
        int from = -1;
        CHECK(ms::place(Q, p[0], p[3], false, false, x, &from) == ms::PATH_MIDPOINT && from == ms::FROM_X);
        CHECK(x[0] == 0.25 && x[1] == 0.25 && x[2] == 0.0 && ms::cost(Q, x) == 0.0);
        const double up[3] = {0.25, 0.25, 0.5};
        CHECK(ms::cost(Q, up) == 6.0 * 0.0625 * 0.25);           // six corners, n = (0, 0, 1/4), distance 1/2
        CHECK(ms::place(Q, p[0], p[3], true, false, x, &from) == ms::PATH_LOCKED && from == ms::FROM_U);
        CHECK(ms::place(Q, p[0], p[3], false, true, x, &from) == ms::PATH_LOCKED && from == ms::FROM_V);
    }
    // a cube corner at (-1/2, -1/2, -1/2) and the next vertex along an edge: the minimiser is the corner, exactly
    {
        const double c[3] = {-0.5, -0.5, -0.5}, e[3] = {-0.25, -0.5, -0.5};
        const double p[7][3] = {{-0.5, -0.5, -0.5}, {-0.25, -0.5, -0.5}, {-0.5, -0.25, -0.5}, {-0.5, -0.5, -0.25}, {-0.25, -0.25, -0.5}, {-0.25, -0.5, -0.25}, {-0.5, -0.25, -0.25}};
        const int f[6][3] = {{0, 2, 4}, {0, 4, 1}, {0, 1, 5}, {0, 5, 3}, {0, 3, 6}, {0, 6, 2}};
        ms::Quadric Q = ms::zero();
        corners(Q, p, f, 6);
        double x[3];
        int from = -1;
        CHECK(ms::place(Q, c, e, false, false, x, &from) == ms::PATH_QUADRIC && from == ms::FROM_X);
        CHECK(x[0] == -0.5 && x[1] == -0.5 && x[2] == -0.5 && ms::cost(Q, x) == 0.0);
        const double far_u[3] = {-0.5, -0.5, -0.5}, far_v[3] = {-0.5 + 1e-3, -0.5, -0.5}, off[3] = {0.5, 0.5, 0.5};
        ms::Quadric R = ms::zero();
        const double q[3][3] = {{0.5, 0.5, 0.5}, {1.0, 0.5, 0.5}, {0.5, 1.0, 0.5}};
        const double r[3][3] = {{0.5, 0.5, 0.5}, {0.5, 1.0, 0.5}, {0.5, 0.5, 1.0}};
        const double s[3][3] = {{0.5, 0.5, 0.5}, {0.5, 0.5, 1.0}, {1.0, 0.5, 0.5}};
        ms::add_corner(R, q[0], q[1], q[2]);
        ms::add_corner(R, r[0], r[1], r[2]);
        ms::add_corner(R, s[0], s[1], s[2]);
        CHECK(ms::place(R, far_u, far_v, false, false, x, &from) != ms::PATH_QUADRIC);      // the minimiser `off` is too far from this edge
        (void)off;
    }
    // hostile values go through every function without a fault, and never win
    {
        ms::Quadric Q = ms::zero();
        const double a[3] = {nan, 0, 0}, b[3] = {inf, -inf, 1e308}, c[3] = {1e-320, -0.0, 3.4e38};
        ms::add_corner(Q, a, b, c);
        double x[3] = {0, 0, 0};
        int from = -1;
        const int path = ms::place(Q, b, c, false, false, x, &from);
        CHECK(path == ms::PATH_MIDPOINT);                        // NaN costs: nothing compares lower than the midpoint
        CHECK(!ms::cost_ok(ms::cost(Q, x), inf) && !ms::cost_ok(nan, 0.0) && ms::cost_ok(inf, inf) && ms::cost_ok(0.0, 0.0) && !ms::cost_ok(1e-300, 0.0));
        CHECK(!ms::keeps_side(a, b, c, 1, x) && !ms::keeps_side(c, c, c, 0, c));
        ms::Quadric Z = ms::zero();
        CHECK(!ms::solve(Z, x, 1.0, x) && ms::cost(Z, b) != ms::cost(Z, b));      // 0 * inf: a NaN stays a NaN
        ms::Quadric S = ms::add(Q, Z);
        CHECK(S.c != S.c);
    }
    // the flip test
    {
        const double q0[3] = {0, 0, 0}, q1[3] = {1, 0, 0}, q2[3] = {0, 1, 0}, same[3] = {0.25, 0.25, 0}, across[3] = {1, 1, 0}, on[3] = {0.5, 0.5, 0};
        CHECK(ms::keeps_side(q0, q1, q2, 0, same) && !ms::keeps_side(q0, q1, q2, 0, across) && !ms::keeps_side(q0, q1, q2, 0, on));
        CHECK(ms::keeps_side(q0, q1, q2, 1, q1) && ms::keeps_side(q0, q1, q2, 2, q2));
    }
    // rings
    {
        std::vector<int> a = {1, 4, 7, 9}, b = {0, 4, 9, 12, 13}, none;
        CHECK(ms::common(a.data(), 4, b.data(), 5) == 2 && ms::common(a.data(), 4, a.data(), 4) == 4);
        CHECK(ms::common(none.data(), 0, b.data(), 5) == 0 && ms::common(a.data(), 4, none.data(), 0) == 0 && ms::common(nullptr, 0, nullptr, 0) == 0);
        CHECK(ms::link_ok(2, 4, 4) && !ms::link_ok(2, 3, 3) && ms::link_ok(2, 3, 4) && !ms::link_ok(1, 6, 6) && !ms::link_ok(3, 6, 6));
    }
    // keys and the budget
    {
        CHECK(ms::key(0.0, 5) == ((0x80000000ull << 32) | 5ull) && ms::key(0.0, 5) < ms::key(1e-30, 0) && ms::key(1.0, 0x7fffffff) < ms::key(1.0000001, 0));
        CHECK(ms::key(1e300, 0) == ms::key(inf, 0) && ms::key(inf, 0x7fffffff) < ms::NO_KEY);      // a cost beyond fp32 becomes +inf
        CHECK(ms::budget(10, 10) == 0 && ms::budget(9, 10) == 0 && ms::budget(11, 10) == 1 && ms::budget(12, 10) == 1 && ms::budget(13, 10) == 2);
        CHECK(ms::budget(2147483647ll, 0) == 1073741824ll);
        CHECK(md::colour(3, 2) == 2 && md::colour(255ull * 1000000, 1000000) == 255);
    }
    std::printf("ok %d\n", checks);
    return 0;
}
