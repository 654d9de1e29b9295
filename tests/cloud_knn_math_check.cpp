// A stand-alone host program over csrc/cloud_knn_math.h: the header's rules are plain C++, so they can run under
// -fsanitize=address,undefined on the CPU (tests/test_cloud_clean_cpu.py builds and runs this).  It walks the candidate order, the
// statistical bound, the covariance, the Jacobi iteration, the choice of the normal and its orientation over ordinary, degenerate and
// hostile values (duplicates, collinear points, the largest and the smallest fp32, NaN) and checks the answers that are known
// exactly.  It prints "ok" and the number of checks; any failed check or sanitizer report ends it with a status != 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "cloud_knn_math.h"

using namespace rcmvs;

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static ck::Sym3 covariance(const float (*p)[3], int m) {
    double s[3] = {(double)p[0][0], (double)p[0][1], (double)p[0][2]};
    for (int i = 1; i < m; ++i)
        for (int a = 0; a < 3; ++a) s[a] = s[a] + (double)p[i][a];
    const double mean[3] = {s[0] / m, s[1] / m, s[2] / m};
    ck::Sym3 c = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < m; ++i) ck::cov_add(mean, p[i][0], p[i][1], p[i][2], &c);
    ck::cov_finish(&c, m);
    return c;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the order of two candidates
    CHECK(ck::before(1.0, 9, 2.0, 0) && !ck::before(2.0, 0, 1.0, 9) && ck::before(1.0, 3, 1.0, 4) && !ck::before(1.0, 4, 1.0, 4) && !ck::before(1.0, 5, 1.0, 4));
    CHECK(ck::before(0.0, 1, inf, 2147483647) && ck::before(inf, 5, inf, 2147483647) && !ck::before(inf, 2147483647, inf, 2147483647));
    CHECK(!ck::before(nan, 0, 1.0, 1) && !ck::before(1.0, 0, nan, 1));
    // the bound
    CHECK(ck::threshold(1.0, 0.5, 2.0) == 2.0 && ck::threshold(1.0, 0.0, inf) == inf && ck::threshold(1.0, 0.5, 0.0) == 1.0);
    CHECK(std::isnan(ck::threshold(nan, nan, 2.0)) && ck::threshold(nan, nan, inf) == inf);
    // a plane z = 0: the normal is exactly (0, 0, 1), in one sweep
    {
        const float p[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {-1, 0, 0}, {0, -1, 0}};
        double n[3];
        bool conv;
        CHECK(ck::normal_of(covariance(p, 5), n, &conv) == ck::WITH_NORMAL && conv && n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0);
        const double above[3] = {0.3, 0.2, 5.0}, below[3] = {0.3, 0.2, -5.0}, in_plane[3] = {4.0, 4.0, 0.0};
        CHECK(!ck::orient(n, 0, 0, 0, above) && n[2] == 1.0);
        CHECK(!ck::orient(n, 0, 0, 0, in_plane) && n[2] == 1.0);                       // a dot of 0 keeps the normal
        CHECK(ck::orient(n, 0, 0, 0, below) && n[2] == -1.0);
    }
    // a tilted plane x + y + z = 0: the normal is (1, 1, 1) / sqrt(3) up to rounding, its largest component positive
    {
        const float p[6][3] = {{1, -1, 0}, {-1, 1, 0}, {1, 0, -1}, {-1, 0, 1}, {0, 1, -1}, {0, -1, 1}};
        double n[3], lam[3], v0[3], v1[3], v2[3];
        bool conv;
        const ck::Sym3 c = covariance(p, 6);
        CHECK(ck::normal_of(c, n, &conv) == ck::WITH_NORMAL && conv);
        const double r = 1.0 / std::sqrt(3.0);
        CHECK(std::fabs(n[0] - r) < 1e-14 && std::fabs(n[1] - r) < 1e-14 && std::fabs(n[2] - r) < 1e-14);
        CHECK(ck::jacobi(c, lam, v0, v1, v2));
        CHECK(std::fabs((v0[0] * v1[0] + v0[1] * v1[1]) + v0[2] * v1[2]) < 1e-15 && std::fabs((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2] - 1.0) < 1e-15);
    }
    // duplicates only and collinear points: no plane
    {
        const float dup[4][3] = {{0.25f, -1.5f, 3.0f}, {0.25f, -1.5f, 3.0f}, {0.25f, -1.5f, 3.0f}, {0.25f, -1.5f, 3.0f}};
        const float line[5][3] = {{0, 0, 0}, {1, 2, 3}, {2, 4, 6}, {3, 6, 9}, {-5, -10, -15}};
        double n[3] = {7, 7, 7};
        bool conv;
        CHECK(ck::normal_of(covariance(dup, 4), n, &conv) == ck::DEGENERATE_N && conv && n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
        n[0] = 7;
        CHECK(ck::normal_of(covariance(line, 5), n, &conv) == ck::DEGENERATE_N && conv && n[0] == 0.0);
    }
    // the largest and the smallest fp32: finite covariances, the iteration ends
    {
        const float big = 3.4e38f, d = 1e-45f;
        const float huge[4][3] = {{big, 0, 0}, {-big, big, -big}, {0, -big, big}, {big, big, big}};
        const float small[4][3] = {{d, 0, 0}, {0, 2 * d, 0}, {0, 0, 3 * d}, {d, d, d}};
        double n[3];
        bool conv;
        const ck::Sym3 c = covariance(huge, 4);
        CHECK(std::isfinite(c.xx) && std::isfinite(c.yz) && ck::normal_of(c, n, &conv) == ck::WITH_NORMAL && conv);
        CHECK(std::fabs((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] - 1.0) < 1e-14);
        CHECK(ck::normal_of(covariance(small, 4), n, &conv) == ck::WITH_NORMAL && conv);
    }
    // many matrices over 80 orders of magnitude: every iteration ends well inside the limit, and V diagonalises
    {
        unsigned long long state = 88172645463325252ull;
        for (int t = 0; t < 20000; ++t) {
            double a[6];
            for (int i = 0; i < 6; ++i) {
                state ^= state << 13; state ^= state >> 7; state ^= state << 17;
                a[i] = ((double)(state >> 11) / 9007199254740992.0 - 0.5) * std::pow(10.0, (double)(t % 80) - 40.0);
            }
            const ck::Sym3 c = {a[0] * a[0] + a[1] * a[1], a[0] * a[2], a[1] * a[3], a[2] * a[2] + a[4] * a[4], a[3] * a[4] + a[2] * a[5], a[3] * a[3] + a[5] * a[5]};
            double lam[3], v0[3], v1[3], v2[3];
            if (!ck::jacobi(c, lam, v0, v1, v2)) { std::printf("matrix %d did not converge\n", t); return 1; }
        }
        ++checks;
    }
    // an exactly diagonal matrix rotates nothing; equal eigenvalues go to the lower column
    {
        const ck::Sym3 c = {2.0, 0.0, 0.0, 2.0, 0.0, 5.0};
        double n[3];
        bool conv;
        CHECK(ck::normal_of(c, n, &conv) == ck::WITH_NORMAL && conv && n[0] == 1.0 && n[1] == 0.0 && n[2] == 0.0);
    }
    std::printf("ok %d\n", checks);
    return 0;
}
