// A stand-alone host program over csrc/poisson_math.h: the header's rules are plain C++, so they can run under
// -fsanitize=address,undefined on the CPU (tests/test_poisson_cpu.py builds and runs this).  It walks the classes of the points, the
// cell and the weights, the fixed-point terms, the planes, the grid rules and the field over ordinary, degenerate and hostile values
// (NaN, +-inf, 1e30, the largest and the smallest fp32, points on voxel centres and one ulp off) and checks the answers that are known
// exactly.  It prints "ok" and the number of checks; any failed check or sanitizer report ends it with a status != 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "poisson_math.h"

using namespace rcmvs;

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
    const double o[3] = {-1.25, -1.25, -1.25}, h = 0.15625;      // 16^3 over a box of side 2.5: centres and faces are exact in fp32
    const int g[3] = {16, 16, 16};
    const float up[3] = {0.0f, 0.0f, 1.0f};
    po::Cell c;
    // classes, in their order of precedence
    {
        const float p[3] = {0.3f, 0.2f, 0.1f};
        const float bad[][3] = {{nanf_, 0, 1}, {inff, 0, 0}, {0, -inff, 0}};
        for (const auto& n : bad) CHECK(po::classify(p, n, o, h, g, &c) == po::NON_FINITE);
        const float q[][3] = {{nanf_, 0, 0}, {0, inff, 0}, {0, 0, -inff}};
        for (const auto& x : q) CHECK(po::classify(x, up, o, h, g, &c) == po::NON_FINITE);
        const float zero[3] = {-0.0f, 0.0f, -0.0f}, far[3] = {1e30f, 0, 0}, farther[3] = {-3.4e38f, 3.4e38f, 3.4e38f};
        CHECK(po::classify(p, zero, o, h, g, &c) == po::ZERO_NORMAL && po::classify(far, zero, o, h, g, &c) == po::ZERO_NORMAL);
        CHECK(po::classify(far, up, o, h, g, &c) == po::OUTSIDE && po::classify(farther, up, o, h, g, &c) == po::OUTSIDE);
        const float tiny[3] = {1e-45f, 0, 0}, huge[3] = {3.4e38f, -3.4e38f, 3.4e38f};
        CHECK(po::classify(p, tiny, o, h, g, &c) == po::SPLATTED && po::classify(p, huge, o, h, g, &c) == po::SPLATTED);
        CHECK(po::unit_component(tiny, 0) == 1.0 && std::fabs(po::unit_component(huge, 1) + 1.0 / std::sqrt(3.0)) < 1e-15);
        const float n3[3] = {3, 4, 12};
        CHECK(po::unit_component(n3, 0) == 3.0 / 13.0 && po::unit_component(n3, 2) == 12.0 / 13.0);
    }
    // a voxel centre: weight exactly 1 on one corner; a cell face: exactly 1/2 and 1/2; the sum of the weights is 1
    {
        const float centre[3] = {(float)(o[0] + 3.5 * h), (float)(o[1] + 4.5 * h), (float)(o[2] + 5.5 * h)};
        CHECK(po::cell_of(centre, o, h, g, &c) && c.b[0] == 3 && c.b[1] == 4 && c.b[2] == 5);
        CHECK(po::corner_weight(c, 0) == 1.0 && po::corner_voxel(c, 0, g) == 3 + 16 * (4 + 16 * 5) && po::corner_voxel(c, 7, g) == 4 + 16 * (5 + 16 * 6));
        for (int code = 1; code < 8; ++code) CHECK(po::corner_weight(c, code) == 0.0);
        const float face[3] = {(float)(o[0] + 4.0 * h), centre[1], centre[2]};
        CHECK(po::cell_of(face, o, h, g, &c) && po::corner_weight(c, 0) == 0.5 && po::corner_weight(c, 1) == 0.5 && po::corner_weight(c, 2) == 0.0);
        const float any[3] = {0.3f, -0.77f, 1.01f};
        CHECK(po::cell_of(any, o, h, g, &c));
        double s = 0.0, s2 = 0.0;
        for (int code = 0; code < 8; ++code) { s += po::corner_weight(c, code); s2 += po::corner_weight(c, code) * po::corner_weight(c, code); }
        CHECK(std::fabs(s - 1.0) < 1e-15 && s2 >= 0.125);         // the bound behind s <= 8
    }
    // the splattable region: the first voxel centre is in, one ulp below is out; the last voxel centre is out, one ulp below is in
    {
        const float lo = (float)(o[0] + 0.5 * h), hi = (float)(o[0] + 15.5 * h);
        const float a[3] = {lo, 0, 0}, b[3] = {std::nextafterf(lo, -inff), 0, 0}, d[3] = {hi, 0, 0}, e[3] = {std::nextafterf(hi, -inff), 0, 0};
        CHECK(po::cell_of(a, o, h, g, &c) && c.b[0] == 0 && c.w[0][1] == 0.0 && !po::cell_of(b, o, h, g, &c));
        CHECK(!po::cell_of(d, o, h, g, &c) && po::cell_of(e, o, h, g, &c) && c.b[0] == 14 && c.w[0][1] < 1.0);
        const int one[3] = {1, 1, 1}, two[3] = {2, 2, 2};
        const float mid[3] = {0, 0, 0};
        const double oo[3] = {-0.5, -0.5, -0.5};
        CHECK(!po::cell_of(mid, oo, 1.0, one, &c) && po::cell_of(mid, o, 1.25, two, &c) && c.b[0] == 0);
    }
    // fixed point: exact for weights that are dyadic, ties to even, symmetric in the sign
    {
        CHECK(po::density_term(1.0) == 268435456ll && po::density_term(0.5) == 134217728ll && po::density_term(0.0) == 0);
        CHECK(po::density_term(1.5 / 268435456.0) == 2 && po::density_term(2.5 / 268435456.0) == 2 && po::density_term(0.4 / 268435456.0) == 0);
        CHECK(po::normal_term(8.0, 1.0, -1.0) == -2147483648ll && po::normal_term(2.0, 0.3, 0.7) == -po::normal_term(2.0, 0.3, -0.7));
        CHECK(po::colour_term(1.0, 255) == 255ll * 1048576ll && po::colour_term(0.0, 255) == 0);
        CHECK(po::plane_of(268435456ll) == 1.0f && po::plane_of(-134217728ll) == -0.5f && po::plane_of(0) == 0.0f && po::plane_of(1) > 0.0f);
        CHECK(po::plane_of(4611686018427387904ll) == 17179869184.0f);                  // 2^62: the overflow bound is a finite plane
        CHECK(po::colour_of(0, 0) == 128.0f && po::colour_of(200ll * 1048576ll / 2, 134217728ll) == 200.0f && po::colour_of(0, 1) == 0.0f);
        CHECK(po::scale_of(0.125, true) == 8.0 && po::scale_of(0.125, false) == 1.0);
    }
    // the grid rules
    {
        CHECK(po::six(1, 2, 3, 4, 5, 6) == 21.0 && po::rhs(1, 3, 10, 14, 100, 108, 0.5) == 14.0);
        // a constant is not a solution under the mirrored ghost: at a corner three neighbours are -x
        CHECK(po::residual(1.0, po::six(-1, 1, -1, 1, -1, 1), 0.0, 1.0) == 6.0);
        // x = the mean of its neighbours and b = 0: the sweep keeps it, the residual is 0
        CHECK(std::fabs(po::jacobi(2.0, 12.0, 0.0, 1.0) - 2.0) < 1e-15 && po::residual(2.0, 12.0, 0.0, 1.0) == 0.0);
        CHECK(std::fabs(po::jacobi(0.0, 0.0, 7.0, 4.0) + (6.0 / 7.0) * 28.0 / 6.0) < 1e-15);
        CHECK(po::prolong_axis(4.0, 8.0) == 5.0 && po::prolong_axis(4.0, -4.0) == 2.0);
        CHECK(po::OMEGA == 6.0 / 7.0 && po::COARSEST_SWEEPS == 64);
    }
    // the field
    {
        CHECK(po::field_value(1.5f, 0.25) == 1.25f && po::field_value(0.0f, 0.0) == 0.0f);
        const float d = 0.37f;
        CHECK(po::field_weight(d, (double)d) == 1.0f && po::field_weight(d, std::nextafter((double)d, 1.0)) == 0.0f && po::field_weight(0.0f, 0.0) == 1.0f);
    }
    std::printf("ok %d\n", checks);
    return 0;
}
