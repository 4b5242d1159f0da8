"""The lower bound of the distance to a box alone (csrc/ltm_box_bound.h, no device and no HIP header): a stand-alone program compiled with g++ without
contraction under the address and undefined-behaviour sanitizers and run as a child process.  At every scale from 1e-24 to 1e18 and at the magnitudes of
the RANGE cases of tests/search_cases.py it draws 10^5 triples (box, float point inside the box, query) and checks that the bound never exceeds the float
distance the kernels compare (FLANN's L2_Simple, restated here), that it is 0 for a query inside the box and +inf for the empty box -- and that the
bound as it was before the absolute term, restated here, DOES exceed the float distance at the scales where squares underflow, so that the check is one
that the defect fails.  The upper side likewise (box_upper_bound, box_is_clique: the clique leaves of the cluster kernels): over the same scales no
pair of float points inside a box has a float distance at or above the smallest r2 at which the box is called a clique, a box beyond the float range is
a clique at no r2, and the rule as it was before the absolute term, restated here, does have such pairs at the scales where squares underflow."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include "ltm_box_bound.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// FLANN L2_Simple<float> as sqdist_l2simple (ltm_device_math.h) evaluates it
static float sqdist(float qx, float qy, float qz, float tx, float ty, float tz)
{
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    float r = dx * dx;
    r = r + dy * dy;
    r = r + dz * dz;
    return r;
}
// the bound before the absolute term: the relative shrink alone
static double relative_only(const float* lo, const float* hi, const float* q)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double g = std::fmax(std::fmax((double)lo[a] - (double)q[a], (double)q[a] - (double)hi[a]), 0.0);
        s += g * g;
    }
    return s * (1.0 - 1.0e-6);
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64()      // xorshift64*
{
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return state * 0x2545f4914f6cdd1dull;
}
static double uniform() { return (double)(next_u64() >> 11) * 0x1p-53; }

struct Scale { const char* name; double origin, side; bool huge; bool must_violate; };

// one scale: kTriples triples, returns how often relative_only exceeded the float distance
static long run(const Scale& S)
{
    const int kTriples = 100000;
    long violations = 0, inside = 0;
    for (int t = 0; t < kTriples; ++t) {
        float lo[3], hi[3], p[3], q[3];
        const int mode = (int)(next_u64() % 4);      // 0: query anywhere around, 1: inside the box, 2: a few floats outside a face, 3: far outside
        bool q_inside = true;
        for (int a = 0; a < 3; ++a) {
            float c0 = (float)(S.origin + S.side * uniform()), c1 = (float)(S.origin + S.side * uniform());
            if (S.huge && next_u64() % 8 == 0) c0 = (next_u64() & 1) ? 3e38f : -3e38f;
            lo[a] = std::fmin(c0, c1); hi[a] = std::fmax(c0, c1);
            if (next_u64() % 16 == 0) hi[a] = lo[a];                     // a box that is flat on this axis
            p[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * uniform());
            p[a] = std::fmin(std::fmax(p[a], lo[a]), hi[a]);
            if (next_u64() % 8 == 0) p[a] = (next_u64() & 1) ? lo[a] : hi[a];      // on a face
            switch (mode) {
            case 0: q[a] = (float)(S.origin + S.side * (3.0 * uniform() - 1.0)); break;
            case 1: q[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * uniform()); q[a] = std::fmin(std::fmax(q[a], lo[a]), hi[a]); break;
            case 2: {
                const bool low = (next_u64() & 1) != 0;
                const int steps = (int)(next_u64() % 4);
                q[a] = low ? lo[a] : hi[a];
                for (int s = 0; s < steps; ++s) q[a] = std::nextafter(q[a], low ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity());
                break;
            }
            default: q[a] = (float)(S.origin + S.side * (2000.0 * uniform() - 1000.0)); break;
            }
            CHECK(std::isfinite(lo[a]) && std::isfinite(hi[a]) && std::isfinite(q[a]) && lo[a] <= p[a] && p[a] <= hi[a]);
            q_inside = q_inside && lo[a] <= q[a] && q[a] <= hi[a];
        }
        const double d = (double)sqdist(q[0], q[1], q[2], p[0], p[1], p[2]);
        CHECK(!std::isnan(d));
        const double b = ltm::box_lower_bound(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], q[0], q[1], q[2]);
        if (!(b <= d)) { std::printf("%s: bound %a above the float distance %a\n", S.name, b, d); std::exit(1); }
        CHECK(b >= 0.0);
        if (q_inside) { CHECK(b == 0.0); ++inside; }
        if (relative_only(lo, hi, q) > d) ++violations;
    }
    CHECK(inside > kTriples / 8);
    return violations;
}

// the clique rule before the absolute term: the relative growth alone
static bool clique_relative_only(const float* lo, const float* hi, float r2)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double e = (double)hi[a] - (double)lo[a];
        s += e * e;
    }
    return s * (1.0 + 1.0e-6) < (double)r2;
}
// the smallest float strictly above x (+inf beyond the float range)
static float float_above(double x)
{
    float f = (float)x;
    if (!((double)f > x)) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

// the upper side at one scale: kTriples pairs of float points inside a box; at the smallest r2 at which box_is_clique says yes (and at twice that) the
// float distance of the pair has to be below r2.  Returns how often the rule before the absolute term, at ITS smallest r2, called a box a clique whose
// pair has float d2 >= r2
static long run_upper(const Scale& S)
{
    const int kTriples = 100000;
    const float inf = std::numeric_limits<float>::infinity();
    long violations = 0, cliques = 0;
    for (int t = 0; t < kTriples; ++t) {
        float lo[3], hi[3], p[3], q[3];
        const bool tight = (next_u64() & 1) != 0;      // the box of the two points themselves: what a leaf of two points has
        for (int a = 0; a < 3; ++a) {
            float c0 = (float)(S.origin + S.side * uniform()), c1 = (float)(S.origin + S.side * uniform());
            if (S.huge && next_u64() % 8 == 0) c0 = (next_u64() & 1) ? 3e38f : -3e38f;
            lo[a] = std::fmin(c0, c1); hi[a] = std::fmax(c0, c1);
            if (next_u64() % 16 == 0) hi[a] = lo[a];
            if (tight) {
                const bool up = (next_u64() & 1) != 0;
                p[a] = up ? lo[a] : hi[a]; q[a] = up ? hi[a] : lo[a];
            } else {
                p[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * uniform());
                q[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * uniform());
                p[a] = std::fmin(std::fmax(p[a], lo[a]), hi[a]); q[a] = std::fmin(std::fmax(q[a], lo[a]), hi[a]);
                if (next_u64() % 4 == 0) p[a] = (next_u64() & 1) ? lo[a] : hi[a];
                if (next_u64() % 4 == 0) q[a] = (next_u64() & 1) ? lo[a] : hi[a];
            }
            CHECK(std::isfinite(lo[a]) && std::isfinite(hi[a]) && lo[a] <= p[a] && p[a] <= hi[a] && lo[a] <= q[a] && q[a] <= hi[a]);
        }
        const float d = sqdist(q[0], q[1], q[2], p[0], p[1], p[2]);
        CHECK(!std::isnan(d));
        const double ub = ltm::box_upper_bound(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
        CHECK(ub >= 0x1p-148 && (ub > (double)std::numeric_limits<float>::max() || (double)d <= ub));
        CHECK(!ltm::box_is_clique(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], (float)ub) || (double)(float)ub > ub);
        CHECK(!ltm::box_is_clique(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], 0.0f));
        const float r2 = float_above(ub);
        if (ub > (double)std::numeric_limits<float>::max()) {
            CHECK(r2 == inf && !ltm::box_is_clique(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], inf));      // the float distance may be +inf, below no r2
        } else {
            CHECK(ltm::box_is_clique(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], r2) && ltm::box_is_clique(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], inf));
            if (!(d < r2)) { std::printf("%s: a clique at r2 = %a has a pair with float distance %a\n", S.name, (double)r2, (double)d); std::exit(1); }
            ++cliques;
        }
        double diag = 0.0;
        for (int a = 0; a < 3; ++a) diag += ((double)hi[a] - (double)lo[a]) * ((double)hi[a] - (double)lo[a]);
        const float r2_old = float_above(diag * (1.0 + 1.0e-6));
        if (std::isfinite(r2_old) && r2_old > 0.0f) {
            CHECK(clique_relative_only(lo, hi, r2_old));
            if (!(d < r2_old)) ++violations;
        }
    }
    CHECK(cliques == kTriples || S.huge || S.side > 1e18);      // only boxes beyond the float range have no r2 at which they are cliques
    return violations;
}

// the squares that round UP are those of differences from 2^-75 = 2.6e-23 on (below it a square is 0, and a distance of 0 is below every r2): the
// relative rule alone goes wrong where the sides are a few times that
static bool upper_must_violate(const Scale& S) { return S.side >= 1e-22 && S.side <= 2e-21; }

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    // the upper side: the empty box and a box beyond the float range are no cliques, a point is one at any r2 above the absolute term
    CHECK(!ltm::box_is_clique(inf, inf, inf, -inf, -inf, -inf, inf) && ltm::box_upper_bound(inf, inf, inf, -inf, -inf, -inf) == (double)inf);
    CHECK(!ltm::box_is_clique(-3e38f, 0.0f, 0.0f, 3e38f, 0.0f, 0.0f, inf) && !ltm::box_is_clique(-3e38f, 0.0f, 0.0f, 3e38f, 0.0f, 0.0f, 3e38f));
    CHECK(ltm::box_is_clique(1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 3.0f, 0x1p-147f) && !ltm::box_is_clique(1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 3.0f, 0x1p-148f));
    CHECK(ltm::box_upper_bound(0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 2.0f) == 9.0 * (1.0 + 1.0e-6) + 0x1p-148);
    CHECK(ltm::box_is_clique(0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 2.0f, 9.00001f) && !ltm::box_is_clique(0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 2.0f, 9.0f));
    {   // the pair of tests/walker_cases.py: squares of 2.6, 2.6 and 2.0 denormal units round to 3 + 3 + 2 = r2, the exact diagonal is 7.2 units
        const float c[3] = {(float)(std::sqrt(2.6) * 0x1p-74 * std::sqrt(0.5)), (float)(std::sqrt(2.6) * 0x1p-74 * std::sqrt(0.5)), (float)(std::sqrt(2.0) * 0x1p-74 * std::sqrt(0.5))};
        const float z[3] = {0.0f, 0.0f, 0.0f};
        const float r2 = 8 * 0x1p-149f;
        CHECK(sqdist(c[0], c[1], c[2], 0.0f, 0.0f, 0.0f) == r2);
        CHECK(clique_relative_only(z, c, r2) && !ltm::box_is_clique(0.0f, 0.0f, 0.0f, c[0], c[1], c[2], r2));
    }
    CHECK(ltm::box_lower_bound(inf, inf, inf, -inf, -inf, -inf, 1.0f, -2.0f, 3e38f) == (double)inf);
    CHECK(ltm::box_lower_bound(inf, inf, inf, -inf, -inf, -inf, 0.0f, 0.0f, 0.0f) == (double)inf);
    CHECK(ltm::box_lower_bound(1.0f, 1.0f, 1.0f, 2.0f, 2.0f, 2.0f, 1.5f, 1.0f, 2.0f) == 0.0);
    // a gap of 3 m on one axis: the relative shrink is what is left of it at this size
    CHECK(ltm::box_lower_bound(0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 4.0f, 0.5f, 0.5f) == 9.0 * (1.0 - 1.0e-6) - 0x1p-148);
    static char names[43][16];
    long total = 0, total_upper = 0;
    int n = 0;
    for (int e = -24; e <= 18; ++e, ++n) {
        std::snprintf(names[n], sizeof names[n], "1e%d", e);
        const Scale S{names[n], 0.0, std::pow(10.0, e), false, e <= -22};
        const long v = run(S);
        std::printf("scale %s: the relative bound alone is above the float distance in %ld of 100000 triples\n", S.name, v);
        if (S.must_violate) CHECK(v > 0);
        total += v;
        const long w = run_upper(S);
        std::printf("scale %s: the relative clique rule alone has a pair at or above r2 in %ld of 100000 boxes\n", S.name, w);
        if (upper_must_violate(S)) CHECK(w > 0);
        if (e >= -12) CHECK(w == 0);      // no box drawn at these sides has a diagonal near 2^-63: no square underflows, the relative term alone was right
        total_upper += w;
    }
    const Scale range[] = {
        {"underflow_cube", 0.0, 1e-23, false, true}, {"partial_underflow", 0.0, 2e-22, false, true}, {"partial_underflow_1e22", 0.0, 1e-22, false, true},
        {"denormal_results", 0.0, 1e-20, false, false}, {"overflow", 0.0, 10.0, true, false}, {"collapse", 0.0, 1e30, false, false},
        {"offset_1e7", 1e7 - 3.0, 6.0, false, false}};
    for (const Scale& S : range) {
        const long v = run(S);
        std::printf("case %s: the relative bound alone is above the float distance in %ld of 100000 triples\n", S.name, v);
        if (S.must_violate) CHECK(v > 0);
        const long w = run_upper(S);
        std::printf("case %s: the relative clique rule alone has a pair at or above r2 in %ld of 100000 boxes\n", S.name, w);
        if (upper_must_violate(S)) CHECK(w > 0);
    }
    CHECK(total > 0 && total_upper > 0);
    std::printf("box bound ok\n");
    return 0;
}
"""


def test_box_bound_alone_under_host_sanitizers(tmp_path):
    src = tmp_path / "box_bound_user.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "box_bound_user"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-g", "-O1", "-I", os.path.join(ROOT, "lt-mapper_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "box bound ok" in r.stdout and not r.stderr, r.stdout + r.stderr
