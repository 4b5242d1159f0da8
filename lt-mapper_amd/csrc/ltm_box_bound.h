// ltm_box_bound.h -- the lower bound of the squared distance from a query to an axis-aligned box of the search index (box_lb of ltm_search_walk.h, hence
// every walk of the box tree), in a form that also compiles for the host so that the very same arithmetic can be checked against the float distance it has
// to stay below (tests/test_box_bound_cpu.py).  Its counterpart, the upper bound over the pairs of points inside a box behind the clique leaves of
// ltm_k_cluster.hip, follows it below.
//
// What it has to bound: the distance the kernels compare, FLANN's L2_Simple in float without contraction (sqdist_l2simple),
//     d = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)),  dx = fl(qx - px), ...
// for every point p inside the box [lo, hi].  With u = 2^-24 (round to nearest):
//  - a float difference is (qx - px)(1 + e), |e| <= u, and exact when it is denormal: a difference never underflows;
//  - a float product is dx*dx (1 + e) + h with |e| <= u and, once the result is below 2^-126, an ABSOLUTE error |h| <= 2^-150 (half the spacing 2^-149
//    of the denormals; a square below 2^-150 becomes 0).  Only the three squares can underflow;
//  - a float sum of two non-negative terms is (a + b)(1 + e), |e| <= u, and exact when it is denormal.
// So d >= D (1 - u)^5 - 3 * 2^-150 >= D (1 - 3e-7) - 1.5 * 2^-149, D the exact squared distance of the two float points, and D >= G, the exact squared
// gap between q and the box.  The double evaluation below has exact differences (floats in double) and a relative error of a few 2^-53 in G, far inside
// the slack between 3e-7 and 1e-6.  The relative shrink alone was the bound until the underflow term was found missing: for a target inside a cube of
// side 1e-23 every float distance is 0 while G is around 1e-46 > 0, and every far leaf was skipped although all its points tie with the k-th.
// kBoxBoundAbs = 2^-148 covers the 1.5 * 2^-149 with the same kind of margin; the result is clamped at 0 (a query inside the box has bound 0, as before),
// and the empty box (+inf, -inf) keeps +inf.  Above G = 2^-148 / 1e-6 = 3e-39 the relative shrink is the larger of the two terms, and a decision moves
// only where a bound lies within 2.8e-45 of the distance it is compared with: nothing a cloud measured in metres decides changes.  (A device that flushed float denormals to zero would need 3 * 2^-126 here; the library is built with
// denormals on, the default for gfx9, and tests/test_gpu_search_edges.py, case denormal_results, would show the difference.)
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LTM_BB_FN __host__ __device__ __forceinline__
#else
#define LTM_BB_FN inline
#endif

namespace ltm {

static constexpr double kBoxBoundRel = 1.0e-6;
static constexpr double kBoxBoundAbs = 0x1p-148;

// lower bound, in double, of sqdist_l2simple(q, p) over every float point p with lo <= p <= hi (component-wise); +inf for the empty box (+inf, -inf)
LTM_BB_FN double box_lower_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz)
{
    const double gx = fmax(fmax((double)lox - (double)qx, (double)qx - (double)hix), 0.0);
    const double gy = fmax(fmax((double)loy - (double)qy, (double)qy - (double)hiy), 0.0);
    const double gz = fmax(fmax((double)loz - (double)qz, (double)qz - (double)hiz), 0.0);
    return fmax((gx * gx + gy * gy + gz * gz) * (1.0 - kBoxBoundRel) - kBoxBoundAbs, 0.0);
}

// The upper side, the counterpart of box_lower_bound: an upper bound, in double, of sqdist_l2simple(p, q) over every pair of float points p, q with
// lo <= p, q <= hi -- what the cluster kernels compare with r2 to call a leaf a clique (every pair inside it adjacent under float d2 < r2).
// The same three facts read the other way: the differences are exact or carry a relative u, each square is dx*dx (1 + e) + h with |h| <= 2^-150 once it is
// below 2^-126 (a square can round UP to the next denormal: 2.6 * 2^-149 becomes 3 * 2^-149), the sums carry a relative u or are exact.  So
//     d <= D (1 + u)^5 + 3 * 2^-150 <= D (1 + 3e-7) + 1.5 * 2^-149,
// and D <= E, the exact squared diagonal of the box.  The double evaluation of E has exact differences and a relative error of a few 2^-53, inside the slack
// between 3e-7 and 1e-6; kBoxBoundAbs = 2^-148 covers the 1.5 * 2^-149 as it does below.  The relative growth alone was the rule of the cluster kernels
// until this term was added: two points whose exact squared distance is 7.2 * 2^-149 have float d2 = 8 * 2^-149 (3 + 3 + 2 units), which is not below
// r2 = 8 * 2^-149, yet 7.2 * 2^-149 * (1 + 1e-6) is.  Above E = 3e-39 the relative term is the larger one and nothing measured in metres moves.
// The empty box (+inf, -inf) has the bound +inf.  A box of finite floats has a finite bound in double even where the float distance overflows to +inf.
LTM_BB_FN double box_upper_bound(float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const double ex = (double)hix - (double)lox, ey = (double)hiy - (double)loy, ez = (double)hiz - (double)loz;
    return (ex * ex + ey * ey + ez * ez) * (1.0 + kBoxBoundRel) + kBoxBoundAbs;
}

// every pair of float points inside the box is adjacent under float d2 < r2.  An upper bound beyond the float range is never a clique, whatever r2: the
// float distance of such a pair may be +inf, which is below no r2.
LTM_BB_FN bool box_is_clique(float lox, float loy, float loz, float hix, float hiy, float hiz, float r2)
{
    const double ub = box_upper_bound(lox, loy, loz, hix, hiy, hiz);
    return ub < (double)r2 && ub <= 3.4028234663852886e38;
}

} // namespace ltm
