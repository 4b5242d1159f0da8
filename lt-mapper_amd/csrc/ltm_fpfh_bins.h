// ltm_fpfh_bins.h -- the bin rules of the FPFH descriptors (include/ltm.h, "fpfh"): 11 bins per feature.  Compiles for the host as well, so that the very
// same expressions can be checked alone.  The theta bin needs no atan2: PCL's floor(11 (theta + pi) / 2 pi) is the number of boundaries
// theta_j = -pi + 2 pi j / 11, j = 1 .. 10, that theta = atan2(y, x) has reached, and whether a boundary is reached is the sign of a cross product with its
// direction (c_j, s_j) = (cos theta_j, sin theta_j) together with the half plane of y.  tools/fpfh_numpy.py carries a copy of the table.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LTM_FB_FN __host__ __device__ __forceinline__
#else
#define LTM_FB_FN inline
#endif

namespace ltm {

static constexpr int kFpfhBins = 11;        // per feature
static constexpr int kFpfhSize = 33;        // floats of a descriptor: alpha, phi, theta

// (c_j, s_j) of boundary j at entry j - 1: the doubles nearest cos and sin of -pi + 2 pi j / 11
#define LTM_FPFH_THETA_TABLE(X)                             \
    X(-0.8412535328311811, -0.5406408174555978)             \
    X(-0.4154150130018863, -0.9096319953545184)             \
    X(0.14231483827328512, -0.9898214418809327)             \
    X(0.6548607339452851, -0.7557495743542583)              \
    X(0.9594929736144975, -0.2817325568414295)              \
    X(0.9594929736144975, 0.2817325568414295)               \
    X(0.6548607339452851, 0.7557495743542583)               \
    X(0.14231483827328512, 0.9898214418809327)              \
    X(-0.41541501300188616, 0.9096319953545186)             \
    X(-0.8412535328311813, 0.5406408174555974)

// the sign bit of a double: set for -0.0 too
LTM_FB_FN bool fpfh_sign_bit(double v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __double_as_longlong(v) < 0;
#else
    int64_t b;
    memcpy(&b, &v, sizeof b);
    return b < 0;
#endif
}

// alpha and phi, both in [-1, 1] up to rounding: floor(11 ((f + 1) 0.5)) clamped to 0 .. 10
LTM_FB_FN int fpfh_bin_unit(double f)
{
    const double t = 11.0 * ((f + 1.0) * 0.5);
    return t >= 11.0 ? 10 : (t >= 1.0 ? (int)t : 0);      // (int) truncates: the floor of a t >= 1
}

// theta = atan2(y, x) without it.  `upper` is the half plane y > 0 or y == +0.  A boundary below the x axis (j <= 5) is reached in the upper half plane
// always and in the lower one iff c_j y - s_j x >= 0; a boundary above it (j >= 6) is reached in the upper half plane iff c_j y - s_j x >= 0 and never in
// the lower one.  x == y == 0 (either sign): bin 5
LTM_FB_FN int fpfh_bin_theta(double y, double x)
{
    if (x == 0.0 && y == 0.0) return 5;
    const bool upper = !fpfh_sign_bit(y);
    int bin = 0, j = 1;
#define LTM_FPFH_STEP(c, s)                                                     \
    {                                                                           \
        const bool side = (c) * y - (s) * x >= 0.0;                             \
        bin += (j <= 5 ? (upper || side) : (upper && side)) ? 1 : 0;            \
        ++j;                                                                    \
    }
    LTM_FPFH_THETA_TABLE(LTM_FPFH_STEP)
#undef LTM_FPFH_STEP
    return bin;
}

} // namespace ltm
