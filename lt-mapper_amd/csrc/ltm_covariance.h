// ltm_covariance.h -- the smallest principal axis of a set of points from its moments, in double: covariance, cyclic Jacobi, unit length, canonical sign
// (include/ltm.h, "normals").  Shared by the kernel units that fit planes: surface normals (ltm_k_normals.hip) and the refinement of plane segmentation
// (ltm_k_plane.hip).  Internal linkage, like ltm_search_walk.h; the arithmetic and its order are part of the interface of both sections.
#pragma once
#include <hip/hip_runtime.h>

namespace ltm {
namespace {

// s: the sums of the n differences d from a reference point, c: the sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz.
// Out: the unit eigenvector of the smallest eigenvalue (the lower axis among equals), component of largest magnitude positive (the lower axis among
// equals); lam: the three eigenvalues in the order of the axes they ended on; returns the axis of the smallest.
__device__ inline int smallest_axis_from_moments(const double* s, const double* c, int n, double& nx, double& ny, double& nz, double lam[3])
{
    const double inv = 1.0 / (double)n;
    const double mx = s[0] * inv, my = s[1] * inv, mz = s[2] * inv;
    double A[3][3], V[3][3];
    A[0][0] = c[0] * inv - mx * mx; A[0][1] = c[1] * inv - mx * my; A[0][2] = c[2] * inv - mx * mz;
    A[1][1] = c[3] * inv - my * my; A[1][2] = c[4] * inv - my * mz; A[2][2] = c[5] * inv - mz * mz;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) V[r][k] = r == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int i = 0; i < 2; ++i)
            for (int j = i + 1; j < 3; ++j) {
                const double apq = A[i][j];
                if (apq == 0.0 || fabs(apq) <= 1.0e-17 * sqrt(fabs(A[i][i] * A[j][j]))) continue;
                rotated = true;
                const double theta = (A[j][j] - A[i][i]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                const int l = 3 - i - j;      // the third axis
                const double aii = A[i][i], ajj = A[j][j], ail = A[i][l], ajl = A[j][l];
                A[i][i] = aii - t * apq; A[j][j] = ajj + t * apq;
                A[i][j] = A[j][i] = 0.0;
                A[i][l] = A[l][i] = cs * ail - sn * ajl;
                A[j][l] = A[l][j] = sn * ail + cs * ajl;
                for (int k = 0; k < 3; ++k) {
                    const double vi = V[k][i], vj = V[k][j];
                    V[k][i] = cs * vi - sn * vj; V[k][j] = sn * vi + cs * vj;
                }
            }
        if (!rotated) break;
    }
    int e = 0;      // the smallest eigenvalue, the lower axis among equals
    if (A[1][1] < A[e][e]) e = 1;
    if (A[2][2] < A[e][e]) e = 2;
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
    nx = V[0][e]; ny = V[1][e]; nz = V[2][e];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len; ny /= len; nz /= len;
    // canonical sign: the component of largest magnitude is positive, the lower axis among equals
    double big = nx;
    if (fabs(ny) > fabs(big)) big = ny;
    if (fabs(nz) > fabs(big)) big = nz;
    if (big < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    return e;
}

} // namespace
} // namespace ltm
