// The per-pair and per-structure arithmetic of the chain-statistics kernels (polymer_kernels.hip), in plain float64 C++
// without device intrinsics: the same text compiles for the host (a stand-alone program can hold the Jacobi iteration
// against a library eigensolver) and for one lane of a kernel.  Compiled with -ffp-contract=off wherever it is included:
// one rounding per operation, in the order written here.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define POLY_HD __host__ __device__ inline
#else
#define POLY_HD inline
#endif

// The squared distance of two fp32 positions: the coordinates converted exactly, i the atom at the lower chain position,
//   dx = x_j - x_i per component, r2 = (dx*dx + dy*dy) + dz*dz
// Five roundings.  The kernels continue with r = sqrt(r2) and 1.0 / r, both correctly rounded.
POLY_HD double poly_dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const double dx = (double)xj - (double)xi, dy = (double)yj - (double)yi, dz = (double)zj - (double)zi;
    return (dx * dx + dy * dy) + dz * dz;
}

// The eigenvalues of a symmetric 3x3 by cyclic Jacobi, ens_jacobi4's iteration (ensemble_math.h; Golub & Van Loan 8.4)
// without the eigenvectors: A <- J^T A J row-cyclically over (0,1), (0,2), (1,2), the full matrix used and overwritten,
// its diagonal the eigenvalues when it returns.  A sweep starts only while off(A)^2 exceeds 2^-120 ||A||_F^2
// (CODLAD_POLYMER_JACOBI_STOP = 2^-60 of the norm is what may be left); a diagonal matrix - a rod along an axis, a cube -
// returns at once with its diagonal untouched.  NaN in, NaN out.
POLY_HD void poly_jacobi3(double A[3][3]) {
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            diag += A[p][p] * A[p][p];
#pragma unroll
            for (int q = p + 1; q < 3; ++q) off += 2.0 * A[p][q] * A[p][q];
        }
        if (off <= 0x1p-120 * (diag + off)) return;
        // p, q, k unrolled: constant indices keep A in registers on the device
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = tau >= 0.0 ? 1.0 / (tau + sqrt(1.0 + tau * tau)) : -1.0 / (-tau + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {                       // A <- A J
                    const double x = A[k][p], y = A[k][q];
                    A[k][p] = c * x - s * y;
                    A[k][q] = s * x + c * y;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {                       // A <- J^T A
                    const double x = A[p][k], y = A[q][k];
                    A[p][k] = c * x - s * y;
                    A[q][k] = s * x + c * y;
                }
                A[p][q] = A[q][p] = 0.0;                            // what the rotation was chosen for, exactly
            }
        }
    }
}

// tensor (xx, yy, zz, xy, xz, yz) -> its eigenvalues in ascending order, each clamped at 0 (rounding below zero of a
// positive semi-definite matrix; NaN stays NaN)
POLY_HD void poly_eigenvalues(const double t[6], double e[3]) {
    double A[3][3] = {{t[0], t[3], t[4]}, {t[3], t[1], t[5]}, {t[4], t[5], t[2]}};
    poly_jacobi3(A);
    double a = A[0][0], b = A[1][1], c = A[2][2], h;
    if (b < a) h = a, a = b, b = h;
    if (c < b) h = b, b = c, c = h;
    if (b < a) h = a, a = b, b = h;
    e[0] = a < 0.0 ? 0.0 : a;
    e[1] = b < 0.0 ? 0.0 : b;
    e[2] = c < 0.0 ? 0.0 : c;
}
