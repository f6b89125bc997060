// The per-pair tail of the superposition kernels (ensemble_kernels.hip): Horn's 4x4 matrix of the 3x3 correlation
// S = sum (a - ca)(b - cb)^T, its largest eigenpair by cyclic Jacobi, the rotation of the unit quaternion and the
// translation.  Plain fp64 C++ without device intrinsics, so the same text compiles for the host (a stand-alone check
// program can run it against an SVD) and for one lane of the kernel.
#pragma once

#ifdef __HIPCC__
#define ENS_HD __host__ __device__ inline
#else
#define ENS_HD inline
#endif

// Cyclic Jacobi on a symmetric 4x4 as Golub & Van Loan state it (Matrix Computations, 8.4: the symmetric Schur
// decomposition of the (p, q) plane, A <- J^T A J row-cyclically, V <- V J): the full matrix A is used and overwritten,
// its diagonal ends as the eigenvalues, V's columns as the eigenvectors.  A sweep starts only while off(A)^2 exceeds
// 2^-120 ||A||_F^2; convergence is quadratic, so what is left then is below 2^-60 ||A|| - scale-free, a matrix of 1e-30
// converges like one of 1e+12, and a zero matrix returns at once with V = I.  Repeated and zero eigenvalues (planar,
// collinear, identical inputs) are no special case, where Newton's iteration on the characteristic polynomial stalls.
// NaN in, NaN out: no comparison here can hide one.
ENS_HD void ens_jacobi4(double A[4][4], double V[4][4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            diag += A[p][p] * A[p][p];
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += 2.0 * A[p][q] * A[p][q];
        }
        if (off <= 0x1p-120 * (diag + off)) return;
        // p, q, k unrolled: constant indices keep A and V in registers on the device
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0.0) continue;
                // (c, s) with the (p, q) element of J^T A J zero, the smaller root of t^2 + 2 tau t - 1 = 0
                const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = tau >= 0.0 ? 1.0 / (tau + sqrt(1.0 + tau * tau)) : -1.0 / (-tau + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                       // A <- A J
                    const double x = A[k][p], y = A[k][q];
                    A[k][p] = c * x - s * y;
                    A[k][q] = s * x + c * y;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {                       // A <- J^T A
                    const double x = A[p][k], y = A[q][k];
                    A[p][k] = c * x - s * y;
                    A[q][k] = s * x + c * y;
                }
                A[p][q] = A[q][p] = 0.0;                            // what the rotation was chosen for, exactly
#pragma unroll
                for (int k = 0; k < 4; ++k) {                       // V <- V J
                    const double x = V[k][p], y = V[k][q];
                    V[k][p] = c * x - s * y;
                    V[k][q] = s * x + c * y;
                }
            }
        }
    }
}

// S[r][c] = sum (a_r - ca_r)(b_c - cb_c); Ga, Gb = sum |a - ca|^2, sum |b - cb|^2; n = atoms summed over.
// -> msd = max(Ga + Gb - 2 lambda, 0) / n with lambda the largest eigenvalue of Horn's matrix (Horn 1987, eq. for N),
// equal to s1 + s2 + sign(det S) s3 of the SVD route: the maximum is over proper rotations only.
// Rt (may be null) = R row-major [9] then t [3], with R a + t superposed on b.
ENS_HD double ens_solve_pair(const double S[9], double Ga, double Gb, const double ca[3], const double cb[3], double n,
                             double *Rt) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4];
    ens_jacobi4(N, V);
    double lam = N[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};     // the largest eigenpair, first of equals
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (N[i][i] > lam) {
            lam = N[i][i];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = V[k][i];
        }
    const double e = Ga + Gb - 2.0 * lam;
    const double msd = (e < 0.0 ? 0.0 : e) / n;       // rounding below zero is clamped; NaN (a non-finite coordinate) stays NaN
    if (Rt) {
        double w = q[0], x = q[1], y = q[2], z = q[3];
        const double nq = sqrt(w * w + x * x + y * y + z * z);     // 1 up to rounding: V is a product of rotations
        w /= nq; x /= nq; y /= nq; z /= nq;
        const double R[9] = {w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                             2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x),
                             2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rt[3 * r + c] = R[3 * r + c];
            Rt[9 + r] = cb[r] - (R[3 * r] * ca[0] + R[3 * r + 1] * ca[1] + R[3 * r + 2] * ca[2]);
        }
    }
    return msd;
}
