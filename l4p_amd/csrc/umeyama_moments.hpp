// Closed-form similarity (Umeyama) from accumulated moments, shared by the seam alignment (umeyama.hip, float model) and the
// camera metrics (metrics.hip, double model): the code is one template, so both round their f64 arithmetic alike.
// Plain C++ apart from the __device__ mark (fabs, sqrt and fmax are all it calls), so a host compiler takes it too:
// tests/umeyama_moments_main.cpp runs it on the CPU against a float64 SVD (tests/test_umeyama_moments_cpu.py).
#pragma once
#if defined(__HIPCC__)
#include "common.hpp"
#define UMEYAMA_FN __device__
#else
#include <math.h>
#define UMEYAMA_FN
#endif

// -------------------------------------------------------------------------------------------------
// Umeyama similarity from accumulated moments (skimage.transform._geometric._umeyama):
// dst ~ s R src + t.  sums: n, mean_s[3], mean_d[3], cov[3][3] = E[(d-md)(s-ms)^T], var_s.
// -------------------------------------------------------------------------------------------------
static UMEYAMA_FN void jacobi3(double A[3][3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j;
    for (int sweep = 0; sweep < 30; ++sweep) {
        if (fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]) < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double x = A[k][p], y = A[k][q];
                    A[k][p] = c * x - s * y;
                    A[k][q] = s * x + c * y;
                }
                for (int k = 0; k < 3; ++k) {
                    const double x = A[p][k], y = A[q][k];
                    A[p][k] = c * x - s * y;
                    A[q][k] = s * x + c * y;
                }
                for (int k = 0; k < 3; ++k) {
                    const double x = V[k][p], y = V[k][q];
                    V[k][p] = c * x - s * y;
                    V[k][q] = s * x + c * y;
                }
            }
    }
}

// The rotation of the closed form on its own: R (a proper rotation at every rank of cov, I for cov = 0) and the sum of the singular
// values with the reflection sign folded into the third, sigma1 + sigma2 +- sigma3 = tr(R^T cov).  Nothing here is divided by a
// variance or multiplied by a scale, so a caller that wants a rigid motion (csrc/object_motion.hip) takes R as it stands;
// tests/umeyama_rotation_main.cpp runs this entry on the CPU against the float64 SVD.
static UMEYAMA_FN void umeyama_rotation(const double cov[3][3], double R[3][3], double* sigma_sum) {
    double AtA[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) AtA[i][j] = cov[0][i] * cov[0][j] + cov[1][i] * cov[1][j] + cov[2][i] * cov[2][j];
    jacobi3(AtA, V);
    int o[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (AtA[o[b]][o[b]] > AtA[o[a]][o[a]]) {
                const int t = o[a];
                o[a] = o[b];
                o[b] = t;
            }
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) {
        v1[i] = V[i][o[0]];
        v2[i] = V[i][o[1]];
    }
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    for (int i = 0; i < 3; ++i) {
        u1[i] = cov[i][0] * v1[0] + cov[i][1] * v1[1] + cov[i][2] * v1[2];
        u2[i] = cov[i][0] * v2[0] + cov[i][1] * v2[1] + cov[i][2] * v2[2];
    }
    const double s1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    for (int i = 0; i < 3; ++i) u1[i] /= fmax(s1, 1e-300);
    // Rank-deficient cov (a full-rank one takes neither branch below, and nothing it computes has moved): R is a proper rotation all
    // the same, completed from the orthonormal v's.  cov = 0 (a static dst or src), or so small that the floor above left u1 short
    // of a unit vector: u1 = v1, hence u2 = v2 below and R = I.
    if (!(s1 >= 1e-300))
        for (int i = 0; i < 3; ++i) u1[i] = v1[i];
    const double dp = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int i = 0; i < 3; ++i) u2[i] -= dp * u1[i];
    double s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int i = 0; i < 3; ++i) u2[i] /= fmax(s2, 1e-300);
    // u2 did not survive the orthogonalisation: it is exactly zero (collinear centres along a coordinate axis: two rows or columns
    // of cov are zero and cov v2 - dp u1 cancels exactly, which left R = u1 v1^T with det 0), or it is rounding noise.  The three
    // products and two sums of a row of cov v2 round by up to 3 eps |cov row| <= 3 eps sigma1 each, 3 sqrt(3) eps sigma1 over the
    // three rows, and v2 itself carries some eps of v1 out of the Jacobi sweeps, which cov turns into as much again: below
    // 16 eps sigma1 the direction of what is left says nothing about the data, and taking it for zero moves s by 16 eps at most.
    // Rank 1 leaves the rotation about u1 free; it is fixed by sending v2 to its own projection off u1 while at least sqrt(1/2) of
    // it stands off u1, and v3 otherwise (|u1.v2|^2 + |u1.v3|^2 <= 1, so then at least sqrt(1/2) of v3 does).  With u1 = v1 this is
    // u2 = v2, u3 = v3 and R = I, and R moves continuously with u1 around there (a choice by the smaller of the two products would
    // flip between v2 and v3 on their rounding).
    if (!(s2 > 16.0 * 2.220446049250313e-16 * s1)) {
        const double d2 = u1[0] * v2[0] + u1[1] * v2[1] + u1[2] * v2[2], d3 = u1[0] * v3[0] + u1[1] * v3[1] + u1[2] * v3[2];
        const bool keep2 = fabs(d2) <= 0.7071067811865476;
        const double* w = keep2 ? v2 : v3;
        const double dw = keep2 ? d2 : d3;
        for (int i = 0; i < 3; ++i) u2[i] = w[i] - dw * u1[i];
        const double nw = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        for (int i = 0; i < 3; ++i) u2[i] /= nw;
        s2 = 0;  // u2^T cov v2 of the completed u2: what the scale that fits this R best takes for sigma2
        for (int i = 0; i < 3; ++i) s2 += u2[i] * (cov[i][0] * v2[0] + cov[i][1] * v2[1] + cov[i][2] * v2[2]);
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    // sigma3 with the reflection sign folded in: u3^T cov v3 (negative when det(cov) < 0)
    double s3 = 0;
    for (int i = 0; i < 3; ++i) s3 += u3[i] * (cov[i][0] * v3[0] + cov[i][1] * v3[1] + cov[i][2] * v3[2]);
    *sigma_sum = s1 + s2 + s3;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
}

// model: [0..8] = s*R row-major, [9..11] = t, [12] = s
template <typename OutT>
UMEYAMA_FN void umeyama_from_moments(const double ms[3], const double md[3], const double cov[3][3], double var_s,
                                     OutT* model) {
    double R[3][3], sigma_sum;
    umeyama_rotation(cov, R, &sigma_sum);
    const double scale = var_s > 0 ? sigma_sum / var_s : 1.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) model[i * 3 + j] = (OutT)(scale * R[i][j]);
        model[9 + i] = (OutT)(md[i] - scale * (R[i][0] * ms[0] + R[i][1] * ms[1] + R[i][2] * ms[2]));
    }
    model[12] = (OutT)scale;
}
