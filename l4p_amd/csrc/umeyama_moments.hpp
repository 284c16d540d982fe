// Closed-form similarity (Umeyama) from accumulated moments, shared by the seam alignment (umeyama.hip, float model) and the
// camera metrics (metrics.hip, double model): the code is one template, so both round their f64 arithmetic alike.
#pragma once
#include "common.hpp"

// -------------------------------------------------------------------------------------------------
// Umeyama similarity from accumulated moments (skimage.transform._geometric._umeyama):
// dst ~ s R src + t.  sums: n, mean_s[3], mean_d[3], cov[3][3] = E[(d-md)(s-ms)^T], var_s.
// -------------------------------------------------------------------------------------------------
static __device__ void jacobi3(double A[3][3], double V[3][3]) {
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

// model: [0..8] = s*R row-major, [9..11] = t, [12] = s
template <typename OutT>
__device__ void umeyama_from_moments(const double ms[3], const double md[3], const double cov[3][3], double var_s,
                                     OutT* model) {
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
    const double dp = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int i = 0; i < 3; ++i) u2[i] -= dp * u1[i];
    const double s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int i = 0; i < 3; ++i) u2[i] /= fmax(s2, 1e-300);
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    // sigma3 with the reflection sign folded in: u3^T cov v3 (negative when det(cov) < 0)
    double s3 = 0;
    for (int i = 0; i < 3; ++i) s3 += u3[i] * (cov[i][0] * v3[0] + cov[i][1] * v3[1] + cov[i][2] * v3[2]);
    const double scale = var_s > 0 ? (s1 + s2 + s3) / var_s : 1.0;
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) model[i * 3 + j] = (OutT)(scale * R[i][j]);
        model[9 + i] = (OutT)(md[i] - scale * (R[i][0] * ms[0] + R[i][1] * ms[1] + R[i][2] * ms[2]));
    }
    model[12] = (OutT)scale;
}
