// Driver of tests/test_object_motion_cpu.py: the rotation entry of csrc/umeyama_moments.hpp (umeyama_rotation, what
// csrc/object_motion.hip calls) on the host, no GPU.  Reads point sets "n" then n lines "sx sy sz dx dy dz" from stdin until it ends,
// forms the covariance the way tests/umeyama_moments_main.cpp does (means, then centred sums, then the division by n, all in double)
// and prints one line of 10 values per set (%.17g): R row-major, then the signed sum of the singular values.
#include <cstdio>
#include <vector>

#include "umeyama_moments.hpp"

int main() {
    int n;
    while (std::scanf("%d", &n) == 1 && n > 0) {
        std::vector<double> p((size_t)n * 6);
        for (double& x : p)
            if (std::scanf("%lf", &x) != 1) return 1;
        double ms[3] = {0, 0, 0}, md[3] = {0, 0, 0}, cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < 3; ++k) {
                ms[k] += p[(size_t)j * 6 + k];
                md[k] += p[(size_t)j * 6 + 3 + k];
            }
        for (int k = 0; k < 3; ++k) {
            ms[k] /= n;
            md[k] /= n;
        }
        for (int j = 0; j < n; ++j)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) cov[a][b] += (p[(size_t)j * 6 + 3 + a] - md[a]) * (p[(size_t)j * 6 + b] - ms[b]);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) cov[a][b] /= n;
        double R[3][3], sigma_sum;
        umeyama_rotation(cov, R, &sigma_sum);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) std::printf("%.17g ", R[a][b]);
        std::printf("%.17g\n", sigma_sum);
    }
    return 0;
}
