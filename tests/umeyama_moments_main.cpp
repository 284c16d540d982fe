// Driver of tests/test_umeyama_moments_cpu.py: the closed-form similarity of csrc/umeyama_moments.hpp on the host, no GPU.  Reads
// point sets "n" then n lines "sx sy sz dx dy dz" from stdin until it ends, forms the moments the way met_cameras_kernel and the
// RANSAC kernels do (means, then centred sums, then the division by n, all in double) and prints two lines of 13 values per set: the
// model for OutT = double (%.17g) and for OutT = float (%.9g).
#include <cstdio>
#include <vector>

#include "umeyama_moments.hpp"

int main() {
    int n;
    while (std::scanf("%d", &n) == 1 && n > 0) {
        std::vector<double> p((size_t)n * 6);
        for (double& x : p)
            if (std::scanf("%lf", &x) != 1) return 1;
        double ms[3] = {0, 0, 0}, md[3] = {0, 0, 0}, cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var = 0;
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < 3; ++k) {
                ms[k] += p[(size_t)j * 6 + k];
                md[k] += p[(size_t)j * 6 + 3 + k];
            }
        for (int k = 0; k < 3; ++k) {
            ms[k] /= n;
            md[k] /= n;
        }
        for (int j = 0; j < n; ++j) {
            double ds[3], dd[3];
            for (int k = 0; k < 3; ++k) {
                ds[k] = p[(size_t)j * 6 + k] - ms[k];
                dd[k] = p[(size_t)j * 6 + 3 + k] - md[k];
                var += ds[k] * ds[k];
            }
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) cov[a][b] += dd[a] * ds[b];
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) cov[a][b] /= n;
        var /= n;
        double m64[13];
        float m32[13];
        umeyama_from_moments<double>(ms, md, cov, var, m64);
        umeyama_from_moments<float>(ms, md, cov, var, m32);
        for (int k = 0; k < 13; ++k) std::printf("%.17g%c", m64[k], k == 12 ? '\n' : ' ');
        for (int k = 0; k < 13; ++k) std::printf("%.9g%c", (double)m32[k], k == 12 ? '\n' : ' ');
    }
    return 0;
}
