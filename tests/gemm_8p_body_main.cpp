// Driver of tests/test_gemm_8p_body_cpu.py: the main-loop body of the dense 8-phase launches (csrc/gemm_select.hpp: knob gemm_8p_body,
// gemm_8p_two_phase) on the host, no GPU.  One query per input line "M N K epi gemm_t192 gemm_8p_body" (a dense bf16 GEMM, out_T only,
// gemm_variant = 10, every other knob 0), answer "<enumerator> <tag tail> <two-phase body: 0 | 1>".
#include <cstdio>
#include <cstring>

#include "gemm_select.hpp"

static float g_dummy[4];

int main() {
    int M, N, K, epi, t192, body;
    while (std::scanf("%d %d %d %d %d %d", &M, &N, &K, &epi, &t192, &body) == 6) {
        l4p_gemm_desc d;
        std::memset(&d, 0, sizeof d);
        d.A = d.W = (decltype(d.A))g_dummy;
        d.out_T = (decltype(d.out_T))g_dummy;
        d.M = M, d.N = N, d.K = K, d.lda = d.ldw = K, d.ldc = N, d.epi = epi;
        GemmKnobs k;
        std::memset(&k, 0, sizeof k);
        k.gemm_variant = 10, k.gemm_t192 = t192, k.gemm_8p_body = body;
        const char* err = "";
        const GemmForm f = gemm_select(0, 2, d, k, &err);
        char buf[GEMM_TAG_MAX];
        // what launch_form runs: the forced enumerators name their body, the plain ones ask the predicate
        const bool two = f == GEMM_8P_2PH_256x256 || f == GEMM_8P_2PH_256x192 || gemm_8p_two_phase(d, f);
        std::printf("%d %s %d\n", (int)f, gemm_form_tag(f, 1, buf), two ? 1 : 0);
    }
    return 0;
}
