// Driver of tests/test_gemm_select_cpu.py: csrc/gemm_select.hpp on the host, no GPU.  One query per input line, answer per line.
//
//   gemm  es=2 mode=0 M=200 N=72 ... k.gemm_variant=10 ...     ->  "<tag tail>"   (mode 2: "K<mean_k> <tag tail>")
//   group es=2 M=.. N=.. ; M=.. N=.. k.gemm_group=1 ...         ->  "group: <tag tail>"
//   a refusal                                                  ->  "invalid: <error text>"
//
// name=value sets an integer field of l4p_gemm_desc (a pointer field: 0 = NULL, else a dummy address that nothing dereferences),
// k.name=value a field of GemmKnobs, ";" starts the next member of a group.  Fields not named are 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gemm_select.hpp"

#define DESC_INTS(X)                                                                                                                    \
    X(lda) X(ldw) X(M) X(N) X(K) X(Ti) X(Hi) X(Wi) X(Cin) X(To) X(Ho) X(Wo) X(st) X(sh) X(sw) X(relu_in) X(act) X(res_f32) X(ldr)        \
    X(res_mod) X(ldc) X(epi) X(S) X(H) X(Dp) X(kt) X(kh) X(kw) X(Cout) X(a_gr) X(a_gs) X(a_go) X(c_gr) X(c_gs) X(c_go) X(splitk)         \
    X(hyper_rows) X(tuning) X(w_gr) X(w_gs) X(b_gs) X(o_gs) X(ups_hi) X(ups_wi) X(kw_cols) X(kw_len)
#define DESC_PTRS(X) X(A) X(W) X(bias) X(res1) X(res2) X(out_f32) X(out_T) X(vt) X(out_relu_T) X(k_tiled) X(partial) X(hyper)
#define KNOBS(X) \
    X(gemm_variant) X(conv_halo) X(gemm_skinny) X(skinny_max_m) X(gemm_deep) X(gemm_group) X(track_deep) X(gemm_t192) X(gemm_4w) X(probe_kernels)

static float g_dummy[4];

static bool set_desc(l4p_gemm_desc& d, const std::string& name, long long v) {
#define X(f) \
    if (name == #f) { d.f = (decltype(d.f))v; return true; }
    DESC_INTS(X)
#undef X
#define X(f) \
    if (name == #f) { d.f = v ? (decltype(d.f))g_dummy : nullptr; return true; }
    DESC_PTRS(X)
#undef X
    return false;
}

static bool set_knob(GemmKnobs& k, const std::string& name, long long v) {
#define X(f) \
    if (name == #f) { k.f = (int)v; return true; }
    KNOBS(X)
#undef X
    return false;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        if (!(in >> kind)) continue;
        std::vector<l4p_gemm_desc> descs(1);
        std::memset(&descs[0], 0, sizeof(l4p_gemm_desc));
        GemmKnobs knobs;
        std::memset(&knobs, 0, sizeof knobs);
        long long es = 2, mode = 0;
        while (in >> tok) {
            if (tok == ";") {
                descs.emplace_back();
                std::memset(&descs.back(), 0, sizeof(l4p_gemm_desc));
                continue;
            }
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "bad token '%s'\n", tok.c_str());
                return 2;
            }
            const std::string name = tok.substr(0, eq);
            const long long v = std::strtoll(tok.c_str() + eq + 1, nullptr, 10);
            bool ok = true;
            if (name == "es")
                es = v;
            else if (name == "mode")
                mode = v;
            else if (name.rfind("k.", 0) == 0)
                ok = set_knob(knobs, name.substr(2), v);
            else
                ok = set_desc(descs.back(), name, v);
            if (!ok) {
                std::fprintf(stderr, "unknown field '%s'\n", name.c_str());
                return 2;
            }
        }
        const char* err = "";
        if (kind == "group") {
            const GemmGroupForm g = gemm_group_select(descs.data(), (int)descs.size(), knobs, &err);
            if (g == GEMM_GROUP_INVALID)
                std::printf("invalid: %s\n", err);
            else
                std::printf("group: %s\n", gemm_group_tag(g));
        } else if (kind == "gemm") {
            const GemmForm f = gemm_select((int)mode, (int)es, descs[0], knobs, &err);
            char buf[GEMM_TAG_MAX];
            const int nsplit = descs[0].splitk > 1 ? descs[0].splitk : 1;
            if (f == GEMM_FORM_INVALID)
                std::printf("invalid: %s\n", err);
            else if (mode == 2)
                std::printf("K%d %s\n", subpixel_mean_k(descs[0]), gemm_form_tag(f, nsplit, buf));
            else
                std::printf("%s\n", gemm_form_tag(f, nsplit, buf));
        } else {
            std::fprintf(stderr, "unknown query '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
