// Driver of tests/test_ln_select_cpu.py: csrc/ln_select.hpp on the host, no GPU.  One query per input line, answer per line.
//
//   ln dtype=0 kind=1 M=131072 C=1408 x=1 delta_T=1 ... k.ln_tracks=1 k.ln_rows16=1   ->  "<form>[ <slots>]"
//   a refusal                                                                         ->  "invalid: <error text>"
//
// name=value sets an integer field of LnParams (a pointer field: 0 = NULL, else a dummy address that nothing dereferences),
// k.name=value a field of LnKnobs.  Fields not named are 0.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "ln_select.hpp"

#define LN_INTS(X) X(kind) X(x_mod) X(x_is_T) X(x_period) X(x_split) X(nsplit) X(act) X(add_mod) X(M) X(C)
#define LN_PTRS(X) \
    X(x) X(x_shared) X(delta_T) X(part) X(pbias) X(dprev_T) X(stats_in) X(g0) X(b0) X(gamma) X(beta) X(add) X(out_T) X(out_T2) X(out_f32) X(out_sum) X(out_stats)
#define KNOBS(X) X(ln_tracks) X(ln_rows16)

static float g_dummy[4];

static bool set_field(LnParams& p, const std::string& name, long long v) {
#define X(f) \
    if (name == #f) { p.f = (int)v; return true; }
    LN_INTS(X)
#undef X
#define X(f) \
    if (name == #f) { p.f = v ? (decltype(p.f))g_dummy : nullptr; return true; }
    LN_PTRS(X)
#undef X
    return false;
}

static bool set_knob(LnKnobs& k, const std::string& name, long long v) {
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
        if (kind != "ln") {
            std::fprintf(stderr, "unknown query '%s'\n", kind.c_str());
            return 2;
        }
        LnParams p = {};
        LnKnobs knobs = {};
        long long dtype = 0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "bad token '%s'\n", tok.c_str());
                return 2;
            }
            const std::string name = tok.substr(0, eq);
            const long long v = std::strtoll(tok.c_str() + eq + 1, nullptr, 10);
            bool ok = true;
            if (name == "dtype")
                dtype = v;
            else if (name.rfind("k.", 0) == 0)
                ok = set_knob(knobs, name.substr(2), v);
            else
                ok = set_field(p, name, v);
            if (!ok) {
                std::fprintf(stderr, "unknown field '%s'\n", name.c_str());
                return 2;
            }
        }
        const char* err = "";
        const LnChoice c = ln_select((int)dtype, p, knobs, &err);
        if (c.form == LN_FORM_INVALID) {
            char text[256];
            std::snprintf(text, sizeof text, err, p.C);
            std::printf("invalid: %s\n", text);
        } else if (c.slots) {
            std::printf("%s %d\n", ln_form_name(c.form), c.slots);
        } else {
            std::printf("%s\n", ln_form_name(c.form));
        }
    }
    return 0;
}
