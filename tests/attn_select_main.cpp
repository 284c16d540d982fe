// Driver of tests/test_attn_select_cpu.py: csrc/attn_select.hpp on the host, no GPU.  One query per input line, answer per line.
//
//   attn dtype=0 B=4 S=2048 H=16 Dh=88 scale=0 k.attn_variant=0 k.attn_persist=1 k.attn64=1
//       ->  "<tag> | ntiles=<n> grid=<g> block=<b> lds=<bytes> persistent=<0|1> c_scale=<%.9g>"
//   a refusal  ->  "invalid: <error text>"
//
// scale is a float ("nan" is accepted); k.name=value sets a field of AttnKnobs.  Fields not named are 0.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "attn_select.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        if (!(in >> kind)) continue;
        if (kind != "attn") {
            std::fprintf(stderr, "unknown query '%s'\n", kind.c_str());
            return 2;
        }
        int dtype = 0, B = 0, S = 0, H = 0, Dh = 0;
        float scale = 0.f;
        AttnKnobs knobs = {};
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "bad token '%s'\n", tok.c_str());
                return 2;
            }
            const std::string name = tok.substr(0, eq);
            const char* text = tok.c_str() + eq + 1;
            const int v = (int)std::strtol(text, nullptr, 10);
            if (name == "dtype") dtype = v;
            else if (name == "B") B = v;
            else if (name == "S") S = v;
            else if (name == "H") H = v;
            else if (name == "Dh") Dh = v;
            else if (name == "scale") scale = std::strtof(text, nullptr);
            else if (name == "k.attn_variant") knobs.attn_variant = v;
            else if (name == "k.attn_persist") knobs.attn_persist = v;
            else if (name == "k.attn64") knobs.attn64 = v;
            else {
                std::fprintf(stderr, "unknown field '%s'\n", name.c_str());
                return 2;
            }
        }
        const char* err = "";
        const AttnChoice c = attn_select(dtype, B, S, H, Dh, scale, knobs, &err);
        if (c.form == ATTN_FORM_INVALID) {
            char msg[256];
            std::snprintf(msg, sizeof msg, err, S, Dh, (double)scale);
            std::printf("invalid: %s\n", msg);
        } else {
            std::printf("%s | ntiles=%d grid=%d block=%d lds=%d persistent=%d c_scale=%.9g\n", attn_form_tag(c), c.ntiles, c.grid, c.block,
                        c.lds_bytes, (int)c.persistent, (double)c.c_scale);
        }
    }
    return 0;
}
