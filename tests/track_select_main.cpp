// Driver of tests/test_track_select_cpu.py: csrc/track_select.hpp on the host, no GPU.  One query per input line, answer per line.
//
//   ctx dtype=0 N=64 P=2048 C=1408 heads=8 tokens=6 Rg=384 shared_from=2048 k.track_deep=1
//   attn dtype=0 kind=2 N=64 P=2048 D=704 heads=8            scores N=64 P=2048 D=704 heads=8 ld=48
//   mask dtype=0 N=64 vox=802816 C=176                       readout N=64 T=16 h=56 w=56 H=224 W=224 k.readout_wide=1
//   delta dtype=0 N=64 P=2048 C=1408 K=64                    t2i_probs N=64 P=2048 HT=48 ld=48
//   i2t_probs M=131072 heads=8 tokens=6 ldp=64 ld=96 pairs=1 cbias=1 rpg=2048
//       ->  "<form> [<profiler tag>] | grid=<x>,<y>,<z> block=<b> lds=<bytes>[ <name>=<value> ...]"
//   a refusal  ->  "invalid: <error text>", formatted with the arguments the launcher passes
//
// Fields not named are 0; k.name=value sets a field of TrackKnobs.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "track_select.hpp"

static std::map<std::string, long long> g_f;
static int I(const char* name) { return (int)g_f[name]; }
static long long LL(const char* name) { return g_f[name]; }

static void geometry(const char* form, const char* tag, const TrackChoice& c) {
    std::printf("%s [%s] | grid=%d,%d,%d block=%d lds=%llu", form, tag, c.gx, c.gy, c.gz, c.block, c.lds_bytes);
}
// the refusals of l4p_small_attn / l4p_t2i_attn_scores, as launch_small_attn / launch_t2i_attn_scores format them
static void attn_refusal(const SmallAttnChoice& c, const char* err, const char* who) {
    char msg[256];
    if (c.form == TRACK_FORM_LDS_REFUSED)
        std::snprintf(msg, sizeof msg, err, who, I("P"), c.hd, c.lds_bytes, LDS_DEVICE_LIMIT);
    else
        std::snprintf(msg, sizeof msg, err, I("D"), I("heads"));
    std::printf("invalid: %s\n", msg);
}
static void attn_answer(const SmallAttnChoice& c, int kind) {
    char tag[64];
    std::snprintf(tag, sizeof tag, small_attn_form_tag(), kind, I("N"), I("P"), I("D"));
    geometry(small_attn_form_name(c.form), tag, c);
    std::printf(" hd=%d scale=%.9g stride=%lld\n", c.hd, (double)c.scale, c.stride);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, tok;
        if (!(in >> what)) continue;
        g_f.clear();
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "bad token '%s'\n", tok.c_str());
                return 2;
            }
            g_f[tok.substr(0, eq)] = std::strtoll(tok.c_str() + eq + 1, nullptr, 10);
        }
        const TrackKnobs knobs = {I("k.track_deep"), I("k.readout_wide")};
        const char* err = "";
        char msg[256], tag[64];
        if (what == "ctx") {
            const T2iContextChoice c = t2i_context_select(I("dtype"), I("N"), I("P"), I("C"), I("heads"), I("tokens"), LL("Rg"), I("shared_from"), knobs, &err);
            if (track_refused(c)) {
                std::snprintf(msg, sizeof msg, err, 0);
                std::printf("invalid: %s\n", msg);
                continue;
            }
            std::snprintf(tag, sizeof tag, t2i_context_form_tag(I("C")), I("N") * I("heads") * I("tokens"), I("C"), I("P"));
            geometry(t2i_context_form_name(c.form), tag, c);
            std::printf(" shared_from=%d\n", c.shared_from);
        } else if (what == "attn") {
            const SmallAttnChoice c = small_attn_select(I("dtype"), I("kind"), I("N"), I("P"), I("D"), I("heads"), &err);
            if (track_refused(c)) attn_refusal(c, err, "small_attn");
            else attn_answer(c, I("kind"));
        } else if (what == "scores") {
            const SmallAttnChoice c = t2i_attn_scores_select(I("N"), I("P"), I("D"), I("heads"), LL("ld"), &err);
            if (track_refused(c)) attn_refusal(c, err, "t2i_attn_scores");
            else attn_answer(c, 5);
        } else if (what == "mask") {
            const TrackChoice c = mask_product_select(I("dtype"), I("N"), LL("vox"), I("C"), &err);
            if (track_refused(c)) {
                std::snprintf(msg, sizeof msg, err, 0);
                std::printf("invalid: %s\n", msg);
                continue;
            }
            geometry(mask_product_form_name(c.form), mask_product_form_tag(), c);
            std::printf("\n");
        } else if (what == "readout") {
            const TrackChoice c = track_readout_select(I("N"), I("T"), I("h"), I("w"), I("H"), I("W"), knobs, &err);
            if (track_refused(c)) {
                if (c.form == TRACK_FORM_LDS_REFUSED)
                    std::snprintf(msg, sizeof msg, err, I("h"), I("w"), c.lds_bytes, LDS_DEVICE_LIMIT);
                else
                    std::snprintf(msg, sizeof msg, err, I("N"), I("T"), I("h"), I("w"), I("H"), I("W"));
                std::printf("invalid: %s\n", msg);
                continue;
            }
            geometry(track_readout_form_name(c.form), track_readout_form_tag(c.form), c);
            std::printf("\n");
        } else if (what == "delta" || what == "t2i_probs" || what == "i2t_probs") {
            TrackChoice c;
            if (what == "delta") {
                c = i2t_delta_select(I("dtype"), I("N"), I("P"), I("C"), I("K"), &err);
                std::snprintf(tag, sizeof tag, i2t_delta_form_tag(), LL("N") * LL("P"), I("C"), I("K"));
            } else if (what == "t2i_probs") {
                c = t2i_probs_select(I("N"), I("P"), I("HT"), LL("ld"), &err);
                std::snprintf(tag, sizeof tag, "%s", t2i_probs_form_tag());
            } else {
                c = i2t_probs_select(LL("M"), I("heads"), I("tokens"), I("ldp"), LL("ld"), I("pairs"), I("cbias") != 0, I("rpg"), &err);
                std::snprintf(tag, sizeof tag, "%s", i2t_probs_form_tag());
            }
            if (track_refused(c)) {
                std::snprintf(msg, sizeof msg, err, 0);
                std::printf("invalid: %s\n", msg);
                continue;
            }
            geometry("only", tag, c);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown query '%s'\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
