// Driver of tests/test_gemm_tile_cpu.py: csrc/gemm_tile.hpp on the host, no GPU.  One query per input line (name=value fields, fields
// not named are 0), one answer line of integers per query:
//
//   xcd ntiles=37                          ->  xcd_tile(bid, ntiles) for bid = 0 .. ntiles - 1
//   banded ntm=3 ntn=19                    ->  "mt nt" of banded_tile for tile = 0 .. ntm * ntn - 1
//   arow a_gr=7 a_gs=100 a_go=5 n=64       ->  gemm_a_row(p, m) for m = 0 .. n - 1
//   conv B=2 Ti=2 Hi=3 Wi=5 st=1 sh=2 sw=2 Cin=64
//                                          ->  the 27 conv_tap_offset values, then per output voxel m: b ti hi wi index mask
//                                              (To, Ho, Wo = the output size of a k = 3, pad = 1 conv: (X - 1) / s + 1)
//   cells Cout=64 kt_=2 kh=2 kw=2 n0=192 n=10
//                                          ->  subpix_cells(p, n0) as "t0 h0 w0 nh nw n", then subpix_tap(cells, j) for j = 0 .. n - 1
//                                              (kt_ = the descriptor's kt)
//   splitk nk=37 nsplit=5                  ->  splitk_begin(nk, s, nsplit) for s = 0 .. nsplit
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "gemm_tile.hpp"

static std::map<std::string, std::string> g_f;
static int I(const char* name) { return g_f.count(name) ? std::atoi(g_f[name].c_str()) : 0; }

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
            g_f[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        l4p_gemm_desc p{};
        p.a_gr = I("a_gr"), p.a_gs = I("a_gs"), p.a_go = I("a_go");
        p.Ti = I("Ti"), p.Hi = I("Hi"), p.Wi = I("Wi"), p.Cin = I("Cin"), p.st = I("st"), p.sh = I("sh"), p.sw = I("sw");
        p.kt = I("kt_"), p.kh = I("kh"), p.kw = I("kw"), p.Cout = I("Cout");
        if (what == "xcd") {
            for (int bid = 0; bid < I("ntiles"); ++bid) std::printf(" %d", xcd_tile(bid, I("ntiles")));
        } else if (what == "banded") {
            for (int tile = 0; tile < I("ntm") * I("ntn"); ++tile) {
                int mt = -1, nt = -1;
                banded_tile(tile, I("ntn"), I("ntm"), mt, nt);
                std::printf(" %d %d", mt, nt);
            }
        } else if (what == "arow") {
            for (int m = 0; m < I("n"); ++m) std::printf(" %lld", gemm_a_row(p, m));
        } else if (what == "conv") {
            p.To = (p.Ti - 1) / p.st + 1, p.Ho = (p.Hi - 1) / p.sh + 1, p.Wo = (p.Wi - 1) / p.sw + 1;
            for (int tap = 0; tap < 27; ++tap) std::printf(" %lld", conv_tap_offset(p, tap));
            for (int m = 0; m < I("B") * p.To * p.Ho * p.Wo; ++m) {
                int b, ti, hi, wi;
                conv_voxel(p, m, b, ti, hi, wi);
                std::printf(" %d %d %d %d %lld %u", b, ti, hi, wi, conv_voxel_index(p, b, ti, hi, wi), conv_tap_mask(p, ti, hi, wi));
            }
        } else if (what == "cells") {
            const SubpixCells cells = subpix_cells(p, I("n0"));
            std::printf(" %d %d %d %d %d %d", cells.t0, cells.h0, cells.w0, cells.nh, cells.nw, cells.n);
            for (int j = 0; j < I("n"); ++j) std::printf(" %d", subpix_tap(cells, j));
        } else if (what == "splitk") {
            for (int s = 0; s <= I("nsplit"); ++s) std::printf(" %d", splitk_begin(I("nk"), s, I("nsplit")));
        } else {
            std::fprintf(stderr, "unknown query '%s'\n", what.c_str());
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
