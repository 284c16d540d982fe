// Which kernel form a GEMM / conv descriptor gets: the decision, and nothing else.  Host-only, plain C++17, no HIP header: the launcher
// (gemm_launch.hpp) calls gemm_select() and launches what it names; tests/test_gemm_select_cpu.py compiles this header alone and
// checks, without a GPU, that every case of the form tests reaches the form it is about.
//
// Kernel / tile selection (measured, tools/probes/gemm_variants.hip):
//  * the 8-phase 256x256 kernel (gemm8p.hpp) once N > 128 and the problem fills the chip with 256-wide tiles:
//    +10..35 % over the 128x128 kernel on the batch-4 encoder linears, the tracker's tall GEMMs and the DPT convs;
//  * 128x128 (4 waves, 2 workgroups per CU) below that - it quantises better on 256 CUs at batch 1;
//  * 128x64 for narrow or small problems.  (The 8-wave 256x128 form of gemm.hpp never beat both of these.)
// L4P_GEMM_VARIANT (tuning aid): 1 = never use the 8-phase kernel, 3 = always 128x64 staged tiles (dense), 10 = always 8-phase.
#pragma once
#include <cstdio>

#include "l4p_hip.h"

// One enumerator per kernel instantiation the launcher can start (per element type; the 16-bit-only ones are marked).
enum GemmForm {
    GEMM_FORM_INVALID = 0,
    // LDS-staged kernel (gemm.hpp gemm_kernel), dense
    GEMM_STAGED_128x64,
    GEMM_STAGED_128x64_DEEP,  // four stages
    GEMM_STAGED_128x128,
    // ... with row-grouped weights (l4p_gemm_desc.w_gr)
    GEMM_WGRP_64x64_DEEP,   // 16-bit
    GEMM_WGRP_128x64_DEEP,  // 16-bit
    GEMM_WGRP_128x64,
    GEMM_WGRP_128x128,
    // ... implicit-GEMM 3x3x3 conv: LDS-DMA loader, and the register loader for the fused input ReLU
    GEMM_CONV_128x64,
    GEMM_CONV_128x128,
    GEMM_CONV_RELU_128x64,
    GEMM_CONV_RELU_128x128,
    // 8-phase kernel (gemm8p.hpp), 16-bit
    GEMM_8P_256x256,
    GEMM_8P_256x192,
    GEMM_8P_SK_256x256,
    GEMM_8P_SK_256x192,
    GEMM_8P_CONV,
    // LDS-halo 3x3x3 conv (conv3_halo.hpp), 16-bit: ConvHaloCfg<2, 4>, <4, 2>; their predecessor body with two phases per k-tile
    // (conv_halo = 2); and <4, 2> with the up-sampling loader (probe builds)
    GEMM_HALO_2x4,
    GEMM_HALO_4x2,
    GEMM_HALO_2x4_2P,
    GEMM_HALO_4x2_2P,
    GEMM_HALO_4x2_UPS,
    // one-wave kernel (gemm_skinny.hpp), 16-bit: plain and with row-grouped weights
    GEMM_SKINNY,
    GEMM_SKINNY_WGRP,
    // two-workgroups-per-CU kernel (gemm4w.hpp), 16-bit, probe builds
    GEMM_4W,
    // sub-pixel conv (l4p_conv3d_subpixel): staged 128x128, and 8-phase (16-bit)
    GEMM_SUBPIX_STAGED,
    GEMM_SUBPIX_8P,
    // 8-phase kernel, dense without split-K, with its main-loop body forced (knob gemm_8p_body = 1 / 2: A/B and parity aids; the plain
    // enumerators above take the body gemm_8p_two_phase names)
    GEMM_8P_2PH_256x256,
    GEMM_8P_2PH_256x192,
    GEMM_8P_4PH_256x256,
    GEMM_8P_4PH_256x192,
    GEMM_FORM_NUM
};

// What l4p_gemm_group does with its members
enum GemmGroupForm { GEMM_GROUP_INVALID = 0, GEMM_GROUP_SKINNY, GEMM_GROUP_DEEP, GEMM_GROUP_ONE_BY_ONE };

// The knobs the decision reads (l4p_set_knob names; the launcher snapshots them once per launch)
struct GemmKnobs {
    int gemm_variant, conv_halo, gemm_skinny, skinny_max_m, gemm_deep, gemm_group, track_deep, gemm_t192, gemm_4w;
    int probe_kernels;  // the build has the measured-and-not-adopted kernels (PROBES=1)
    int gemm_8p_body;   // main-loop body of the dense 8-phase forms: 0 = gemm_8p_two_phase decides, 1 = two phases per k-tile, 2 = four
};

// ---- the forms' names: the tail of the profiler tag after "M%d N%d K%d epi%d act%d " (the tests match these byte for byte) ----
enum { GEMM_TAG_MAX = 40 };
inline const char* gemm_form_tag(GemmForm form, int nsplit, char (&buf)[GEMM_TAG_MAX]) {
    const char* head = "";  // "<head>[sk<nsplit>]<tail>"
    const char* tail = nullptr;
    switch (form) {
        case GEMM_STAGED_128x64: tail = " t128x64"; break;
        case GEMM_STAGED_128x64_DEEP: tail = " t128x64 deep"; break;
        case GEMM_STAGED_128x128: tail = " t128x128"; break;
        case GEMM_WGRP_64x64_DEEP: tail = " t64x64 deep wgrp"; break;
        case GEMM_WGRP_128x64_DEEP: tail = " t128x64 deep wgrp"; break;
        case GEMM_WGRP_128x64: tail = " t128x64 wgrp"; break;
        case GEMM_WGRP_128x128: tail = " t128x128 wgrp"; break;
        case GEMM_CONV_128x64: tail = " t128x64"; break;
        case GEMM_CONV_128x128: tail = " t128x128"; break;
        case GEMM_CONV_RELU_128x64: tail = " t128x64"; break;
        case GEMM_CONV_RELU_128x128: tail = " t128x128"; break;
        case GEMM_8P_SK_256x256: head = "8p ", tail = " t256x256"; break;
        case GEMM_8P_SK_256x192: head = "8p ", tail = " t256x192"; break;
        case GEMM_8P_256x256: return "8p t256x256";
        case GEMM_8P_256x192: return "8p t256x192";
        case GEMM_8P_CONV: return "8p t256x256";
        case GEMM_HALO_2x4: return "halo t256x256";
        case GEMM_HALO_4x2: return "halo t512x128";
        case GEMM_HALO_2x4_2P: return "halo 2p t256x256";
        case GEMM_HALO_4x2_2P: return "halo 2p t512x128";
        case GEMM_HALO_4x2_UPS: return "halo ups t512x128";
        case GEMM_SKINNY: return "skinny";
        case GEMM_SKINNY_WGRP: return "wgrp skinny";
        case GEMM_4W: return "4w t256x128";
        case GEMM_SUBPIX_STAGED: return "subpix t128x128";
        case GEMM_SUBPIX_8P: return "subpix 8p t256x256";
        case GEMM_8P_2PH_256x256: return "8p 2ph t256x256";
        case GEMM_8P_2PH_256x192: return "8p 2ph t256x192";
        case GEMM_8P_4PH_256x256: return "8p 4ph t256x256";
        case GEMM_8P_4PH_256x192: return "8p 4ph t256x192";
        default: return "invalid";
    }
    snprintf(buf, sizeof buf, "%ssk%d%s", head, nsplit, tail);
    return buf;
}
// ... of a grouped launch, after "group of %d: M%d N%d K%d ... " (the first member's shape)
inline const char* gemm_group_tag(GemmGroupForm form) { return form == GEMM_GROUP_SKINNY ? "skinny" : form == GEMM_GROUP_DEEP ? "t128x64 deep" : "one by one"; }

// ---- shared predicates ----
inline long long gemm_tiles(const l4p_gemm_desc& p, int bm, int bn) { return (long long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); }

// "big": the 128x128 tile instead of 128x64.
// 128x128 runs two workgroups per CU (512 slots on 256 CUs): a grid that spills less than a quarter of a second round
// (the batch-1 QKV projection: 576 tiles) is better served by 128x64 tiles (measured 46 -> 41 us)
// split-K problems (the low-resolution DPT convs, N >= 256): always the wider tile.  With 128x64 tiles four
// co-resident workgroups per CU pull (128 + 64) x 64 operands per k-tile each and the launch is bound by L2
// bandwidth (M = 8192, N = 256, K = 27648: 2.65 GB of tile loads in 250 us); 128x128 halves the bytes per FLOP
// (250 -> 147 us, 77 -> 59 us, 133 -> 92 us on the c3 shapes).  The split count (conv3d_splitk) assumes this.
inline bool gemm_is_big(const l4p_gemm_desc& p) {
    const long long t128 = gemm_tiles(p, 128, 128);
    return (t128 >= 400 && !(t128 > 512 && t128 < 640)) || (p.splitk > 1 && p.N >= 256);
}

// Split-K factor of a 3x3x3 conv whose output has too few tiles to occupy 256 CUs while K is long (the low-resolution DPT convs:
// M = 256..16384 voxels, K = 27*256..27*1024).  A contract between caller and launcher - the caller allocates
// partial[splitk][M][N] - so it is stated once: the DPT graph calls it, everyone else reaches it as l4p_conv3d_splitk.
inline int conv3d_splitk(long long M, int N, int K, int esize) {
    const int nk = (K + 128 / esize - 1) / (128 / esize);
    if (nk < 32) return 1;
    long long s;
    if (N >= 256) {  // 128x128 tiles, two workgroups per CU: aim at 512 workgroups (gemm_is_big picks the tile)
        const long long tiles = ((M + 127) / 128) * ((N + 127) / 128);
        if (tiles >= 400) return 1;
        s = 512 / tiles;
    } else {  // 128x64 tiles: ~1024 workgroups (4 per CU): one 4-wave workgroup per CU is latency-bound
        const long long tiles = ((M + 127) / 128) * ((N + 63) / 64);
        if (tiles >= 512) return 1;
        s = 1024 / tiles;
    }
    if (s > 16) s = 16;
    if (s > nk / 8) s = nk / 8;
    return s < 1 ? 1 : (int)s;
}

// a problem the grouped launch takes: what gemm_select would run on the four-stage 128x64 kernel
inline bool gemm_is_small_deep(const l4p_gemm_desc& p) {
    return !gemm_is_big(p) && p.splitk <= 1 && !p.relu_in && gemm_tiles(p, 128, 64) <= 256 && p.K >= 6 * 64 && !(p.tuning & 1) && p.w_gr == 0;
}

// A handful of rows (gemm_skinny.hpp: one wave per 16 x 32 output block, operands streamed into fragment registers; bit-identical to
// the LDS-staged kernels).  The wave count bounds it to problems whose weight stream is re-read by few row blocks.
inline bool gemm_is_skinny(const l4p_gemm_desc& p, const GemmKnobs& k) {
    // (tools/probes/skinny_m_sweep.py, N = 1408, K = 1408: 6.1 us against 13.9 us up to 64 rows, 9.7 against 14.2 at 96 - 128 rows - more than
    //  256 waves, two to a CU; beyond 512 blocks the staged kernel is as fast)
    return k.gemm_skinny && p.M >= 1 && p.M <= k.skinny_max_m && p.K >= 64 && p.K % 64 == 0 && p.lda % 8 == 0 && p.ldw % 8 == 0 && p.N % 8 == 0 &&
           p.w_gr == 0 && p.kw_cols == 0 && p.splitk <= 1 && !p.relu_in && p.epi == L4P_EPI_DENSE && !(p.tuning & 4) &&
           gemm_tiles(p, 16, 32) <= 512;  // (wider: every row block streams the weights again - measured
                                          //  slower than the staged kernel at N = 11264: 14.8 vs 11.5 us)
}
// row-grouped weights (l4p_gemm_desc.w_gr) on few rows: the value projection of the folded token -> image attention - 8 head groups of
// 128 context rows against their head's 88 x 1408 block of W_v: 8 workgroups of the staged kernel, each alone with its 22 k-tiles
inline bool gemm_is_skinny_grouped(const l4p_gemm_desc& p, const GemmKnobs& k) {
    // (few rows per group only: on the folded score products - 2048 rows per track against 48 folded rows - the one-wave kernel was
    //  measured at 32.7 us against the staged kernel's 12.4 us for 8 tracks, tools/probes/scores_time.py: every 16-row block streams
    //  its track's weights again)
    return k.gemm_skinny && p.w_gr > 0 && p.w_gr % 16 == 0 && p.M >= 1 && p.M <= 2048 && p.K >= 64 && p.K % 64 == 0 && p.lda % 8 == 0 &&
           p.ldw % 8 == 0 && p.N % 8 == 0 && p.a_gr == 0 && p.splitk <= 1 && !p.relu_in && p.epi == L4P_EPI_DENSE && !(p.tuning & 4) &&
           gemm_tiles(p, 16, 32) <= 512;
}

// host-side twin of gemm_epilogue_dense_cases (gemm_epilogue.hpp): the lean dense family
inline bool dense_epilogue_is_lean(const l4p_gemm_desc& p) {
    if ((p.tuning & 1) || p.epi != L4P_EPI_DENSE || p.res_mod > 0 || p.c_gr > 0 || p.a_gr > 0) return false;
    const int res = !p.res1 ? 0 : (p.res_f32 ? 1 : 2);
    if (res == 1 && p.res2) return false;
    return (res == 0) || (res == 1 && p.act == L4P_ACT_NONE) || (res == 2 && (p.act == L4P_ACT_NONE || p.act == L4P_ACT_RELU));
}
// host-side twin of gemm_epilogue_dense_dispatch (gemm_epilogue.hpp): true when the kernel will take one of the lean epilogues
inline bool epilogue_is_lean_8p(const l4p_gemm_desc& p) {
    if (p.tuning & 1) return false;
    if (p.epi == L4P_EPI_QKV) return !p.res1 && p.act == L4P_ACT_NONE && p.c_gr == 0;
    if (p.epi == L4P_EPI_CONVT) return !p.res1 && p.act == L4P_ACT_NONE && p.out_T && !p.out_f32 && !p.out_relu_T;
    return dense_epilogue_is_lean(p);
}

// Main-loop body of a dense, non-split-K 8-phase launch (gemm8p.hpp; form: GEMM_8P_256x256 or GEMM_8P_256x192): true = two phases of
// 32 / 24 MFMAs per k-tile with predicate-free steady-state staging, false = four phases of 16 / 12.  Same sums in the same order.
// Rule: the two-phase body from 8 whole k-tiles on (K >= 512); below that most k-tiles of a tile run its peeled, predicated form
// (measured on c3, same call: K = 1408 / 6144 shapes 2.0 - 10.2 % faster on it, the mask product, K = 352, 2.8 % slower).
inline bool gemm_8p_two_phase(const l4p_gemm_desc& p, GemmForm form) {
    return (form == GEMM_8P_256x256 || form == GEMM_8P_256x192) && p.K >= 8 * 64;
}

// The tile of the LDS-halo conv, host side (the launcher asserts it equal to conv3_halo.hpp's ConvHaloCfg<WR, WC>)
template <int WR, int WC>
struct ConvHaloTile {
    static constexpr int BM = WR * 128, BN = WC * 64;
    static constexpr int TT = 2, TW = 16, TH = BM / (TT * TW);
};
// LDS-halo 3x3x3 conv (conv3_halo.hpp): stride 1, 16-bit, all of N in one tile column, output volume made of whole blocks, and an
// epilogue of the lean dense family (the kernel has no generic epilogue)
template <int WR, int WC>
inline bool conv_halo_fits(const l4p_gemm_desc& p) {
    typedef ConvHaloTile<WR, WC> Cfg;
    if (p.ups_hi > 0 && !(WR == 4 && WC == 2 && p.ups_wi > 0 && (long long)p.ups_hi * p.ups_wi * p.Cin * 2 < (1ll << 31))) return false;
    return p.N == Cfg::BN && p.st == 1 && p.sh == 1 && p.sw == 1 && p.Cin % 32 == 0 && p.To % Cfg::TT == 0 && p.Ho % Cfg::TH == 0 &&
           p.Wo % Cfg::TW == 0 && p.To == p.Ti && p.Ho == p.Hi && p.Wo == p.Wi && p.M / Cfg::BM >= 192 && p.ldc == p.N &&
           (!p.res1 || p.ldr == p.N) && (long long)p.M * p.Cin * 2 < (1ll << 32) && !p.relu_in && p.splitk <= 1 && dense_epilogue_is_lean(p);
}

// Two-workgroups-per-CU form (gemm4w.hpp): 256 x 128 tiles on 4-wave workgroups, dense GEMM, 16-bit
inline bool gemm4w_fits(const l4p_gemm_desc& p) {
    if (p.relu_in || p.K % 8 || p.N <= 128) return false;
    // (one past the largest physical row the device-side map gemm_a_row, gemm_tile.hpp, can return for m < M)
    const long long pm = p.a_gr > 0 ? (long long)((p.M - 1) / p.a_gr) * p.a_gs + p.a_go + p.a_gr : p.M;
    // (LDS-DMA pieces are addressed through 32-bit buffer offsets)
    return pm * p.lda * 2 < (1ll << 31) && (long long)p.N * p.ldw * 2 < (1ll << 31);
}

// block-structured weights (l4p_gemm_desc.kw_cols): what gemm_body's per-tile k-window relies on - a tile's columns lie inside one
// column group (kw_cols a multiple of the widest tile) and the window is the tile's whole contraction (no split-K, no row groups).
// One statement for l4p_gemm and l4p_gemm_group: gemm_body honours kw_cols unconditionally.
inline bool kw_cols_ok(int mode, const l4p_gemm_desc& p, const char** err) {
    if (mode != 0 || p.w_gr > 0 || p.splitk > 1 || p.relu_in || p.kw_cols % 128 || p.kw_len < 1 || p.K % 8) {
        *err = "l4p_gemm: kw_cols needs a dense GEMM without split-K / row groups, kw_cols a multiple of 128";
        return false;
    }
    return true;
}

// Sub-pixel conv: the mean executed K of the launch (2 M N K = executed FLOPs) - it stands for K in that form's profiler tag - and the
// fewest active cells of any sub-position
inline int subpixel_mean_k(const l4p_gemm_desc& p, int* min_cells_out = nullptr) {
    int cells = 0, min_cells = 27;
    for (int s = 0; s < p.kt * p.kh * p.kw; ++s) {
        const int ks[3] = {p.kt, p.kh, p.kw}, ss[3] = {s / (p.kw * p.kh), (s / p.kw) % p.kh, s % p.kw};
        int n = 1;
        for (int a = 0; a < 3; ++a) n *= ks[a] == 1 ? 3 : (ss[a] == 0 || ss[a] == ks[a] - 1) ? 2 : 1;
        cells += n;
        min_cells = n < min_cells ? n : min_cells;
    }
    if (min_cells_out) *min_cells_out = min_cells;
    return (int)((long long)cells * p.Cin / (p.kt * p.kh * p.kw));
}

// ---- the decision ----
// mode: 0 dense GEMM, 1 conv 3x3x3, 2 sub-pixel conv (arguments checked by launch_gemm); esize: bytes per element (the 8-phase,
// LDS-halo, one-wave and 4-wave kernels and the deep ring exist for the 16-bit types only); p: the effective descriptor (the
// launcher has set the tuning bits of the epi_generic / maskdot_mfma knobs).  GEMM_FORM_INVALID: a refusal (L4P_E_INVALID), *err its text.
inline GemmForm gemm_select(int mode, int esize, const l4p_gemm_desc& p, const GemmKnobs& k, const char** err) {
    const bool t16 = esize == 2;
    const int variant = k.gemm_variant;
    if (mode == 2) {
        // Sub-pixel conv (l4p_conv3d_subpixel): the 8-phase form where 256 x 256 tiles fill the chip - the dense decoders' levels 0
        // and 1 at batch 4: 32 x 32 and 32 x 8 tiles - else 128 x 128 tiles (gemm_variant: 1 = never 8-phase, 10 = always)
        int min_cells;
        subpixel_mean_k(p, &min_cells);
        const long long t8 = (long long)((p.M + 255) / 256) * (p.N / 256);
        if (t16 && p.Cout % 256 == 0 && p.Cin % 64 == 0 && min_cells * (p.Cin / 64) >= 2 && variant != 1 && (variant == 10 || t8 >= 256))
            return GEMM_SUBPIX_8P;
        return GEMM_SUBPIX_STAGED;
    }
    if (p.kw_cols > 0) {  // block-structured weights (l4p_gemm_desc.kw_cols): the LDS-staged kernels, whose k-tile range is per tile
        if (!kw_cols_ok(mode, p, err)) return GEMM_FORM_INVALID;
        return t16 && gemm_tiles(p, 128, 64) <= 256 ? GEMM_STAGED_128x64_DEEP : GEMM_STAGED_128x64;
    }
    if (p.w_gr > 0) {  // row-grouped weights (l4p_gemm_desc.w_gr): the 128-row-tile kernels, one instantiation per tile width
        if (mode != 0 || p.splitk > 1 || p.relu_in || p.w_gr % 128 || p.K % 8) {
            *err = "l4p_gemm: row-grouped weights need a dense GEMM without split-K, w_gr a multiple of 128";
            return GEMM_FORM_INVALID;
        }
        if (t16) {
            if (gemm_is_skinny_grouped(p, k)) return GEMM_SKINNY_WGRP;
            // a grid that leaves CUs idle (the folded score products of a rank's 8-track shard: 128 tiles of K = 1408) is bound by the
            // round trips of its k-tiles: four stages (three k-tiles in flight) instead of two; the same sums in the same order
            if (k.track_deep && p.N <= 64 && (long long)((p.M + 127) / 128) <= 256 && p.K >= 6 * 64) {
                // (at most 128 tiles of 128 rows - the 8-track shard: 16384 rows - leave half the chip idle: 64-row tiles)
                return (p.M + 127) / 128 <= 128 && p.w_gr % 64 == 0 ? GEMM_WGRP_64x64_DEEP : GEMM_WGRP_128x64_DEEP;
            }
        }
        return p.N <= 64 ? GEMM_WGRP_128x64 : GEMM_WGRP_128x128;
    }
    if (t16 && mode == 0 && gemm_is_skinny(p, k)) return GEMM_SKINNY;
    const bool big = gemm_is_big(p);
    if (t16) {
        if (mode == 1 && p.ups_hi > 0) {  // up-sampling fused into the loader: the LDS-halo kernel or nothing
            if (!k.probe_kernels) {
                *err = "conv3d: the fused up-sampling loader (l4p_gemm_desc.ups_hi) is a measured-and-not-adopted form: build with PROBES=1";
                return GEMM_FORM_INVALID;
            }
            if (conv_halo_fits<4, 2>(p)) return GEMM_HALO_4x2_UPS;
            *err = "conv3d: the fused up-sampling loader takes N == 128, stride 1, Cin % 32 == 0, whole 2 x 16 x 16 output blocks";
            return GEMM_FORM_INVALID;
        }
        // L4P_CONV_HALO=0: the implicit-GEMM forms for every conv; 2: the LDS-halo kernel's predecessor body, two phases of 16 MFMAs
        // per k-tile - bit-identical to the default's one phase of 32 (A/B aids; l4p_set_knob("conv_halo", ..): the tests switch
        // forms inside one process)
        if (mode == 1 && k.conv_halo && variant != 1) {
            if (conv_halo_fits<2, 4>(p)) return k.conv_halo == 2 ? GEMM_HALO_2x4_2P : GEMM_HALO_2x4;
            if (conv_halo_fits<4, 2>(p)) return k.conv_halo == 2 ? GEMM_HALO_4x2_2P : GEMM_HALO_4x2;
        }
        if (p.splitk > 1 && mode == 0 && !p.relu_in && p.K % 8 == 0 && variant != 1 && p.N > 128) {
            // split-K on 256x256 tiles when the slices fill most of the chip exactly once (the batch-1 MLP-out projection:
            // 48 tiles x 4 slices = 192 workgroups of 24 k-tiles each, against 352 half-occupancy workgroups of 128x128 tiles:
            // 76.1 -> 72.0 us including the reduction pass; the float partials cost most of what the main loop gains)
            const long long w8 = gemm_tiles(p, 256, 256) * p.splitk;
            // (256 x 192 tiles when they fill the chip better in that one round: the same projection is 64 tiles x 4 slices = 256
            //  workgroups; L4P_GEMM_T192=0: A/B aid)
            const long long w192 = gemm_tiles(p, 256, 192) * p.splitk;
            if (k.gemm_t192 && w192 > w8 && w192 <= 256 && w8 >= 144 && p.K / p.splitk >= 512) return GEMM_8P_SK_256x192;
            if (w8 >= 144 && w8 <= 256 && p.K / p.splitk >= 512) return GEMM_8P_SK_256x256;
        }
        if (p.splitk <= 1 && !p.relu_in && p.K % 8 == 0 && variant != 1 && p.N > 128) {
            const long long t8 = gemm_tiles(p, 256, 256);
            // (t8 >= 144 with a long K: the batch-1 encoder's MLP-in and QKV projections, 192 / 144 tiles - one 256x256 tile per CU
            //  on part of the chip beats 1.1 - 1.5 rounds of 128-wide tiles: 51.7 -> 42.9 us and 43.9 -> 40.8 us; with K = 512 or
            //  fewer tiles the 128-wide kernels win)
            const bool use8 = variant == 10 || (variant == 0 && (t8 >= 256 || (t8 >= 192 && p.M >= 4096) || (t8 >= 144 && p.K >= 1024)));
            if (use8 && mode == 0) {
                // the two-workgroups-per-CU form (gemm4w.hpp).  MEASURED, NOT ADOPTED (round 4, tools/probes/ab_4w.sh + gemm4w_probe.hip):
                // its main loop moves 1.5x the 8-phase kernel's L2 -> LDS bytes and loses wherever the main loop dominates (K >= 704:
                // 1.05 - 1.17x slower on the c3 shapes); it wins where a tile's epilogue or tile quantisation dominates - mask product
                // (K = 352, VALU-heavy epilogue) 1062 -> 1017 us, the K = 256 1x1 convs 0.93 - 0.95x, QKV 1.00x - but the c3 STEP got
                // 1 % slower with exactly those shapes on it (821 vs 831 frames/s, two alternations): the tracker's GEMMs run beside
                // the dense decoders' convs on other streams, and a CU that has taken one 80 KB workgroup can host neither a second
                // kernel's 118 KB conv workgroup nor - until one arrives - a partner, so it runs half empty; the 8-phase kernel's
                // workgroups own their CU.  L4P_GEMM_4W: 0 = never (default), 1 = the shapes above, 2 = whenever it fits.
                // (l4p_set_knob("gemm_4w", ..): the tests switch forms inside one process)
                if (k.probe_kernels && k.gemm_4w) {
                    const long long t4 = gemm_tiles(p, 256, 128);
                    const bool pays = t4 >= 512 && (p.epi == L4P_EPI_MASKDOT || p.K <= 512 || (p.epi == L4P_EPI_QKV && t4 >= 1024));
                    if (gemm4w_fits(p) && (k.gemm_4w >= 2 || pays)) return GEMM_4W;
                }
                // 256 x 192 tiles (wave tile 64 x 96) where they quantise better on the 256 CUs: rounds x outputs per tile
                // (the batch-4 encoder: out projection / MLP-out 192 tiles -> 256, QKV 576 -> 768; L4P_GEMM_T192=0: A/B aid)
                const long long n192 = gemm_tiles(p, 256, 192);
                const long long c256 = (t8 + 255) / 256 * 65536, c192 = (n192 + 255) / 256 * 49152;
                const bool t192 = k.gemm_t192 && c192 < c256 && epilogue_is_lean_8p(p);
                // knob gemm_8p_body: 1 / 2 force the two-phase / four-phase main loop (bit-identical) and say so in the tag
                if (k.gemm_8p_body == 1) return t192 ? GEMM_8P_2PH_256x192 : GEMM_8P_2PH_256x256;
                if (k.gemm_8p_body == 2) return t192 ? GEMM_8P_4PH_256x192 : GEMM_8P_4PH_256x256;
                return t192 ? GEMM_8P_256x192 : GEMM_8P_256x256;
            }
            if (use8 && mode == 1 && p.Cin % 64 == 0) return GEMM_8P_CONV;
        }
    }
    if (mode == 0) {
        if (variant == 3) return GEMM_STAGED_128x64;
        // Small problems (the tracker's token-side GEMMs: M = 6 x tracks rows against 1408 x 1408 weights that come from HBM /
        // the Infinity Cache every time): at most one workgroup per CU and a k-tile is a round trip of memory latency, not
        // of bandwidth, so the two-deep ring leaves the launch latency-bound (22 k-tiles x ~1 us).  Four stages keep three
        // k-tiles in flight (96 KB of LDS: irrelevant when the grid does not fill the chip anyway).  L4P_GEMM_DEEP=0: A/B aid.
        if (t16 && !big && p.splitk <= 1 && k.gemm_deep && gemm_tiles(p, 128, 64) <= 256 && p.K >= 6 * 64) return GEMM_STAGED_128x64_DEEP;
        // (between one and two rounds of 128 x 64 tiles - the batch-1 encoder's attention projection, 352 tiles: the four-stage form on
        //  128 x 128 tiles, one workgroup per CU, was measured at +0.2 % on configs[1] (1561 -> 1564 frames/s, two alternations): not kept)
        return big ? GEMM_STAGED_128x128 : GEMM_STAGED_128x64;
    }
    if (p.relu_in) return big ? GEMM_CONV_RELU_128x128 : GEMM_CONV_RELU_128x64;
    return big ? GEMM_CONV_128x128 : GEMM_CONV_128x64;
}

// l4p_gemm_group on the 16-bit types (members already passed launch_gemm's alignment checks): all members skinny - one launch of the
// one-wave kernel; all of them small and deep - one launch of the four-stage 128x64 kernel; else one l4p_gemm each
inline GemmGroupForm gemm_group_select(const l4p_gemm_desc* p, int n, const GemmKnobs& k, const char** err) {
    for (int i = 0; i < n; ++i)  // (before anything is launched: a refused member leaves every output untouched)
        if (p[i].kw_cols > 0 && !kw_cols_ok(0, p[i], err)) return GEMM_GROUP_INVALID;
    if (!k.gemm_group || n < 2 || n > L4P_GEMM_GROUP_MAX) return GEMM_GROUP_ONE_BY_ONE;
    bool sk = true;
    long long waves = 0;
    for (int i = 0; sk && i < n; ++i) {
        sk = gemm_is_skinny(p[i], k);
        waves += gemm_tiles(p[i], 16, 32);
    }
    if (sk && waves <= 1024) return GEMM_GROUP_SKINNY;  // (more: four waves and up to a CU - the staged grouped launch below)
    bool ok = k.gemm_deep != 0;
    long long total = 0;
    for (int i = 0; ok && i < n; ++i) {
        ok = gemm_is_small_deep(p[i]);
        total += gemm_tiles(p[i], 128, 64);
    }
    // (more than two workgroups per CU's worth: nothing left to gain from sharing a launch)
    return ok && total <= 512 ? GEMM_GROUP_DEEP : GEMM_GROUP_ONE_BY_ONE;
}
