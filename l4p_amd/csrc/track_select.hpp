// Which kernel form a tracker launch gets: the decisions, their launch geometry and the constants launchers and kernels share, and
// nothing else.  Host-only, plain C++17, no HIP header: the launchers (track.hip, track_readout.hip) call a *_select() and launch what
// it names; the kernels read their tile constants and LDS layouts from here (constexpr functions); tests/test_track_select_cpu.py
// compiles this header alone and checks, without a GPU, which form every launch reaches.
#pragma once
#include <math.h>

#include "device_limits.hpp"
#include "l4p_hip.h"

// ---- the chip and the tiles (written once) ----
constexpr int TRACK_CUS = 256;           // compute units of the MI355X: "at most one workgroup per CU"
constexpr int T2I_SPLIT = 256;           // keys per softmax split of the folded token -> image attention
constexpr int T2I_MAX_SPLITS = 16;       // splits whose weights t2i_scales keeps in LDS: P <= 16 * 256
constexpr int T2I_HT = 48;               // score columns (token, head) of the folded token -> image attention
constexpr int T2I_CTX_KT = 32;           // keys per stage of the context kernel's ring
constexpr int I2T_DELTA_CW = 128;        // columns of a track one i2t_delta workgroup owns
constexpr int SMALL_ATTN_HD_MAX = 96;    // largest head dim of the token <-> image kernels = floats per staged query row
constexpr int T2I_ATTN_SCRATCH = 256;    // floats of reduction scratch behind the staged queries
constexpr int MASK_PRODUCT_VT = 128;     // voxels (= threads) of the LDS-staged mask product's tile
constexpr int READOUT_RB = 32;           // output rows whose samples the 1024-thread read-out forms at a time
constexpr int READOUT_WIDE_MAX_W = 256;  // ... its column threads: one per output column
constexpr int READOUT_WIDE_MAX_GROUPS = 512;  // (track, frame) workgroups up to which the 1024-thread form is taken
constexpr int READOUT_STATIC_LDS = 4 * 8 * 4;  // red[4][8] of both read-out kernels
// one stage of the context kernel's ring: keys [32][CW] + probs [32][48], 16-bit
constexpr int t2i_ctx_stage_bytes(int CW) { return T2I_CTX_KT * CW * 2 + T2I_CTX_KT * T2I_HT * 2; }
// t2i_attn_kernel's LDS, in floats: score rows [6][P] | the queries [6][96] | 256 of scratch; the P.V partial sums [nkg][6][hd] reuse
// the score rows, and the allocation grows by what they need beyond them (short P)
constexpr int t2i_attn_qs_off(int P) { return 6 * P; }
constexpr int t2i_attn_red_off(int P) { return 6 * P + 6 * SMALL_ATTN_HD_MAX; }
constexpr unsigned long long t2i_attn_lds_bytes(int P, int hd) {
    const unsigned long long base = ((unsigned long long)t2i_attn_red_off(P) + T2I_ATTN_SCRATCH) * 4;
    const unsigned long long scores = 6ull * P * 4, pv = hd >= 4 ? (unsigned long long)(256 / (hd / 4)) * 6 * hd * 4 : 0;
    return pv > scores ? base + (pv - scores) : base;
}
// the i2t kernels' k / v rows [2][6][D] as floats (the LDS form's q tile starts behind them, 16-byte aligned)
constexpr int i2t_attn_kv_bytes(int D) { return 12 * D * 4; }
constexpr int i2t_attn_tile_off(int D) { return (i2t_attn_kv_bytes(D) + 15) & ~15; }
// the mask product's hyper-network rows [3][Cc] as floats (the LDS form's voxel tile starts behind them, 16-byte aligned)
constexpr int mask_product_hyper_bytes(int Cc) { return 3 * Cc * 4; }
constexpr int mask_product_tile_off(int Cc) { return (mask_product_hyper_bytes(Cc) + 15) & ~15; }
// the read-out's dynamic LDS: the three source maps and the per-source-index weights [3][h w] + [w] + [h]; the 1024-thread form adds
// two interpolation tables per output row / column and RB rows of samples
constexpr unsigned long long readout_lds_bytes(int h, int w) { return (3ull * (unsigned long long)h * w + w + h) * 4; }
constexpr unsigned long long readout_wide_lds_bytes(int h, int w, int H, int W) {
    return readout_lds_bytes(h, w) + (2ull * ((unsigned long long)W + H) + (unsigned long long)READOUT_RB * W) * 4;
}

// workgroups of 256 threads for `total` work items, at most `cap` (grid-stride kernels)
inline int grid1d(long long total, long long cap) { return (int)((total + 255) / 256 < cap ? (total + 255) / 256 : cap); }
inline int track_esize(int dtype) { return dtype == L4P_F32 ? 4 : 2; }
inline bool track_is16(int dtype) { return dtype == L4P_BF16 || dtype == L4P_F16; }

// The knobs the decisions read (l4p_set_knob names; a launcher snapshots them once per launch)
struct TrackKnobs {
    int track_deep;    // context kernel: the deep rings on launches of at most one workgroup per CU
    int readout_wide;  // read-out: the 1024-thread form on launches of few (track, frame) workgroups
};

// ---- what a selection answers ----
// form: an enumerator of the family's enum below; the two refusals are shared.  A refusal is L4P_E_INVALID with *err as its text - a
// printf format whose arguments each *_select names.
constexpr int TRACK_FORM_INVALID = 0;        // the arguments are refused
constexpr int TRACK_FORM_LDS_REFUSED = -1;   // the geometry needs more LDS than a workgroup has: lds_bytes says how much
struct TrackChoice {
    int form;
    int gx, gy, gz, block;         // workgroups, threads per workgroup
    unsigned long long lds_bytes;  // dynamic LDS
};
inline bool track_refused(const TrackChoice& c) { return c.form <= 0; }
inline TrackChoice track_choice(int form, long long gx, long long gy, long long gz, int block, unsigned long long lds) {
    return TrackChoice{form, (int)gx, (int)gy, (int)gz, block, lds};
}

// ---- token -> image context (l4p_t2i_context) ----
enum T2iContextForm {
    T2I_CTX_F32 = 1,  // t2i_ctx_kernel<float>: one thread per column
    T2I_CTX_MFMA64,   // t2i_ctx_mfma_kernel, 64 columns per workgroup, ring of 4 stages
    T2I_CTX_RING4,    // ... 128 columns, ring of 4: the chip-filling form
    T2I_CTX_RING8,    // ... ring of 8, two stages per barrier
    T2I_CTX_RING12,   // ... ring of 12, four stages per barrier
};
struct T2iContextChoice : TrackChoice {
    int shared_from;  // clamped to P
};
// the MFMA forms' template arguments: stages of the ring, columns per workgroup
constexpr int t2i_ctx_ring(int form) { return form == T2I_CTX_RING12 ? 12 : form == T2I_CTX_RING8 ? 8 : 4; }
constexpr int t2i_ctx_columns(int form) { return form == T2I_CTX_MFMA64 ? 64 : 128; }
inline const char* t2i_context_form_name(int form) {
    switch (form) {
        case T2I_CTX_F32: return "ctx_f32";
        case T2I_CTX_MFMA64: return "ctx_mfma64";
        case T2I_CTX_RING4: return "ctx_ring4";
        case T2I_CTX_RING8: return "ctx_ring8";
        case T2I_CTX_RING12: return "ctx_ring12";
        default: return "invalid";
    }
}
// profiler tag (a printf format: N * heads * tokens, C, P).  Every 128-column launch carries the same tag, the f32 kernel's included:
// the tag names the column tile of the FLOP model's executed-shapes check, not the ring.
inline const char* t2i_context_form_tag(int C) {
    return C % 128 ? "M%d N%d K%d epi0 act0 ctx t48x64" : "M%d N%d K%d epi0 act0 ctx t48x128";
}
// *err takes no arguments
inline T2iContextChoice t2i_context_select(int dtype, int N, int P, int C, int heads, int tokens, long long Rg, int shared_from,
                                           const TrackKnobs& k, const char** err) {
    T2iContextChoice c = {};
    if (N < 1 || heads * tokens != T2I_HT || C % 64 || P % T2I_CTX_KT || P < 96 || P > T2I_MAX_SPLITS * T2I_SPLIT || Rg < (long long)N * tokens ||
        shared_from < 0 || shared_from % T2I_CTX_KT) {
        *err = "t2i_context: heads * tokens == 48, C %% 64 == 0, P %% 32 == 0, 96 <= P <= 4096, Rg >= N * tokens, shared_from %% 32 == 0";
        return c;
    }
    c.shared_from = shared_from > P ? P : shared_from;
    c.gy = N, c.gz = 1, c.block = 256;
    if (!track_is16(dtype)) {
        c.form = T2I_CTX_F32, c.gx = (C + 255) / 256;
        return c;
    }
    // at most one workgroup per CU (a rank's query shard): four 32-key stages per barrier on a twelve-stage ring (8 tracks: 53.8 -> 34.2 us;
    // two per barrier: 39.0), else - P not a multiple of 128 - two
    const bool deep = C % 128 == 0 && (long long)(C / 128) * N <= TRACK_CUS && k.track_deep;
    if (deep && P % 128 == 0) c.form = T2I_CTX_RING12;
    else if (deep && P % 64 == 0) c.form = T2I_CTX_RING8;
    else c.form = C % 128 == 0 ? T2I_CTX_RING4 : T2I_CTX_MFMA64;
    c.gx = C / t2i_ctx_columns(c.form);
    c.lds_bytes = (unsigned long long)t2i_ctx_ring(c.form) * t2i_ctx_stage_bytes(t2i_ctx_columns(c.form));
    return c;
}

// ---- small-token attention (l4p_small_attn kinds 0 - 4, l4p_t2i_attn_scores) ----
enum SmallAttnForm {
    SMALL_ATTN_NONE = 1,  // a kind outside 0 .. 4: nothing is launched and the call succeeds
    SMALL_ATTN_SELF6,     // self_attn6_kernel: one wave per (track, head)
    SMALL_ATTN_T2I,       // t2i_attn_kernel: one workgroup per (track, head)
    SMALL_ATTN_I2T_LDS,   // i2t_attn_lds_kernel: 256 / heads image tokens per workgroup, staged through LDS
    SMALL_ATTN_I2T,       // i2t_attn_kernel: one thread per (image token, head), straight from global memory
};
struct SmallAttnChoice : TrackChoice {
    int hd;
    float scale;       // hd^-0.5 (1 when the scores arrive formed)
    long long stride;  // elements between two tracks' image-side operand: K / V (t2i) or q (i2t); 0 = shared by every track
};
inline const char* small_attn_form_name(int form) {
    switch (form) {
        case SMALL_ATTN_NONE: return "none";
        case SMALL_ATTN_SELF6: return "self6";
        case SMALL_ATTN_T2I: return "t2i";
        case SMALL_ATTN_I2T_LDS: return "i2t_lds";
        case SMALL_ATTN_I2T: return "i2t";
        default: return "invalid";
    }
}
// profiler tag (a printf format: kind - 5 for l4p_t2i_attn_scores -, N, P, D), the same for every form
inline const char* small_attn_form_tag() { return "small_attn kind%d N%d P%d D%d"; }
// the t2i form's geometry, or the LDS refusal (shared by l4p_small_attn kinds 1 / 3 and l4p_t2i_attn_scores).  *err: "<who>", P, hd,
// lds_bytes, LDS_DEVICE_LIMIT
inline void t2i_attn_geometry(SmallAttnChoice& c, int N, int P, int heads, const char** err) {
    c.gx = N, c.gy = heads, c.gz = 1, c.block = 256;
    c.lds_bytes = t2i_attn_lds_bytes(P, c.hd);
    c.form = SMALL_ATTN_T2I;
    if (c.lds_bytes > LDS_DEVICE_LIMIT) {
        *err = "%s: P=%d keys at head dim %d need %llu bytes of LDS, the device has %zu";
        c.form = TRACK_FORM_LDS_REFUSED;
    }
}
// *err: TRACK_FORM_INVALID takes D, heads; TRACK_FORM_LDS_REFUSED (t2i, or the direct i2t form) what t2i_attn_geometry says, <who> =
// "small_attn".  heads < 1 or D < 1 is refused with the geometry text (was: a division by zero on the host)
inline SmallAttnChoice small_attn_select(int dtype, int kind, int N, int P, int D, int heads, const char** err) {
    SmallAttnChoice c = {};
    const int hd = heads > 0 ? D / heads : 0;
    if (heads < 1 || D < 1 || hd * heads != D || (kind != 0 && (hd % 4 || hd > SMALL_ATTN_HD_MAX)) ||
        ((kind == 1 || kind == 3) && P % 4)) {  // (P % 4: 16-byte LDS rows)
        *err = "small_attn: unsupported head geometry D=%d heads=%d";
        return c;
    }
    c.hd = hd, c.scale = 1.0f / sqrtf((float)hd);
    if (kind == 0) {  // 6 x 6 self attention
        c.form = SMALL_ATTN_SELF6, c.gx = N, c.gy = heads, c.gz = 1, c.block = 64;
    } else if (kind == 1 || kind == 3) {  // tokens -> image (3: one K / V set shared by every query)
        c.stride = kind == 1 ? (long long)P * D : 0;
        t2i_attn_geometry(c, N, P, heads, err);
    } else if (kind == 2 || kind == 4) {  // image -> tokens (4: one query set shared by every track)
        c.stride = kind == 2 ? (long long)P * D : 0;
        c.gy = N, c.gz = 1, c.block = 256;
        const int es = track_esize(dtype);
        const int rows = 256 % heads == 0 ? 256 / heads : 0;
        const unsigned long long lds_tile = (unsigned long long)i2t_attn_tile_off(D) + (unsigned long long)rows * D * es;
        // the LDS form: whole token rows per workgroup, in 16-byte chunks; a tile past the device's LDS takes the direct form
        if (rows && (D * es) % 16 == 0 && lds_tile <= LDS_DEVICE_LIMIT) {
            c.form = SMALL_ATTN_I2T_LDS, c.gx = (P + rows - 1) / rows, c.lds_bytes = lds_tile;
        } else {
            c.form = SMALL_ATTN_I2T, c.gx = (int)(((long long)P * heads + 255) / 256), c.lds_bytes = 12ull * D * 4;
            if (c.lds_bytes > LDS_DEVICE_LIMIT) {  // (D > 3413: even the six key and value rows do not fit)
                *err = "%s: P=%d queries at head dim %d need %llu bytes of LDS, the device has %zu";
                c.form = TRACK_FORM_LDS_REFUSED;
            }
        }
    } else {
        c.form = SMALL_ATTN_NONE;
    }
    return c;
}
// tokens -> image attention from scores formed elsewhere.  *err: TRACK_FORM_INVALID takes no arguments; TRACK_FORM_LDS_REFUSED what
// t2i_attn_geometry says, <who> = "t2i_attn_scores"
inline SmallAttnChoice t2i_attn_scores_select(int N, int P, int D, int heads, long long ld_scores, const char** err) {
    SmallAttnChoice c = {};
    const int hd = heads > 0 ? D / heads : 0;
    if (heads < 1 || hd * heads != D || hd % 4 || hd > SMALL_ATTN_HD_MAX || P % 4 || ld_scores < 6 * heads) {
        *err = "t2i_attn_scores: D = heads * hd with hd %% 4 == 0, hd <= 96, P %% 4 == 0, ld_scores >= 6 * heads";
        return c;
    }
    c.hd = hd, c.scale = 1.f, c.stride = (long long)P * D;
    t2i_attn_geometry(c, N, P, heads, err);
    return c;
}

// ---- mask product (l4p_mask_product) ----
enum MaskProductForm {
    MASK_PRODUCT_LDS = 1,  // mask_product_lds_kernel: a tile of 128 voxels x Cc channels staged through LDS
    MASK_PRODUCT_DIRECT,   // mask_product_kernel: voxel rows straight from global memory
};
inline const char* mask_product_form_name(int form) {
    return form == MASK_PRODUCT_LDS ? "lds" : form == MASK_PRODUCT_DIRECT ? "direct" : "invalid";
}
inline const char* mask_product_form_tag() { return "mask_product"; }
// *err takes no arguments
inline TrackChoice mask_product_select(int dtype, int N, long long vox, int Cc, const char** err) {
    if (Cc % 8) {
        *err = "mask_product: C %% 8 != 0";
        return TrackChoice{};
    }
    const unsigned long long lds_tile = (unsigned long long)mask_product_tile_off(Cc) + (unsigned long long)MASK_PRODUCT_VT * Cc * track_esize(dtype);
    if (lds_tile <= LDS_DEVICE_LIMIT) return track_choice(MASK_PRODUCT_LDS, (vox + MASK_PRODUCT_VT - 1) / MASK_PRODUCT_VT, N, 1, MASK_PRODUCT_VT, lds_tile);
    return track_choice(MASK_PRODUCT_DIRECT, grid1d(vox, 1024), N, 1, 256, (unsigned long long)mask_product_hyper_bytes(Cc));
}

// ---- read-out (l4p_track_readout) ----
enum ReadoutForm {
    READOUT_WIDE = 1,  // track_readout_wide_kernel: 1024 threads form the samples of 32 rows at a time
    READOUT_COLUMN,    // track_readout_kernel: 256 threads, one output column each
};
inline const char* track_readout_form_name(int form) { return form == READOUT_WIDE ? "wide" : form == READOUT_COLUMN ? "column" : "invalid"; }
inline const char* track_readout_form_tag(int form) { return form == READOUT_WIDE ? "track_readout wide" : "track_readout"; }
// the refusal of the arguments (arguments: N, T, h, w, H, W): the launcher, which sees the pointers, refuses a null one with it too
constexpr const char* READOUT_ERR_ARGS = "track_readout: needs every pointer and N, T, h, w, H, W >= 1 (N=%d T=%d h=%d w=%d H=%d W=%d)";
// *err: TRACK_FORM_INVALID is READOUT_ERR_ARGS; TRACK_FORM_LDS_REFUSED takes h, w, lds_bytes, LDS_DEVICE_LIMIT
inline TrackChoice track_readout_select(int N, int T, int h, int w, int H, int W, const TrackKnobs& k, const char** err) {
    if (N < 1 || T < 1 || h < 1 || w < 1 || H < 1 || W < 1 || (long long)N * T > 0x7FFFFFFFLL) {
        *err = READOUT_ERR_ARGS;
        return TrackChoice{};
    }
    // both kernels keep the three low-resolution maps in LDS (+ the 128 static bytes of red[][])
    const unsigned long long lds_need = readout_lds_bytes(h, w) + READOUT_STATIC_LDS;
    if (lds_need > LDS_DEVICE_LIMIT) {
        *err = "track_readout: the %d x %d source maps need %llu bytes of LDS, the device has %zu";
        return track_choice(TRACK_FORM_LDS_REFUSED, 0, 0, 0, 0, lds_need);
    }
    // the 1024-thread form: few (track, frame) workgroups - a rank's query shard of the sharded long video - leave most of the chip idle
    // and the launch is one workgroup's serial walk; with many tracks the 256-thread form fills the chip just as well.
    // (h * w < 65536: its index tables pack two source offsets into 32 bits)
    const unsigned long long lds_wide = readout_wide_lds_bytes(h, w, H, W);
    if (k.readout_wide && W <= READOUT_WIDE_MAX_W && h * w < 65536 && N * T <= READOUT_WIDE_MAX_GROUPS && lds_wide + READOUT_STATIC_LDS <= LDS_DEVICE_LIMIT)
        return track_choice(READOUT_WIDE, N * T, 1, 1, 1024, lds_wide);
    return track_choice(READOUT_COLUMN, N * T, 1, 1, 256, readout_lds_bytes(h, w));
}

// ---- one form each: checks and grid ----
constexpr int TRACK_FORM_ONLY = 1;
inline const char* i2t_delta_form_tag() { return "M%lld N%d K%d epi0 act0 delta t16x128 wgrp"; }  // (long long)N * P, C, K
inline const char* t2i_probs_form_tag() { return "t2i_probs"; }
inline const char* i2t_probs_form_tag() { return "i2t_probs"; }
// gz = the row halves of a track (each workgroup owns P / gz rows).  *err takes no arguments
inline TrackChoice i2t_delta_select(int dtype, int N, int P, int C, int K, const char** err) {
    if (!track_is16(dtype) || K != 64 || C % I2T_DELTA_CW || P % 16 || N < 1) {
        *err = "i2t_delta: 16-bit engine, k = 64, C %% 128 == 0, P %% 16 == 0 (other shapes: the row-grouped-weights GEMM)";
        return TrackChoice{};
    }
    return track_choice(TRACK_FORM_ONLY, C / I2T_DELTA_CW, N, P % 128 == 0 ? 2 : 1, 256, 0);
}
// *err takes no arguments
inline TrackChoice t2i_probs_select(int N, int P, int HT, long long ld_scores, const char** err) {
    if (N < 1 || P < 1 || P > T2I_MAX_SPLITS * T2I_SPLIT || HT != T2I_HT || ld_scores < HT || ld_scores % 4) {
        *err = "t2i_probs: HT == 48, P <= 4096, score row stride >= HT and a multiple of 4";
        return TrackChoice{};
    }
    return track_choice(TRACK_FORM_ONLY, (P + T2I_SPLIT - 1) / T2I_SPLIT, N, 1, 192, 0);
}
// *err takes no arguments
inline TrackChoice i2t_probs_select(long long M, int heads, int tokens, int ldp, long long ld_scores, int pairs, bool cbias, int rows_per_group,
                                    const char** err) {
    if (tokens < 1 || tokens > 8 || heads < 1 || ldp < tokens * heads || ld_scores < (pairs ? 2 : 1) * tokens * heads || (cbias && rows_per_group < 1)) {
        *err = "i2t_probs: 1 <= tokens <= 8, ldp >= tokens * heads, score row stride >= (pairs ? 2 : 1) * tokens * heads";
        return TrackChoice{};
    }
    return track_choice(TRACK_FORM_ONLY, grid1d(M * heads, 16384), 1, 1, 256, 0);
}
