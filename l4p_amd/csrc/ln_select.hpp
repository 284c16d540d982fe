// Which kernel form a LayerNorm launch gets: its parameters, the decision, and nothing else.  Host-only, plain C++17, no HIP header:
// the launcher (elementwise.hip launch_layernorm) calls ln_select() and launches what it names; tests/test_ln_select_cpu.py compiles
// this header alone and checks, without a GPU, which form every launch of the engine reaches.
#pragma once
#include "l4p_hip.h"

// What is normalised: the rows themselves; x[row % x_mod] + an addend (l4p_layernorm_res); or the previous key LayerNorm's float result,
// re-derived from its inputs and statistics, + this layer's update (l4p_layernorm_chain)
enum LnKind { LN_ROWS = 0, LN_RES, LN_CHAIN };

// One LayerNorm launch over the last dim of [M][C].  Zero-initialised (ln_params): a field not named is absent.
struct LnParams {
    int kind;  // LnKind
    // the rows: float [M][C] - or, x_is_T, stored in the engine dtype (that form has out_T and act only; the f32 engine: float rows).
    // LN_RES / LN_CHAIN: row r is x[r % x_mod] (x_mod = 0: x[r])
    const void* x;
    int x_mod, x_is_T;
    // LN_RES: rows p = r % x_period >= x_split come from x_shared[p - x_split] instead - the part of the tracker's key stream that is
    // still common to all tracks
    const float* x_shared;
    int x_period, x_split;
    // LN_RES addend: delta_T [M][C] in the engine dtype, or pbias [C] + nsplit float partials part[nsplit][M][C] of a split-K
    // projection, summed in slice order.  LN_CHAIN: this layer's update delta_T
    const void* delta_T;
    const float *part, *pbias;
    int nsplit;
    // LN_CHAIN: the row is ln_affine(x[r % x_mod] + dprev_T[r], stats_in[r], g0, b0) + delta_T[r]
    const void* dprev_T;
    const float *stats_in, *g0, *b0;
    const float *gamma, *beta;
    float eps;
    int act;  // L4P_ACT_GELU: GELU before the addend and every store (LN_ROWS)
    // out_T2 = T(y + add[r % add_mod]): the "+ positional / + prompt token" operand of the tracker
    const float* add;
    int add_mod;
    // any of: y in the engine dtype / as float; LN_RES: the float sum itself (out_sum: the encoder's pre-norm residual stream, may alias
    // x) and (mean, rstd) per row (out_stats [M][2]: what the chained form of the next layer needs).  Outputs may alias x.
    void *out_T, *out_T2;
    float *out_f32, *out_sum, *out_stats;
    int M, C;
};
inline LnParams ln_params(LnKind kind, const void* x, const float* gamma, const float* beta, float eps, int M, int C) {
    LnParams p = {};
    p.kind = kind, p.x = x, p.gamma = gamma, p.beta = beta, p.eps = eps, p.M = M, p.C = C;
    return p;
}

// One enumerator per kernel form the launcher can start
enum LnForm {
    LN_FORM_INVALID = 0,
    // one wave per row (layernorm_kernel), 2 / 6 / 8 float4 slots per lane: 2 covers C <= 512, 6 the 1408-wide streams, 8 the 2048 limit
    LN_ROW,
    LN_ROW_T,      // rows stored in the engine dtype (16-bit)
    LN_ROW_RES,    // + delta; 2 / 6 slots
    LN_ROW_PART,   // + bias + split-K partials; 2 / 6 slots
    LN_ROW_CHAIN,  // layernorm_chain_kernel
    // one wave per token, walking the tracks (key_ln_tracks_kernel): every float row shared / the tracks' own key master / chained
    LN_TOKEN_SHARED,
    LN_TOKEN_OWN,
    LN_TOKEN_CHAIN,
    LN_ROWS16,  // 16 lanes per short row stored in the engine dtype (ln_rows16_kernel), 6 / 8 slots
    LN_FORM_NUM
};
struct LnChoice {
    LnForm form;
    int slots;  // of the forms with several instantiations, else 0
};
inline const char* ln_form_name(LnForm f) {
    static const char* const names[LN_FORM_NUM] = {"invalid", "row", "row T", "row res", "row part", "row chain", "token shared", "token own",
                                                   "token chain", "rows16"};
    return f >= 0 && f < LN_FORM_NUM ? names[f] : "invalid";
}

// The knobs the decision reads (l4p_set_knob names; the launcher snapshots them once per launch)
struct LnKnobs {
    int ln_tracks, ln_rows16;
};

// the token-ordered form applies when every float row is shared with period P = add_mod (x_mod = 0: the tracks' own float rows), both
// T outputs are wanted and the rows are whole tracks of a multiple of four tokens
inline bool ln_tokens_fit(const LnParams& p, const LnKnobs& k) {
    return k.ln_tracks && (p.x_mod == 0 || p.x_mod == p.add_mod) && p.add_mod > 0 && p.add_mod % 4 == 0 && p.M % p.add_mod == 0 && p.C % 4 == 0 &&
           p.C <= 1536 && p.add && p.out_T && p.out_T2;
}

// ---- the decision ----
// {LN_FORM_INVALID, 0}: a refusal (L4P_E_INVALID), *err its text - a printf format whose one argument is p.C.
inline LnChoice ln_select(int dtype, const LnParams& p, const LnKnobs& k, const char** err) {
    const bool t16 = dtype == L4P_BF16 || dtype == L4P_F16;
    const bool t2_bad = p.out_T2 && (!p.add || p.add_mod <= 0);
    const auto refuse = [&](const char* text) {
        *err = text;
        return LnChoice{LN_FORM_INVALID, 0};
    };
    const int slots = p.C <= 512 ? 2 : p.C <= 1536 ? 6 : 8;
    if (p.kind == LN_RES) {
        if (p.part && (p.nsplit < 1 || p.nsplit > 16)) return refuse("layernorm_res: 1 <= nsplit <= 16 slices of float partials");
        if (p.x_shared && (p.x_period <= 0 || p.x_split < 0 || p.x_split > p.x_period))
            return refuse("layernorm_res: shared rows need 0 <= x_split <= x_period, x_period > 0");
        if (p.C % 4 || p.C > 1536 || (!p.delta_T && !p.part) || t2_bad)
            return refuse("layernorm_res: C=%d must be a multiple of 4 and <= 1536, delta or partials must be given (and out_T2 needs add/add_mod)");
        if (!p.part && !p.out_sum && p.delta_T && ln_tokens_fit(p, k) &&
            (p.x_mod > 0 ? !p.x_shared : (!p.x_shared || p.x_period == p.add_mod)))
            return {p.x_mod > 0 ? LN_TOKEN_SHARED : LN_TOKEN_OWN, 0};
        // (the split-K-partials form is its own instantiation: its four-slices-at-a-time requests double the register count, which the
        //  delta form - the encoder's and the tracker's rows at 8 waves per SIMD - must not pay)
        return {p.part ? LN_ROW_PART : LN_ROW_RES, slots};
    }
    if (p.kind == LN_CHAIN) {
        if (p.C % 4 || p.C > 1536 || p.x_mod < 1 || !p.x || !p.dprev_T || !p.stats_in || !p.delta_T || t2_bad)
            return refuse("layernorm_chain: C=%d must be a multiple of 4 and <= 1536; shared rows, both updates and the statistics are required");
        return {ln_tokens_fit(p, k) ? LN_TOKEN_CHAIN : LN_ROW_CHAIN, 0};
    }
    if (p.x_is_T && t16) {
        if (p.C % 4 || p.C > 2048) return refuse("layernorm_T: C=%d must be a multiple of 4 and <= 2048");
        // short rows, many of them: one DPP row of 16 lanes per row
        if (k.ln_rows16 && p.C <= 512 && p.M >= 4096) return {LN_ROWS16, p.C <= 384 ? 6 : 8};
        return {LN_ROW_T, slots};
    }
    if (p.C % 4 || p.C > 2048 || t2_bad) return refuse("layernorm: C=%d must be a multiple of 4 and <= 2048 (and out_T2 needs add/add_mod)");
    return {LN_ROW, slots};
}
