// Which kernel form an encoder self-attention launch gets: the decision, its launch geometry, and nothing else.  Host-only, plain
// C++17, no HIP header: the launcher (attention.hip launch_attention) calls attn_select() and launch_attn_form() launches what it
// names; tests/test_attn_select_cpu.py compiles this header alone and checks, without a GPU, which form every launch reaches.
#pragma once
#include "l4p_hip.h"

// ---- the chip and the tiles (written once; the kernels read the tile constants from here) ----
constexpr int ATTN_CUS = 256;        // compute units of the MI355X: one persistent workgroup each
constexpr int ATTN_TWO_PER_CU = 512; // workgroups of a launch that puts two of them on every CU
constexpr int ATTN_DP = 96;          // head dim as stored: 88 / 64 zero-padded
constexpr int ATTN_KVB16 = 64;       // keys per KV block, 16-bit types
constexpr int ATTN_KVB32 = 32;       // ... f32: KVB * sizeof(T) == 128 either way
constexpr int ATTN_QROWS = 128;      // query rows of a 4-wave tile (32 per wave)
constexpr int ATTN_QROWS2 = 256;     // ... of a query-split (8 waves x 32) or rows64 (4 waves x 64) tile
constexpr int ATTN_KV_ROW_BYTES = 128;                                                   // KVB * sizeof(T)
constexpr int ATTN_TILE_BYTES = ATTN_DP / 16 * ATTN_KV_ROW_BYTES * 16;                   // one K tile = one V^T tile: 12 KB
constexpr int ATTN_RING_BYTES = 2 * (ATTN_TILE_BYTES + ATTN_DP * ATTN_KV_ROW_BYTES);     // K and V^T, double-buffered
constexpr int ATTN_QSTAGE_BYTES = ATTN_QROWS2 * ATTN_DP * 2;                             // the next tile's Q rows (16-bit), staged by DMA
static_assert(ATTN_TILE_BYTES == ATTN_DP * ATTN_KV_ROW_BYTES && ATTN_RING_BYTES == 49152 && ATTN_RING_BYTES + ATTN_QSTAGE_BYTES == 98304,
              "12 KB tiles; the persistent forms use 96 KB");

// The knobs the decision reads (l4p_set_knob names; the launcher snapshots them once per launch)
struct AttnKnobs {
    int attn_variant;  // tuning aid: 1 = compiler-scheduled body, 2 = no query split
    int attn_persist;  // query-split form: persistent workgroups (0: one workgroup per tile)
    int attn64;        // the one-wave-per-SIMD kernel on chip-filling launches
};

// One enumerator per kernel family (each has its dtype x head-dim instantiations; query split: head dim 88 only)
enum AttnForm {
    ATTN_FORM_INVALID = 0,
    ATTN_F32,         // attn_kernel<float, KVB 32>: 4 waves, compiler-scheduled
    ATTN_UNSPLIT,     // 4 waves x 32 query rows, hand-scheduled
    ATTN_UNSPLIT_CS,  // ... compiler-scheduled
    ATTN_KVSPLIT,     // 8 waves: two wave groups walk the even / odd KV blocks of the same 128 query rows; hand-scheduled
    ATTN_KVSPLIT_CS,  // ... compiler-scheduled
    ATTN_QSPLIT,      // 8 waves x 32 query rows share one K / V^T ring (attn_kernel<..., QS = 2>)
    ATTN_ROWS64,      // 4 waves x 64 query rows, one wave per SIMD (attention64.hip)
    ATTN_FORM_NUM
};
struct AttnChoice {
    AttnForm form;
    int ntiles;        // query tiles of the launch: (S / tile rows) * H * B
    int grid, block;   // workgroups, threads per workgroup
    int lds_bytes;     // dynamic LDS
    bool persistent;   // the grid is capped at one workgroup per CU and a workgroup walks tiles blockIdx.x, + grid, ...
    float c_scale;     // scale * log2(e); exactly 1 for pre-scaled q
};
// which form ran (include/l4p_hip.h, at l4p_prof_detail): the tests assert it.  The only place these strings are written.
inline const char* attn_form_tag(const AttnChoice& c) {
    switch (c.form) {
        case ATTN_F32: return "f32";
        case ATTN_UNSPLIT: return "unsplit";
        case ATTN_UNSPLIT_CS: return "unsplit cs";
        case ATTN_KVSPLIT: return "kvsplit";
        case ATTN_KVSPLIT_CS: return "kvsplit cs";
        case ATTN_QSPLIT: return c.persistent ? "qsplit persist" : "qsplit pertile";
        case ATTN_ROWS64: return "rows64";
        default: return "invalid";
    }
}

// ---- the decision ----
// scale = Dh^-0.5 (reference modeling_finetune.py:150), or 0 (L4P_ATTN_PRESCALED): q already carries head_dim^-0.5 * log2(e) and the
// kernels multiply by exactly 1.  form == ATTN_FORM_INVALID: a refusal (L4P_E_INVALID), *err its text - a printf format whose
// arguments are S, Dh and (double)scale.
inline AttnChoice attn_select(int dtype, int B, int S, int H, int Dh, float scale, const AttnKnobs& k, const char** err) {
    AttnChoice c = {};
    if (S % ATTN_QROWS || (Dh != 88 && Dh != 64) || !(scale >= 0.f)) {
        *err = "attention: need S %% 128 == 0, head_dim in {88, 64} and scale >= 0 (S=%d Dh=%d scale=%g)";
        return c;
    }
    c.c_scale = scale > 0.f ? scale * 1.4426950408889634f : 1.0f;
    const bool t16 = dtype == L4P_BF16 || dtype == L4P_F16;
    const long long tiles128 = (long long)(S / ATTN_QROWS) * H * B, tiles256 = (long long)(S / ATTN_QROWS2) * H * B;
    // (S % 128 == 0 from here on, so S / 64 is even: a KV split always has whole pairs of blocks; and where S % 256 == 0 is asked
    //  for below, S / 64 is a multiple of 4 - at least 4 blocks, an even number of them - which is what the persistent tile walk needs:
    //  a tile's block j and the next tile's land in ring slot j & 1 alike, and the next Q is requested four steps before the end)
    // too few workgroups for two per CU: split the KV range over two wave groups inside each workgroup
    const bool split = tiles128 < ATTN_TWO_PER_CU;
    int variant = k.attn_variant;
    // bf16 with the scale inside: the hand-scheduled bodies fold scale * log2(e) into their Q fragments, a second bf16 rounding of
    // q (2^-9 per element) that shifts the scores of a large-norm query row against large-norm keys by a few percent of a unit -
    // measured 2.7e-2 of max|out| on a row of 8x norm against keys of 6x norm.  The compiler-scheduled body applies the scale in
    // float to the accumulated scores.  (The engine passes pre-scaled q and is not affected.)
    if (dtype == L4P_BF16 && scale > 0.f) variant = 1;
    int qrows = ATTN_QROWS;
    if (!t16) {
        c.form = ATTN_F32;
    } else if (variant == 0 && k.attn64 && S % ATTN_QROWS2 == 0 && tiles256 >= ATTN_CUS) {
        // chip-filling 16-bit launches: one wave per SIMD, 64 query rows per wave (attention64.hip)
        c.form = ATTN_ROWS64, qrows = ATTN_QROWS2;
    } else if (variant == 1) {
        c.form = split ? ATTN_KVSPLIT_CS : ATTN_UNSPLIT_CS;
    } else if (Dh == 88 && !split && S % ATTN_QROWS2 == 0 && tiles256 >= ATTN_TWO_PER_CU && variant != 2) {
        // query split (8 waves share the K / V^T tiles): when the launch still fills the chip with 256-row workgroups, two per CU.
        // (head dim 88 only: there is no 64-wide instantiation)
        c.form = ATTN_QSPLIT, qrows = ATTN_QROWS2;
    } else {
        c.form = split ? ATTN_KVSPLIT : ATTN_UNSPLIT;
    }
    c.ntiles = (S / qrows) * H * B;
    // rows64: 256 persistent workgroups (one per CU) walk the tiles.  query split: persistent workgroups (one 8-wave workgroup per CU;
    // 250 registers: two waves per SIMD) that walk the tiles with the next tile's operands prefetched across the seam - measured:
    // ~3.8 us per seam at batch 4 otherwise, every workgroup of the chip fetching its prologue at the same time
    c.persistent = c.form == ATTN_ROWS64 || (c.form == ATTN_QSPLIT && k.attn_persist);
    c.grid = c.persistent && c.ntiles > ATTN_CUS ? ATTN_CUS : c.ntiles;
    const bool two_groups = c.form == ATTN_KVSPLIT || c.form == ATTN_KVSPLIT_CS || c.form == ATTN_QSPLIT;
    c.block = two_groups ? 512 : 256;
    // a ring per KV-split group; the query-split and rows64 forms stage the next tile's Q behind their one ring
    const bool kv2 = c.form == ATTN_KVSPLIT || c.form == ATTN_KVSPLIT_CS;
    c.lds_bytes = (kv2 ? 2 : 1) * ATTN_RING_BYTES + (qrows == ATTN_QROWS2 ? ATTN_QSTAGE_BYTES : 0);
    return c;
}
