/*
 * l4p_hip.h — C ABI of libl4p_hip.so: the MI355X (gfx950) engine behind the L4P inference hot path.
 *
 * This is the drop-in boundary.  The reference (NVlabs/L4P) is pure Python/PyTorch with no native
 * layer, so there is no FFI to mirror one-to-one: each entry point below replaces the ATen/cuDNN
 * work done by a specific reference function (cited per entry as file:line relative to the
 * reference tree).  The Python host (package l4p_amd, same class / argument names as the
 * reference's l4p.l4p.L4PLitModule, l4p.models.*) binds these symbols with ctypes; INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer named *dev* / every tensor argument is a DEVICE
 *    pointer owned by the caller (the Python host allocates with torch and passes data_ptr()).
 *  - every function returns 0 on success, a negative L4P_E_* code otherwise; the message is
 *    available through l4p_last_error() (thread-local).  No C++ exception crosses this boundary.
 *  - all work is enqueued asynchronously on the caller-supplied HIP stream (l4p_stream ==
 *    hipStream_t, NULL = default stream).  No hidden synchronisation, no allocation.
 *  - dtype selects the arithmetic/storage type T of activations and weights: L4P_BF16 (bf16 storage,
 *    bf16 MFMA, f32 accumulate; residual stream, LayerNorm and softmax statistics always f32) or
 *    L4P_F32 (f32 storage, exact-f32 MFMA) — the parity mode; L4P_F16: as L4P_BF16 with IEEE half in place of bf16
 *    (3 more mantissa bits, 5-bit exponent: the arithmetic class of the reference's fp16 autocast).
 */
#ifndef L4P_HIP_H
#define L4P_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4P_BF16 0
#define L4P_F32 1
#define L4P_F16 2 /* IEEE half storage + f16 MFMA, f32 accumulate: what the reference's shipped "16-mixed" (fp16 autocast) computes in */

#define L4P_OK 0
#define L4P_E_INVALID (-1) /* bad argument / unsupported shape */
#define L4P_E_HIP (-2)     /* a HIP runtime call failed */
#define L4P_E_MISSING (-3) /* a required weight was never bound */

typedef void* l4p_stream; /* hipStream_t */
typedef struct l4p_engine l4p_engine;

const char* l4p_last_error(void);
int l4p_abi_version(void); /* 26: object motion and models (l4p_objects_motion_ws_bytes, l4p_objects_motion, l4p_objects_canonical,
                              * l4p_objects_place);
                              * 25: moving objects (l4p_objects_ws_bytes, l4p_objects_label, l4p_objects_roots, l4p_objects_tables_ws_bytes,
                              * l4p_objects_tables, l4p_objects_tracks, l4p_objects_overlay);
                              * 24: results at the video's own resolution (l4p_guided_upsample);
                              * 23: the static scene map (l4p_static_map_ws_bytes, l4p_static_map_insert, l4p_static_map_count, l4p_static_map_emit);
                              * 22: dense scene flow and camera-compensated flow (l4p_scene_flow, l4p_scene_flow_summary, l4p_scene_flow_colors);
                              * 21: tracking in both time directions (l4p_time_reverse, l4p_track_bidir_queries, l4p_track_bidir_merge);
                              * 20: the split-K rule of the 3x3x3 conv, stated once for caller and launcher (l4p_conv3d_splitk);
                              * 19: 3D-track metrics, inverse-depth alignment and log-space depth errors (l4p_metric_tracks3d,
                              * l4p_metric_tracks3d_ws_bytes, l4p_metric_depth_full, l4p_metric_depth_full_ws_bytes);
                              * 18: the L4PDataset base class (l4p_gt_dense_clip, l4p_gt_query_select, l4p_gt_tracks_clip);
                              * 17: evaluation metrics (l4p_metric_ws_bytes, l4p_metric_depth, l4p_metric_flow, l4p_metric_mask,
                              * l4p_metric_tracks, l4p_metric_cameras, l4p_select_median_dev);
                              * 16: the free-viewpoint 4D renderer (l4p_view_splat, l4p_view_mesh, l4p_view_resolve);
                              * 15: l4p_conv3d_subpixel, knob dpt_fold_rn (dpt.<task>.fold{i}.w / .b);
                              * 14: DAVIS / DyCheck datasets (l4p_pil_nearest_table, l4p_torch_nearest_table, l4p_instance_mask_clip,
                              * l4p_seg_query_select); 13: the 2D result video (l4p_vis_stats, l4p_vis_panels, l4p_vis_track_prep, l4p_vis_track_raster);
                              * 12: every launcher switch is a knob; 11: 4D reconstruction (l4p_recon_cameras, l4p_point_map,
                              * l4p_track_point_map, l4p_recon_track_prep, l4p_recon_track_scale, l4p_recon_trails);
                              * 10: l4p_gemm_desc.kw_cols / kw_len, l4p_t2i_context(shared_from); 9: l4p_similarity_prefix, knobs attn64 / probe_kernels; 8: l4p_gemm_desc.ups_hi / ups_wi; 7: L4P_F16; 6: l4p_set_knob / l4p_get_knob; 5: l4p_layernorm_res(out_stats), l4p_layernorm_chain, l4p_stream_create_cu_mask; 4: l4p_gemm_desc.o_gs, l4p_i2t_delta,
                              * l4p_t2i_probs, l4p_t2i_context; 3: l4p_gemm_desc.w_gr / w_gs / b_gs, l4p_i2t_probs,
                              * l4p_t2i_attn_scores, l4p_split_hilo, l4p_transpose_pad */

/* A HIP stream restricted to CUs [first_cu, first_cu + n_cus) (hipExtStreamCreateWithCUMask) / its release.  Plumbing for the sharded
 * long-video path (l4p_amd/parallel.py): the tracker recursion's small dependent kernels on a slice of the chip of their own. */
int l4p_stream_create_cu_mask(int first_cu, int n_cus, l4p_stream* out);
int l4p_stream_destroy(l4p_stream stream);

/* Dispatch knobs of the launchers (A/B and test aids; the defaults are the shipped configuration).  A knob starts from its
 * environment variable (read ONCE, at first use) and can be changed at run time through l4p_set_knob - no getenv on a launch path.
 *   "conv_halo"  (L4P_CONV_HALO, default 1): 0 = implicit-GEMM forms for every 3x3x3 conv, 1 = the LDS-halo kernel where it fits,
 *                2 = that kernel's predecessor body (two barrier pairs per k-tile; bit-identical to 1, A/B and test aid)
 *   "gemm_4w"    (L4P_GEMM_4W,   default 0): the two-workgroups-per-CU GEMM: 0 never, 1 on the shapes it won, 2 wherever it fits
 *   "maskdot_mfma" (L4P_MASKDOT_MFMA, default 1): L4P_EPI_MASKDOT of the 16-bit engines contracts the activated row with the
 *                hyper-network vectors on the matrix pipe (the row rounded to T first, as the reference's autocast holds it);
 *                0 = the all-VALU form (float row, float dot products)
 *   "conv_ups"   (L4P_CONV_UPS, default 0): 1 = l4p_dpt_forward forms the up-sampling in front of the head conv inside that conv's
 *                loader (l4p_gemm_desc.ups_hi) where the shape allows - the same result bit for bit, 822 MB per head never written,
 *                but MEASURED SLOWER (round 5: head conv 2190 -> 3404 us against 290 us of up-sampling saved: with one pass of four
 *                taps in flight - all the registers the kernel has left - the taps' latency is not hidden); 0 = up-sample, then convolve
 *   "dpt_fold_rn" (L4P_DPT_FOLD_RN, default 1): l4p_dpt_forward runs the up-scaling ConvTranspose of a level and the 3x3x3 conv behind it
 *                (act{i}.1 -> rn{i}, dpt_block.py:255-276: no non-linearity between them) as ONE sub-pixel conv over the token grid
 *                (l4p_conv3d_subpixel with the weights dpt.<task>.fold{i}.w / .b that packing.py folds once) where those weights are
 *                bound and the shape qualifies: a fifth of the multiply-adds, the up-scaled intermediate never exists, one weight and
 *                one activation rounding fewer; 0 = ConvTranspose, then conv.  Equal to rounding, not bit for bit.  1 folds the levels
 *                whose three axes are all up-scaled (the flow / depth / mask heads: c3 70.47 -> 67.92 ms per step); 2 also the camray
 *                head's k = (2, 1, 1) levels, which keep 2/3 of the multiply-adds (measured 32 us of the step: within run-to-run noise).
 *   "ln_tracks"  (L4P_LN_TRACKS, default 1): the tracker's key LayerNorms (l4p_layernorm_res / l4p_layernorm_chain with a positional
 *                addend of period P = add_mod over whole tracks) run laid out by TOKEN: a wave owns one token and walks its tracks,
 *                the shared float rows stay in registers and the parameter vectors in LDS (bit-identical to the row kernels;
 *                473 -> 223 us and 485 -> 309 us for 64 tracks x 2048 tokens); 0 = one wave per row
 *   "ln_rows16"  (L4P_LN_ROWS16, default 1): l4p_layernorm_t on short rows (C <= 512, >= 4096 of them: the tracker's LayerNorm3d + GELU)
 *                gives a row to one DPP row of 16 lanes - four rows per wave at a time, statistics by rotations inside the DPP row,
 *                gamma / beta in registers over 16 rows per wave; 0 = one wave per row.  Equal to float rounding, not bit for bit.
 *   "attn64"     (L4P_ATTN64, default 1): l4p_attention of the 16-bit engines on chip-filling launches (>= 256 tiles of 256 query rows,
 *                S % 256 == 0): one wave per SIMD with 64 query rows (csrc/attention64.hip: every K / V^T fragment read feeds two
 *                MFMAs); 0 = the 8-wave form with 32 rows per wave.  Equal to the rounding of P, not bit for bit (the rare rescale of
 *                the deferred maximum is decided per wave).
 *   "gemm_skinny" (L4P_GEMM_SKINNY, default 1): l4p_gemm / l4p_gemm_group of the 16-bit engines on dense problems with M <= 128 rows and
 *                K % 64 == 0 (the tracker's token-side projections of a rank's query shard) run one wave per 16 x 32 output block with
 *                the operands streamed from global memory into MFMA fragment registers (csrc/gemm_skinny.hpp); bit-identical to the
 *                LDS-staged kernels (0)
 *   "readout_wide" (L4P_READOUT_WIDE, default 1): l4p_track_readout with at most 512 (track, frame) pairs runs 1024 threads per pair
 *                (the samples of 32 rows formed by all threads, then summed per column in the order of the 256-thread kernel:
 *                bit-identical; 58 -> ~20 us per launch on a rank's 8-track shard); 0 = the 256-thread kernel
 *   "track_deep" (L4P_TRACK_DEEP, default 1): row-grouped GEMMs whose grid leaves CUs idle (the folded score products of a rank's
 *                8-track shard) run four stages deep - the same sums in the same order; 0 = the two-stage form
 * The tracker window (l4p_track_window_forward / l4p_track_window_workspace_bytes; read once per window - the workspace size follows them):
 *   "track_fold_l0" (L4P_TRACK_FOLD_L0, default 1): a later window's layer 0 runs its token -> image attention in the folded form; 0 = projected form
 *   "track_fold_t2i" (L4P_TRACK_FOLD_T2I, default 1): token -> image attention with the keys' projection folded into the tokens; 0 = every key row projected
 *   "track_fold_t2i_v" (L4P_TRACK_FOLD_T2I_V, default 1): ... and the value projection too (l4p_t2i_probs / l4p_t2i_context); 0 = the projected values + l4p_t2i_attn_scores
 *   "track_kwin" (L4P_TRACK_KWIN, default 1): the folded weights' products walk only the k-tiles of a tile's head (l4p_gemm_desc.kw_cols: bit-identical); 0 = all k-tiles
 *   "track_ln_chain" (L4P_TRACK_LN_CHAIN, default 1): chained key LayerNorm in a first window (l4p_layernorm_chain); 0 keeps the float key master
 *   "track_fold_i2t" (L4P_TRACK_FOLD_I2T, default 1): image -> token attention folded into the 6 prompt tokens of each track; 0 = i2t.q / i2t.out over every image token
 *   "track_fold_pair" (L4P_TRACK_FOLD_PAIR, default 0): 1 = K' of the folded image -> token scores as a PAIR of bf16 matrices (l4p_split_hilo; measured: changes nothing)
 *   "track_delta_kernel" (L4P_TRACK_DELTA_KERNEL, default 1): delta = P x V' + b_out by its own streaming kernel (l4p_i2t_delta, bit-identical); 0 = the row-grouped GEMM
 * The GEMM launchers (A/B and tuning aids):
 *   "gemm_persist" (L4P_GEMM_PERSIST, default 1): kept so that setting it succeeds; no build launches the persistent form of the 8-phase kernel, so it selects nothing
 *   "skinny_max_m" (L4P_SKINNY_MAX_M, default 128): most rows the one-wave kernel of "gemm_skinny" takes
 *   "gemm_deep"  (L4P_GEMM_DEEP, default 1): small problems (at most one workgroup per CU, K >= 384) on the four-stage 128x64 kernel; 0 = the two-deep ring
 *   "gemm_group" (L4P_GEMM_GROUP, default 1): l4p_gemm_group runs independent projections as one launch; 0 = one launch each
 *   "epi_generic" (L4P_EPI_GENERIC, default 0): 1 = the generic epilogue instead of the lean ones (l4p_gemm_desc.tuning bit 0)
 *   "gemm_variant" (L4P_GEMM_VARIANT, default 0): 1 = never use the 8-phase kernel, 10 = always, 3 = 128x64 tiles
 *   "gemm_t192"  (L4P_GEMM_T192, default 1): 256 x 192 tiles of the 8-phase kernel where they quantise better on the 256 CUs; 0 = 256 x 256
 *   "gemm_8p_body" (L4P_GEMM_8P_BODY, default 0): main-loop body of the dense, non-split-K 8-phase kernel: 0 = the launcher's choice per shape,
 *                1 = two phases of 32 MFMAs per k-tile, 2 = four phases of 16 (bit-identical; profiler tags "8p 2ph" / "8p 4ph")
 * Attention, up-sampling, the encoder:
 *   "attn_persist" (L4P_ATTN_PERSIST, default 1): the persistent form of the 16-bit attention kernel where it applies; 0 = one workgroup per tile
 *   "attn_variant" (L4P_ATTN_VARIANT, default 0): tuning aid: 1 = compiler-scheduled body, 2 = no query split
 *   "ups_ipt"    (L4P_UPS_IPT, default 2) / "ups_nt" (L4P_UPS_NT, default 1): l4p_upsample_trilinear: items per thread / the 16-bit form with
 *                non-temporal stores (0 = plain stores)
 *   "fc2_splitk8" (L4P_FC2_SPLITK8, default -1): split-K of the encoder's MLP-out projection: -1 = chosen by tile count, 0 = the 2-slice form, n = n slices
 *   "enc_defer_res" (L4P_ENC_DEFER_RES, default 1) / "enc_sk_in_ln" (L4P_ENC_SK_IN_LN, default 1): the 16-bit encoder defers a block's residual
 *                sum to the LayerNorm that follows (0 = the fused-epilogue form) / that LayerNorm also sums the split-K partials (0 = finish pass)
 *   "probe_kernels" (read-only): 1 when the library was built with PROBES=1 and contains the measured-and-not-adopted kernels the knobs
 *                "gemm_4w" and "conv_ups" select; in the shipped build (0) those two knobs stay 0 and setting them is an error.
 * l4p_set_knob returns L4P_E_INVALID for an unknown name; l4p_get_knob returns the current value (or -1). */
int l4p_set_knob(const char* name, int value);
int l4p_get_knob(const char* name);

/* Optional per-kernel-class timing: when enabled every kernel launch is bracketed by a HIP event pair
 * recorded on the launch stream (bench.py's live roofline numbers).  Classes: gemm, conv3d, attention,
 * layernorm, elementwise, track, preprocess.  l4p_prof_read sums the pair durations of one class since the last
 * reset; the caller synchronises the stream first. */
int l4p_prof_enable(int on);
int l4p_prof_reset(void);
int l4p_prof_num_classes(void);
const char* l4p_prof_class_name(int cls);
int l4p_prof_read(int cls, double* total_ms, long long* count);
/* Per-(class, tag) breakdown (tag = GEMM shape, LayerNorm shape, kernel name ...) of the same event pairs as text
 * lines "class\ttag\tcount\ttotal_ms\n", largest first.  Returns the bytes needed incl. the terminator; writes at
 * most cap bytes to buf (buf may be NULL to query the size).  Tuning aid behind tools/prof_detail.py.
 * Tags of the attention class (l4p_attention): "B<B> S<S> H<H> Dh<Dh> <form>", at most 63 characters; <form> names the kernel
 * the launcher chose:
 *   "rows64"          the 64-row kernel (csrc/attention64.hip; knob "attn64")
 *   "qsplit persist"  the 8-wave query-split kernel, 256 persistent workgroups that walk the tiles
 *   "qsplit pertile"  the same kernel, one workgroup per tile (knob "attn_persist" = 0, or no more than 256 tiles)
 *   "kvsplit"         the 8-wave KV-split kernel (too few tiles for two workgroups per CU)
 *   "unsplit"         the 4-wave kernel, one workgroup per 128 query rows
 *   "kvsplit cs" / "unsplit cs"  the same two with the compiler-scheduled body (knob "attn_variant" = 1)
 *   "f32"             the f32 engine's kernel */
long long l4p_prof_detail(char* buf, long long cap);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entry points (also the unit-parity surface of tests/).
 * ---------------------------------------------------------------------------------------------- */

#define L4P_EPI_DENSE 0
#define L4P_EPI_QKV 1
#define L4P_EPI_CONVT 2
#define L4P_EPI_MASKDOT 3
#define L4P_ACT_NONE 0
#define L4P_ACT_GELU 1
#define L4P_ACT_RELU 2

/* out[m][n] = epilogue( sum_k A[m][k] * W[n][k] ), both operands k-contiguous.
 * Replaces F.linear / nn.Linear (modeling_finetune.py:57-68,176,188; sam/transformer.py:215-218,
 * 225-228; mask_decoder.py:160-180), nn.Conv3d 1x1x1 (dpt_block.py:447-507,218-227),
 * nn.ConvTranspose3d with kernel == stride (dpt_block.py:255-265; mask_decoder.py:58-66) and,
 * through l4p_conv3d_k3, nn.Conv3d 3x3x3 (dpt_block.py:44-79,110-129,266-276,406-414). */
typedef struct l4p_gemm_desc {
    const void* A; /* [M][lda] T (dense) or channels-last conv input [B][Ti][Hi][Wi][Cin] T */
    long long lda;
    const void* W; /* [ceil(N/128)*128][ldw] T, rows >= N are zero */
    long long ldw;
    int M, N, K;
    /* conv3d k=3 pad=1 (l4p_conv3d_k3 only): M = B*To*Ho*Wo, K = 27*Cin, k = tap*Cin + c */
    int Ti, Hi, Wi, Cin, To, Ho, Wo, st, sh, sw, relu_in;
    /* epilogue: v = acc + bias[n]; v = act(v); v += res1[m][n] (+ res2[m][n]); store */
    const float* bias;
    int act;
    const void* res1;
    const void* res2;
    int res_f32;   /* residual element type: 1 float, 0 T */
    long long ldr; /* residual row stride (elements) */
    int res_mod;   /* > 0: residual row is m % res_mod (broadcast table, e.g. the pos-embed) */
    float* out_f32; /* optional float output  [M][ldc] */
    void* out_T;    /* optional T output      [M][ldc] */
    long long ldc;
    int epi;
    /* L4P_EPI_QKV (Dp = 96): n < H*Dp -> q: out_T[m][n] (ldc = H*Dp); H*Dp <= n < 2*H*Dp -> k: kt, tiled
     * in 8-element groups [b][h][S/KVB][Dp/16][KVB][half ^ ((key>>3)&1)], KVB = 64 (bf16) / 32 (f32);
     * n >= 2*H*Dp -> v transposed: vt[b][h][d][s] */
    void* vt;
    int S, H, Dp;
    /* L4P_EPI_CONVT: n = tap*Cout + co, tap = (dt*kh + dh)*kw + dw; A rows are the (Ti,Hi,Wi) grid;
     * output is channels-last [B][Ti*kt][Hi*kh][Wi*kw][Cout] */
    int kt, kh, kw, Cout;
    /* optional row re-mapping (0 = off): logical row m lives at physical row
     * (m / gr) * gs + go + (m % gr) — used to read / write one temporal half of per-query token blocks
     * (tracker memory tokens, sparse_heads.py:406-448).  a_*: rows of A, c_*: rows of out / residual. */
    int a_gr, a_gs, a_go;
    int c_gr, c_gs, c_go;
    /* optional second T output = relu(v), same addressing as out_T: the pre-activated operand of the next
     * ResidualConvUnit conv (dpt_block.py:139-146), so that conv can stream its input without a fused ReLU */
    void* out_relu_T;
    /* L4P_EPI_QKV: K destination in the attention kernel's tile order (see l4p_attention) */
    void* k_tiled;
    /* split-K (L4P_EPI_DENSE only; for problems with too few output tiles to fill 256 CUs, e.g. the low-resolution
     * DPT convs with K = 27*1024): splitk > 1 slices contract disjoint k ranges into partial[splitk][M][N] (float,
     * caller-provided), a second kernel sums them and applies the epilogue. */
    int splitk;
    float* partial;
    /* L4P_EPI_MASKDOT (the tracker's last up-scaling ConvTranspose fused with the hyper-network mask product,
     * mask_decoder.py:136-139): the activated outputs are not stored; for every 32-column chunk c of row m
     *   out_f32[(c * 3 + i) * M + m] = sum_{n in chunk} act(acc + bias)[m][n] * hyper[((m / hyper_rows) * 3 + i) * Cout + n % Cout]
     * (i = 0..2).  Columns are tap-major with Cout (a multiple of 32, zero padded) columns per tap;
     * l4p_mask_gather sums a tap's chunks and scatters the taps to the up-scaled grid. */
    const float* hyper;
    int hyper_rows;
    /* L4P_EPI_QKV: the q columns (n < H*Dp) are multiplied by q_scale (after the bias, before rounding to T) — the
     * reference's `q = q * self.scale` (modeling_finetune.py:180) folded into the projection; the engine passes
     * head_dim^-0.5 * log2(e) so that the scores leave the attention MFMA in the exp2 domain (see l4p_attention).
     * 0 is treated as 1. */
    float q_scale;
    /* tuning aid, normally 0.  bit 0: use the generic run-time-dispatched epilogue even where a lean specialisation exists
     * (set by the launcher when L4P_EPI_GENERIC=1: in-run A/B of the two forms).  bit 1: a split-K launch leaves its float
     * partials [splitk][M][N] to the caller and runs no finish pass (bias / residual / outputs of the descriptor are ignored):
     * the encoder sums them in the LayerNorm that follows the batch-1 MLP-out projection.  bit 2: L4P_EPI_MASKDOT in its all-VALU
     * form (set by the launcher when the "maskdot_mfma" knob is 0). */
    int tuning;
    /* Row-grouped weights (0 = off; dense GEMM without split-K, w_gr a multiple of 128): rows [g * w_gr, (g + 1) * w_gr) of A
     * multiply their OWN weight matrix W + g * w_gs (elements, same ldw) and add their own bias row bias + g * b_gs (b_gs = 0: one
     * bias for all groups).  The tracker's image -> token attention with the projections folded into the token side
     * (sparse_heads.py / sam/transformer.py:180-185, see l4p_amd/models/task_heads/sparse_heads.py): every track's 2048 key rows
     * meet that track's 48 x 1408 folded key matrix, then its 1408 x 48 folded value matrix.  A group's matrix needs exactly N rows
     * (tile rows past N re-read row N - 1); the plain (w_gr = 0) path reads whole tiles: W padded to a multiple of 128 rows. */
    int w_gr;
    long long w_gs;
    int b_gs;
    /* ... and write to out_T / out_f32 + g * o_gs (elements; with the c_* row map rows of all groups can land on the same physical rows
     * in their own column blocks: the per-head value projection of the folded token -> image attention, l4p_t2i_context) */
    long long o_gs;
    /* l4p_conv3d_k3 with the bilinear up-sampling of its input fused into the loader (ups_hi > 0; 16-bit engines, stride 1, the
     * LDS-halo kernel's shapes: N == 128, Cin % 32 == 0, To % 2 == Ho % 16 == Wo % 16 == 0): A is the LOW-resolution volume
     * [B][Ti][ups_hi][ups_wi][Cin]; the conv reads F.interpolate(A, (Ti, Hi, Wi), trilinear, align_corners=True) - the time axis is
     * not resized - rounded to T exactly as l4p_upsample_trilinear would have stored it, without that tensor ever existing
     * (dpt_head.py:79-84: interpolate -> head conv).  l4p_conv3d_k3 returns L4P_E_INVALID for shapes the fused loader does not take. */
    int ups_hi, ups_wi;
    /* Block-structured weights (dense GEMM, kw_cols > 0): output columns [g * kw_cols, (g + 1) * kw_cols) only meet the kw_len elements
     * [g * kw_len, (g + 1) * kw_len) of the contraction - W is zero everywhere else (the tracker's folded projections, packing.py
     * fold_i2t / fold_t2i: head h's 1408 columns meet head h's 88 inputs) - so a tile walks only the k-tiles that cover its group's
     * window: the same sums bit for bit (the skipped tiles add zeros), 1/4 of the weight bytes.  kw_cols a multiple of 128. */
    int kw_cols, kw_len;
} l4p_gemm_desc;

int l4p_gemm(l4p_stream stream, int dtype, const l4p_gemm_desc* d);
/* n <= L4P_GEMM_GROUP_MAX INDEPENDENT dense GEMMs (no output of one is an input of another).  Equal to n l4p_gemm calls,
 * bit for bit; small bf16 problems run as ONE kernel launch (the tracker's token-side projections, sam/transformer.py:159-185:
 * q / k / v of the self-attention, k / v of the image -> token attention, the hyper-network MLP stages of the three mask
 * tokens, mask_decoder.py:130-133), anything else as separate launches. */
#define L4P_GEMM_GROUP_MAX 4
int l4p_gemm_group(l4p_stream stream, int dtype, const l4p_gemm_desc* d, int n);
int l4p_conv3d_k3(l4p_stream stream, int dtype, const l4p_gemm_desc* d);
/* The split-K factor the engine gives a 3x3x3 conv of M output voxels, N output channels and K = 27 * Cin (l4p_gemm_desc.splitk:
 * 1 = none, at most 16): the caller of l4p_conv3d_k3 allocates partial[splitk][M][N], so caller and l4p_dpt_forward read the one
 * rule.  Pure host arithmetic, no GPU needed; 0 for an unknown dtype or a size < 1. */
int l4p_conv3d_splitk(long long M, int N, int K, int dtype);
/* Sub-pixel conv: nn.ConvTranspose3d with kernel == stride == (kt, kh, kw) followed by nn.Conv3d 3x3x3, pad 1, no bias
 * (dpt_block.py:255-276: act_postprocess[i][1] -> scratch.layer_rn[i]) as one implicit GEMM over the LOW-resolution grid.
 *   A       channels-last [B][Ti][Hi][Wi][Cin] T;  M = B*Ti*Hi*Wi
 *   out_T   channels-last [B][Ti*kt][Hi*kh][Wi*kw][Cout] T (out_relu_T, optional: relu of the same values, same addressing)
 *   N       kt*kh*kw*Cout: column n = s*Cout + f, s = (s_t*kh + s_h)*kw + s_w the position of the output voxel inside its cell
 *   W       [N][ldw] T.  Along an axis of stride k the three conv taps of position k*i + s reach the cells {i-1, i} (s = 0),
 *           {i, i+1} (s = k-1), {i} (0 < s < k-1) or {i-1, i, i+1} (k = 1).  Row n holds, for the active cells of its
 *           sub-position in ascending (c_t, c_h, c_w) order, the Cin-vector  sum over the taps d that land in the cell of
 *           W_conv[f][:][d] x W_convT[:][:][sub-tap]^T;  the rest of the row (ldw >= 2^#(k>1) * 3^#(k==1) * Cin) is never read
 *           past the last active cell's k-tiles rounded up to the kernel's look-ahead, and is zero.  K is ignored.
 *   bias    float [27][Cout] or NULL: row (c_t*3 + c_h)*3 + c_w, c = 0 / 1 / 2 where the output position p has p-1 outside the
 *           up-scaled grid / both neighbours inside / p+1 outside: the sum of W_conv[f][:][d] x b_convT over the taps d inside.
 * Cells outside the grid (the batch boundaries included) contribute zero.  A column tile contracts only its sub-position's
 * cells, in that fixed order: deterministic sums.  Requires Cin % 64 (16-bit) / % 32 (f32), Cout % 128, every up-scaled axis
 * >= 2 long; no residual, activation, split-K, row map.  All three engines.  packing.py fold_convT_rn builds W and bias. */
int l4p_conv3d_subpixel(l4p_stream stream, int dtype, const l4p_gemm_desc* d);

/* Row LayerNorm of a float [M][C] stream -> T and/or float.  Replaces nn.LayerNorm
 * (modeling_finetune.py:212,235; l4p_videomae.py:115,177; sam/transformer.py:143-153) and
 * LayerNorm3d over channels-last data (mask_decoder.py:145-157). */
int l4p_layernorm(l4p_stream stream, int dtype, const float* x, const float* gamma, const float* beta, float eps,
                  void* out_T, float* out_f32, int M, int C);

/* Fused softmax(q k^T * scale) v for the encoder (modeling_finetune.py:180-186).
 * q: [B*S][H*96] T, kt: tiled K, vt: [B][H][96][S] T (all three written by L4P_EPI_QKV), out: [B*S][H*Dh] T.
 * Dh in {88, 64} (head dim < 96: the padding carries the softmax denominator (V^T) and the running maximum (Q, K)).
 * scale > 0: q is the plain projection; the f16 kernel folds scale * log2(e) into its Q fragments (a second f16
 * rounding of q), the bf16 engine runs the compiler-scheduled body ("kvsplit cs" / "unsplit cs" below), which applies
 * the scale in float to the scores - a second bf16 rounding of q would cost percents on peaked rows.  scale == 0 (L4P_ATTN_PRESCALED): q was already multiplied by head_dim^-0.5 * log2(e) when it was
 * produced (l4p_gemm_desc.q_scale) and the weights are exp2(q k^T) — the form the engine uses: one rounding of q. */
#define L4P_ATTN_PRESCALED 0.0f
int l4p_attention(l4p_stream stream, int dtype, const void* q, const void* kt, const void* vt, void* out, int B, int S,
                  int H, int Dh, float scale);

/* Tubelet gather of PatchEmbed's Conv3d(kernel=stride) (modeling_finetune.py:269-283):
 * rgb [B][Cin][T][H][W] float -> out [B*nT*nH*nW][Kp] T, zero-padded columns >= Cin*pt*ph*pw. */
int l4p_patch_gather(l4p_stream stream, int dtype, const float* rgb, void* out, int B, int Cin, int T, int H, int W,
                     int pt, int ph, int pw, int Kp);

int l4p_cast(l4p_stream stream, int dtype, const float* x, void* y, long long n);

/* Trilinear resize of channels-last data [B][Ti][Hi][Wi][C] -> [B][To][Ho][Wo][C] (C % 8 == 0).
 * Replaces F.interpolate(mode="trilinear", align_corners=True) in the DPT decoders
 * (dpt_block.py:229-234; dpt_head.py:79-83) and align_corners=False in the tracker
 * (sparse_heads.py:645-647). */
int l4p_upsample_trilinear(l4p_stream stream, int dtype, const void* x, void* y, int B, int Ti, int Hi, int Wi, int To,
                           int Ho, int Wo, int C, int align_corners);

/* DPT head2[2]: Conv3d 1x1x1 C(=128) -> Cout (<= 8) + optional exp; channels-last T in, NCDHW float out
 * (dpt_block.py:413; dense_heads.py:73,179,215 with apply_fn 'exp' misc.py:23-24).
 * w: float [Cout][C], bias: float [Cout], y: float [B][Cout][vox_per_b]. */
int l4p_head_out(l4p_stream stream, int dtype, const void* x, const float* w, const float* bias, float* y,
                 long long vox_per_b, int B, int C, int Cout, int post_exp);

/* LstSqAffineAligner (aligner.py:29-66): least-squares scale/shift between two overlapping depth
 * windows, in inverse depth (mode bit 0 set: f = safe_inverse, misc.py:48-62) or directly (bit 0 clear).
 * solve: sol[0..1] = argmin_{s,t} || s f(pred) + t - f(target) ||^2 over n floats.
 * Mode bit 1 (L4P_ALIGN_RATIO_MEAN) selects LinearAligner(method="mean") instead (aligner.py:69-118):
 * sol = (mean(f(target) / (f(pred) + 1e-8)), 0).
 * scratch: L4P_AFFINE_SCRATCH_DOUBLES doubles (per-workgroup partial sums, added in a fixed order: the
 * result is bit-reproducible).
 * apply: y = f(s f(x) + t). */
#define L4P_ALIGN_INVERSE 1
#define L4P_ALIGN_RATIO_MEAN 2
#define L4P_AFFINE_SCRATCH_DOUBLES 4096
int l4p_affine_align_solve(l4p_stream stream, const float* pred, const float* target, long long n, int mode,
                           double* scratch, float* sol);
int l4p_affine_align_apply(l4p_stream stream, const float* x, float* y, long long n, int inverse, const float* sol);

/* rays_to_cameras + pose inversion (geometry_utils.py:331-406, :249-328; dense_heads.py:346-348):
 * rays float [B][6][T][h][w] (Pluecker direction|moment), K float [B][4][4][T] pixel intrinsics of an
 * H x W image  ->  out float [B][16][T] = row-major world_T_cam per frame. */
int l4p_rays_to_pose(l4p_stream stream, const float* rays, const float* K, float* out, int B, int T, int h, int w,
                     int H, int W);

/* Intrinsics from the ray map of frame t0 (compute_optimal_rotation_intrinsics, geometry_utils.py:409-456, as
 * used by rays_to_cameras_and_fixed_per_frame_intrinsics :493-579): homography pixel -> direction by
 * normalised DLT re-estimated on its consensus set (reprojection error < reproj_thr), H^-1 = K R, RQ.
 * Deterministic replacement of cv2.findHomography(RANSAC)+cv2.RQDecomp3x3 ("parity unpinned").
 * rays float [B][6][T][h][w], out_K float [B][4][4][T] (pixel units of the H x W image, same K for all
 * frames), diag optional float [B][2] = (consensus size, iterations). */
int l4p_rays_to_intrinsics(l4p_stream stream, const float* rays, float* out_K, float* diag, int B, int T, int h, int w,
                           int H, int W, int t0, float reproj_thr);

/* The per-frame VARIABLE intrinsics branch (fixed_intrinsics = False: rays_to_cameras_and_variable_per_frame_intrinsics,
 * geometry_utils.py:582-654; reached from dense_heads.py:336-344): the same estimator run on EVERY frame's ray map:
 * out_K float [B][4][4][T] = frame t's own K; out_R float [B][9][T] = the rotation R of H^-1 = K R (row-major), which that
 * branch uses as the camera rotation as it is (no Kabsch step); diag optional float [B*T][2].  l4p_rays_to_pose_rot then
 * gives world_T_cam = [R^T | c] with the camera centre c solved from the rays (intersect_skew_lines_high_dim, :249-282). */
int l4p_rays_to_intrinsics_frames(l4p_stream stream, const float* rays, float* out_K, float* out_R, float* diag, int B, int T,
                                  int h, int w, int H, int W, float reproj_thr);
int l4p_rays_to_pose_rot(l4p_stream stream, const float* rays, const float* R, float* out, int B, int T, int h, int w);

/* ------------------------------------------------------------------------------------------------
 * Joint depth + camera seam alignment (KabaschUmeyama3DAligner, aligner.py:121-265;
 * generate_point_map, geometry_utils.py:13-53).  The reference runs numpy + skimage.measure.ransac on
 * the CPU (randomised, unpinned): these are deterministic GPU restatements of the same estimator,
 * validated against synthetic ground truth ("parity unpinned").
 * ---------------------------------------------------------------------------------------------- */

/* EXACT q-quantile of n finite floats (either sign) with torch.quantile's linear interpolation (aligner.py:187): radix
 * select of the order statistics floor(q (n-1)) and the next one on an order-preserving integer image of the float bit
 * patterns, then ATen's lerp.  ws >= L4P_QUANTILE_WS_UINTS uints. */
#define L4P_QUANTILE_WS_UINTS 2052
int l4p_quantile(l4p_stream stream, const float* x, long long n, float q, unsigned* ws, float* out);
/* EXACT order statistic `rank` (0-based, ascending) of n finite floats; torch.median(x) = rank (n - 1) / 2. */
int l4p_select_rank(l4p_stream stream, const float* x, long long n, long long rank, unsigned* ws, float* out);
/* The lower median when the number of elements that count is known only on the device.  Per clip b of B:
 * out[b * out_stride] = the order statistic (count[b * count_stride] - 1) / 2 of x[b][0..n), NaN when that count is 0.  x holds no
 * NaN and +inf (the largest key) wherever an element does not count, count <= n.  The rank is written into the workspace by a small
 * kernel from the device-side count, and the result is the selected element itself.  ws: B * L4P_QUANTILE_WS_UINTS uints. */
int l4p_select_median_dev(l4p_stream stream, const float* x, long long n, int B, const unsigned long long* count,
                          long long count_stride, unsigned* ws, float* out, long long out_stride);
/* LinearAligner(method="median").solve (aligner.py:96-107): sol[0] = torch.median over f(target) / (f(pred) + 1e-8)
 * (f = safe_inverse when `inverse`, misc.py:48-62; float arithmetic; the LOWER median as torch.median returns it),
 * sol[1] = 0, so that l4p_affine_align_apply applies it.  ratios: n floats of scratch; ws >= L4P_QUANTILE_WS_UINTS uints. */
int l4p_ratio_median_solve(l4p_stream stream, const float* pred, const float* target, long long n, int inverse,
                           float* ratios, unsigned* ws, float* sol);

/* world-space points of a hashed 1/ratio pixel subset of F frames: depth [F][H*W], K and P (world_T_cam)
 * [F][16] row-major 4x4  ->  out [F*(H*W/ratio)][3] */
int l4p_point_map_samples(l4p_stream stream, const float* depth, const float* K, const float* P, float* out, int F,
                          int H, int W, int ratio, unsigned seed);

/* RANSAC similarity dst ~ s R src + t over n correspondences (min_samples per trial, inlier threshold
 * q98[0]*thr_rel, best model re-estimated on its inliers as skimage does).  ws: float[15*trials].
 * out: float[18] = row-major 4x4 [sR|t;0 0 0 1], s, inlier count. */
int l4p_similarity_ransac(l4p_stream stream, const float* src, const float* dst, int n, const float* q98,
                          float thr_rel, int trials, int min_samples, unsigned seed, float* ws, float* out);

/* aligner.apply (aligner.py:239-265): pose [16][T] <- T pose with the 3x3 block / s ; depth[n] *= s */
int l4p_similarity_apply(l4p_stream stream, const float* sim, float* pose, int T, float* depth, long long n);

/* Prefix composition of per-seam similarities (l4p_similarity_ransac records): rel [n][B][18], seam i = window i + 1 aligned to the
 * RAW window i; out [n + 1][B][18], out[0] = identity, out[w] = out[w - 1] o rel[w - 1] = window w in window 0's frame (applying two
 * records in a row = applying the 4x4 product with the product of the scales: l4p_similarity_apply divides the rotation block by
 * the scale after each product).  The sharded long-video path's seam-local exchange (reference loop
 * dense_heads.py:444-467, which aligns every window to the accumulated buffer one after the other). */
int l4p_similarity_prefix(l4p_stream stream, const float* rel, float* out, int n, int B);

/* ------------------------------------------------------------------------------------------------
 * 4D reconstruction (generate_4D_visualization, l4p/utils/vis.py:107-221, traj3d branch): world point clouds of every pixel,
 * camera frusta and 3D track trails of one clip (B = 1), from the depth, camray (traj3d) and track_2d outputs.  Matrices are
 * float [16][T] (the b16t / b44t layout of one clip: element (i, j) of frame t at (i * 4 + j) * T + t).  All arithmetic f32,
 * f64 where the reference computes in numpy float64 (frustum vertices, trail interpolation, colour normalisation).
 * ---------------------------------------------------------------------------------------------- */

/* Cameras (vis.py:138-141; get_cam_T_ref geometry_utils.py:128-143; generate_video_camera_trajectory vis.py:621-641 with
 * create_camera_frustum vis.py:529-618), A [B][16][T]: a_is_pose = 1: A = traj3d_est_b16t and cam_T_world_t = A_t^-1;
 * a_is_pose = 0: A = cam_T_world.  cam_T_ref [B][16][T] = cam_T_world_t cam_T_world_ref^-1, world_T_cam [B][16][T] =
 * cam_T_ref^-1, frustum [B][T][8][3] = world_T_cam applied to the frustum's camera-frame vertices (height 2 near tan_half_fov at
 * z = near, 2 far tan_half_fov at z = far, aspect 1).  world_T_cam and frustum may be NULL. */
int l4p_recon_cameras(l4p_stream stream, const float* A, int B, int T, int ref, int a_is_pose, double tan_half_fov, double near_d,
                      double far_d, float* cam_T_ref, float* world_T_cam, float* frustum);
/* Dense point map (generate_point_map, geometry_utils.py:13-53; every pixel, no filtering): depth [B][T][H][W], K and P
 * (world_T_cam) [B][16][T]; component c of point (b, t, pixel q) goes to xyz[b * bs + (t * H * W + q) * ps + c * cs]
 * (ps = 3, cs = 1: [T H W][3]; ps = 1, cs = T H W, bs = 3 T H W: b3thw).  Optional colour (vis.py:143, B = 1 only; rgb_u8 NULL
 * skips it): rgb [3][T][H][W] * std[c] + mean[c] -> rgb_u8 [T H W][3] as min(255, max(0, c * 255)) truncated. */
int l4p_point_map(l4p_stream stream, const float* depth, const float* K, const float* P, int B, int T, int H, int W, float* xyz,
                  long long ps, long long cs, long long bs, const float* rgb, const float* mean, const float* stdv,
                  unsigned char* rgb_u8);
/* 3D track point map (generate_3d_track_point_map + unproject_2d_track_to_3d, geometry_utils.py:56-106): traj [B][N][2][T],
 * depth [B][N][T] (times scale[0] when scale is not NULL, vis.py:169), K, P [B][16][T] -> out [B][N][3][T]; row i holds track
 * order[b * N + i] when order is not NULL (the height sort, vis.py:722-727). */
int l4p_track_point_map(l4p_stream stream, const float* traj, const float* depth, const float* K, const float* P,
                        const float* scale, const int* order, int B, int N, int T, float* out);
/* Track preparation (vis.py:146-169, 722-727, 745): order [N] = stable argsort of the y at frame 0 (ties to the lower index);
 * per frame t and sorted track i: visible = sigmoid(vis_logit) > vis_thr; the depth map dmap [T][H][W] sampled as
 * grid_sample(mode="nearest", align_corners=False) after the reference's (W - 1), (H - 1) normalisation (0 outside the image);
 * ratios [T][N] = sample / depth for visible pairs (invisible ones hold the largest key of l4p_select_rank); flag [1] != 0 when a
 * visible ratio is NaN; slot [T][N] = rank among the frame's visible tracks or -1; counts [T] visible tracks per frame;
 * off [T + 2]: off[t] = first trail point of frame t (points per visible track: 1 at t = 0, seg * min(t, trail) after),
 * off[T] = all trail points, off[T + 1] = all visible pairs.  traj [N][2][T], vis_logit and depth [N][T]. */
int l4p_recon_track_prep(l4p_stream stream, const float* traj, const float* vis_logit, const float* depth, const float* dmap,
                         int N, int T, int H, int W, float vis_thr, int trail, int seg, int* order, int* slot, float* ratios,
                         int* flag, int* counts, long long* off);
/* scale[0] = torch.median of the nvis visible ratios (vis.py:167, the lower median: l4p_select_rank of rank (nvis - 1) / 2 over
 * the n = N T values of l4p_recon_track_prep), NaN when flag[0] != 0 or nvis = 0 (then no select is launched).
 * ws >= L4P_QUANTILE_WS_UINTS uints, sel: one float of scratch. */
int l4p_recon_track_scale(l4p_stream stream, const float* ratios, long long n, long long nvis, const int* flag, unsigned* ws,
                          float* sel, float* scale);
/* Trails (generate_3d_track_point_clouds, vis.py:738-766, tracks_leave_trace = trail, linspace(0, 1, seg)): X [N][3][T] world
 * track points in sorted order (l4p_track_point_map with order), slot / off from l4p_recon_track_prep, lut [256][3] uchar hsv
 * colours -> xyz [total][3], rgb [total][3], total = off[T].  total = 0 launches nothing. */
int l4p_recon_trails(l4p_stream stream, const float* X, const int* slot, const long long* off, const unsigned char* lut, int N,
                     int T, int trail, int seg, long long total, float* xyz, unsigned char* rgb);

/* ------------------------------------------------------------------------------------------------
 * The 2D result video (generate_video_visualizations, l4p/utils/vis.py:34-104) of one clip (batch element 0): RGB, turbo depth,
 * colour-wheel flow, thresholded motion mask and track trails over the grey video side by side, out [T][H][P W][3] float or
 * uchar (the project's own byte rule min(255, max(0, x * 255 + 0.5)) truncated).  f32 where the reference computes in torch f32,
 * f64 where it computes in Python floats / numpy float64 (the flow panel from its clip on, under NumPy 2 promotion).
 * ---------------------------------------------------------------------------------------------- */

/* Statistics (vis.py:60-63, 413-417), one launch: depth [n] (or NULL), flow [2][n] (or NULL) -> stats [3] uint: [0] = ~bits of the
 * smallest positive depth (0: none), [1] = bits of the largest, [2] = bits of max(u * u + v * v).  The consumers form
 * depth_range = (max(min, 0.05), min(max, 20)) and rad_max = min(25, sqrt(.)) from them in double. */
int l4p_vis_stats(l4p_stream stream, const float* depth, const float* flow, long long n, unsigned* stats);
/* The fused dense panels (vis.py:48-50 rgb * std + mean; :57-67 with colormap_image :227-282, turbo [256][3] float already
 * flipped; :69-77 with flow_video_to_color_with_bounds / flow_to_color_with_bounds / flow_uv_to_colors :338-428, wheel [55][3]
 * double = make_colorwheel() / 255.0; :79-87 sigmoid > 0.85; the grey background of visualize_2d_tracks :453, :464-465).
 * rgb [3][T][H][W], depth / mask [T][H][W], flow [2][T][H][W]; P panels per row, rgb in slot 0, p_* = the slot of each task or
 * -1.  out_u8 != 0 with a track panel: the grey background goes to grey [T][H][W] float for l4p_vis_track_raster instead.
 * scalars [3] double receives depth_range (NaN, NaN and an all-zero depth panel when no depth is positive) and rad_max. */
int l4p_vis_panels(l4p_stream stream, const float* rgb, const float* mean, const float* stdv, const float* depth, const float* flow,
                   const float* mask, const unsigned* stats, const float* turbo, const double* wheel, int T, int H, int W, int P,
                   int p_depth, int p_flow, int p_mask, int p_track, void* out, int out_u8, float* grey, double* scalars);
/* Display list of the track panel (visualize_2d_tracks vis.py:454-466, plot_2d_tracks :479-483, :500-502, :514-515): order [N] =
 * stable argsort of key_traj[:, 1, 0] (the batch's trajectory; ties to the lower index); per frame t and rank i: xy [T][N][2] =
 * the estimate traj [N][2][T] of track order[i] rounded half to even, vis [T][N] = sigmoid(vis_logit [N][T]) > vis_thr (and the
 * coordinates finite), colors [N][3] float = hsv [256][3] double at Normalize(0, N - 1)(i). */
int l4p_vis_track_prep(l4p_stream stream, const float* key_traj, const float* traj, const float* vis_logit, const double* hsv,
                       int N, int T, float vis_thr, int* order, int* xy, unsigned char* vis, float* colors);
/* Track raster (plot_2d_tracks vis.py:489-521; cv2.line LINE_AA / cv2.addWeighted / cv2.circle replaced by the project's own
 * rules): per frame the trail steps s of the last `trail` frames in order, each: segments in ascending rank with
 * coverage clamp(1 - distance, 0, 1), then the blend alpha F + (1 - alpha) G with the step's start G, alpha = (s + 1) / (L - 1);
 * then the discs dx^2 + dy^2 <= 5 in ascending rank.  src: background, pixel (t, y, x) at t * s_frame + y * s_row + x * s_px (may
 * alias out); out pixel (t, y, x) channel c at t * o_frame + y * o_row + x * 3 + c, float or uchar (out_u8).  N = 0 copies. */
int l4p_vis_track_raster(l4p_stream stream, const int* xy, const unsigned char* vis, const float* colors, int N, int T, int H,
                         int W, int trail, const float* src, long long s_px, long long s_row, long long s_frame, void* out,
                         long long o_row, long long o_frame, int out_u8);

/* ------------------------------------------------------------------------------------------------
 * Free-viewpoint renderer of the 4D reconstruction: what the reference shows through its viser viewer (the point cloud of frame t,
 * its track trails and the camera frustum from a camera the user moves, l4p/utils/viser.py:58-75), as depth-tested images of V
 * views.  View v shows frame frame[v] under the f32 view matrix M = cam_T_world [V][4][4] (row-major) and the pinhole
 * intr [V][4] = (fx, fy, cx, cy).  Its points are the dense cloud points[frame * HW + i], i in [0, HW), followed by the trail
 * points track_xyz[off[frame] + (i - HW)], i - HW in [0, off[frame + 1] - off[frame]); i is the point's local index.
 * zbuf [V][Ho][Wo] unsigned long long holds per pixel the smallest key (bits(z) << 32) | low: a positive f32 orders as its bit
 * pattern, so that is the nearest surface, ties to the smallest low word; low = i for a point, 0x80000000 | (frame << 4 | tri)
 * for a frustum triangle, all ones in an empty pixel.  The minimum does not depend on the order of arrival: the image is
 * reproducible bit for bit (tests/view4d_restate.py restates the rules in numpy).  A view whose frame[v] is outside [0, T) stays
 * empty; a trail block that does not lie inside track_xyz counts as empty.
 * The viewer's own rasteriser is not restated: these rules are the project's.  Every operation rounds in f32 in the order written.
 * ---------------------------------------------------------------------------------------------- */

/* Points (viser.py:58-75, add_point_cloud with point_size).  Clears zbuf to all ones on the stream, then for every point P:
 *   1. x = ((M00 X + M01 Y) + M02 Z) + M03, likewise y (row 1) and z (row 2);
 *   2. skip unless x, y, z are finite and z >= near;
 *   3. u = (fx x) / z + cx, v = (fy y) / z + cy;
 *   4. skip unless |u| < 2^20 and |v| < 2^20;
 *   5. px = floor(u + 0.5), py = floor(v + 0.5): pixel index = integer coordinate, as in generate_point_map;
 *   6. h = floor(min(((point_size fx) / z) 0.5, max_half))  (min(a, b) = a if a < b else b; skip unless h >= 0);
 *   7. the point covers the square [px - h, px + h] x [py - h, py + h], clipped to the image;
 *   8. every covered pixel takes min(zbuf, (bits(z) << 32) | i).
 * track_xyz / off may be NULL (or n_track = 0, the rows of track_xyz): dense points only.  HW + n_track < 2^31, max_half <= 64,
 * near > 0, V <= 65535. */
int l4p_view_splat(l4p_stream stream, const float* points, const float* track_xyz, const long long* off, int T, int HW,
                   long long n_track, const float* cam_T_world, const float* intr, const int* frame, int V, int Ho, int Wo,
                   float point_size, int max_half, float near_z, unsigned long long* zbuf);
/* Frustum triangles into the same buffer, after the splat (viser.py:58-75, add_mesh_trimesh of the camera mesh): frustum [T][8][3]
 * (the vertices of the recon cameras call), create_camera_frustum's 12 triangles.  View v draws the frustum of frame f = frame[v]
 * and, with stride >= 1, of every f < frame[v] with f % stride = 0 (the camera path).  Vertices k = 0, 1, 2 go through steps 1-4
 * (a skipped vertex skips the triangle).  With d(a, b, p) = (u_b - u_a) (p_y - v_a) - (v_b - v_a) (p_x - u_a): A = d(0, 1, P_2),
 * a triangle with A = 0 is skipped; over the integer pixels p of [ceil(min u), floor(max u)] x [ceil(min v), floor(max v)] clipped
 * to the image: b0 = d(1, 2, p) / A, b1 = d(2, 0, p) / A, b2 = d(0, 1, p) / A; covered when b0, b1, b2 >= 0 (two-sided, edges
 * included); z = 1 / ((b0 / z0 + b1 / z1) + b2 / z2) (perspective-correct), kept when finite and >= near; the pixel takes
 * min(zbuf, (bits(z) << 32) | 0x80000000 | (f << 4 | tri)).  T <= 65535. */
int l4p_view_mesh(l4p_stream stream, const float* frustum, int T, const float* cam_T_world, const float* intr, const int* frame,
                  int V, int Ho, int Wo, int stride, float near_z, unsigned long long* zbuf);
/* zbuf -> image [V][Ho][Wo][3] uchar, depth [V][Ho][Wo] float (the winner's camera z, +inf where empty), index [V][Ho][Wo] int
 * (the low word: the local point index, the triangle code with the high bit set, -1 where empty) (viser.py:58-75: what the viewer
 * puts on the screen).  Colours: colors [T HW][3] / track_colors [n_track][3] uchar of the winning point, the background
 * (bg_r, bg_g, bg_b) where empty, and for triangle tri the frustum colour (255, 127, 127) * shade[tri] / 32 in integers,
 * shade = {32, 31, 18, 17, 27, 26, 23, 22, 29, 28, 21, 20}.  Same T, HW, off, n_track, frame as the splat call that filled zbuf. */
int l4p_view_resolve(l4p_stream stream, const unsigned long long* zbuf, const unsigned char* colors, const unsigned char* track_colors,
                     const long long* off, int T, int HW, long long n_track, const int* frame, int V, int Ho, int Wo, int bg_r,
                     int bg_g, int bg_b, unsigned char* image, float* depth, int* index);

/* ------------------------------------------------------------------------------------------------
 * Scene flow (csrc/sceneflow.hip; the definitions are this project's own, DESIGN.md "Scene flow"): the dense heads combined across
 * time.  depth [B][1][T][H][W], flow [B][2][T][H][W] (backward: pixel p of frame t is found at p + flow in frame t - 1; channel 0 =
 * x), P = world_T_cam and K = pixel intrinsics [B][16][T] (b44t; P affine, upper-left 3x3 of K), pixel (i = column, j = row) at
 * integer coordinates.  For t >= 1, all in f32, every operation rounded on its own:
 *   X  = P_t [D_t(p) K_t^-1 (i, j, 1); 1];   q = (i + flow_x, j + flow_y);   inside = 0 <= q_x <= W - 1 and 0 <= q_y <= H - 1
 *   d' = w00 v00 + w01 v01 + w10 v10 + w11 v11 of D_{t-1} at rows y0 = floor(q_y), y1 = min(y0 + 1, H - 1) and columns x0, x1
 *        likewise (v01 = D[y0][x1]), a = q - floor(q), w00 = (1 - a_y)(1 - a_x), w01 = (1 - a_y) a_x, w10 = a_y (1 - a_x), w11 = a_y a_x
 *   X' = P_{t-1} [d' K_{t-1}^-1 (q_x, q_y, 1); 1];   scene = X' - X (world frame, pointing backward in time like the flow)
 *   u  = P_{t-1}^-1 [X; 1];  if u_z > 1e-6: rigid = (K_{t-1} u)_xy / u_z - (i, j);   comp = flow - rigid
 *   valid = inside and D_t(p) > 0 and d' > 0 and u_z > 1e-6 and every result finite; where valid is 0 the three fields are 0.
 * K^-1 (general 3x3) and P^-1 (general affine) are formed in double and rounded to f32 once.  Frame 0 has no predecessor: fields
 * and valid are 0 there, and nothing before frame 0 is read (T = 1: everything 0).  scene [B][3][T][H][W], rigid and comp
 * [B][2][T][H][W], valid [B][1][T][H][W] uchar.  `mask` (the motion-mask logits, may be NULL) is accepted for symmetry with the
 * summary and not read: the fields do not depend on it.  H W <= 2^30.
 *
 * Summary: rows [B][T][8] doubles = n_valid, n_static (valid and mask <= 0; all valid pixels when mask is NULL), n_dynamic (valid
 * and mask > 0), sum |comp| over static, over dynamic, sum |scene| over static, over dynamic, n_moving (valid and |comp| > tau_px).
 * Magnitudes are f32 (sqrtf of the unfused sum of squares, left to right, of the stored values) accumulated in double in a fixed
 * order (per-block partials in ws, then a second pass; no atomics): the same bits on every run.
 * ws: B T ceil(H W / L4P_SCENE_FLOW_CHUNK) 8 doubles.  B T < 65536.
 *
 * Colours: colors [B][T H W][3] uchar, frame-major as l4p_point_map's: a valid pixel takes lut[k] (lut [256][3] uchar) with
 * k = floor(255 min(1, |scene| / s_max[0])) in f32, an invalid one (128, 128, 128).  s_max: one float on the device.
 * Every entry returns L4P_E_INVALID, with nothing launched, for a size < 1 or a null pointer it needs.
 * ---------------------------------------------------------------------------------------------- */
#define L4P_SCENE_FLOW_CHUNK 1024
int l4p_scene_flow(l4p_stream stream, const float* depth, const float* flow, const float* P, const float* K, const float* mask, int B,
                   int T, int H, int W, float* scene, float* rigid, float* comp, unsigned char* valid);
int l4p_scene_flow_summary(l4p_stream stream, const float* scene, const float* comp, const unsigned char* valid, const float* mask,
                           int B, int T, int H, int W, float tau_px, double* ws, double* rows);
int l4p_scene_flow_colors(l4p_stream stream, const float* scene, const unsigned char* valid, const unsigned char* lut, int B, int T,
                          int H, int W, const float* s_max, unsigned char* colors);

/* ------------------------------------------------------------------------------------------------
 * Static scene map (csrc/static_map.hip; this project's own, the reference writes one PLY per frame; DESIGN.md "Static scene map"):
 * the clip's world points fused into one voxel map.  points [M][3] float and colors [M][3] uchar are frame-major as l4p_point_map
 * writes them, M = T HW, point m belongs to frame m / HW; grid [4] float on the device = (ox, oy, oz, v): origin and voxel size.
 * Point rule, all f32, every operation rounded on its own.  Point m = (x, y, z) is dropped
 *   as non-finite  if a coordinate is NaN or +-Inf;
 *   as masked      else if mask_logit != NULL and mask_logit[m] > 0 (a NaN logit is not > 0), or keep != NULL and keep[m] == 0;
 *   as out of range else if not (v > 0 and v finite), or if for an axis i = floorf(q), q = (p - o) / v, is not in [-2^20, 2^20 - 1]
 *                  (a NaN i is not).
 * Otherwise per axis f = (int)floorf((q - i) * 65536.0f), in [0, 65535], and the voxel key is
 *   (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42     (63 bits; all ones marks an empty slot).
 * Per voxel, integers only, so that no result depends on the order of arrival: count, the three sums of f, the three colour sums,
 * first_point (the smallest m; first_frame = first_point / HW), last_frame, and n_frames, the number of distinct frames with a point
 * in the voxel.  Table: open addressing on the key with atomicCAS, linear probing from a mix of the key, `capacity` slots of 64
 * bytes, capacity a power of two <= 2^30; the probe loop ends after `capacity` steps, and a point that found no slot counts in
 * n_overflow and is in no voxel.  T HW <= 2^24 (the colour sums are 32-bit).
 * Order: voxels leave by first appearance, ascending first_point, among those kept: n_frames >= min_frames and count >= min_points.
 * Emitted per kept voxel: xyz [V][3] float, in f64, every operation rounded on its own:
 *   fx = ((double)sum_fx + 0.5 * (double)count) / ((double)count * 65536.0);   x = (float)((double)ox + ((double)ix + fx) * (double)v)
 * rgb [V][3] uchar = (2 sum_c + count) / (2 count) in integers (half rounds up); count, n_frames, first_frame, last_frame,
 * first_point [V] int; key [V] long long.  voxel_id [M] int: the output row of the point's voxel, -1 for a dropped point, a point
 * without a slot or a filtered voxel.
 * The three calls share ws (l4p_static_map_ws_bytes(capacity, M) bytes; 0 for sizes the entries refuse) and run in this order:
 *   insert  clears ws, inserts all points in one launch and then marks the frames, one small launch per frame in stream order
 *           (that is what counts n_frames);
 *   count   marks the kept voxels and fills counters [8] unsigned long long on the device = n_points, n_used (points with a key),
 *           n_nonfinite, n_masked, n_out_of_range, n_voxels, n_kept, n_overflow (n_points = n_used + the three drop counts);
 *   emit    writes the n_kept rows (n_kept as counted: the caller reads counters back to size them) and voxel_id.
 * Every entry returns L4P_E_INVALID, with nothing launched, for a size it refuses or a null pointer it needs.
 * ---------------------------------------------------------------------------------------------- */
size_t l4p_static_map_ws_bytes(long long capacity, long long M);
int l4p_static_map_insert(l4p_stream stream, const float* points, const unsigned char* colors, const float* mask_logit,
                          const unsigned char* keep, const float* grid, int T, int HW, long long capacity, void* ws);
int l4p_static_map_count(l4p_stream stream, void* ws, int T, int HW, long long capacity, int min_frames, int min_points,
                         unsigned long long* counters);
int l4p_static_map_emit(l4p_stream stream, void* ws, const float* grid, int T, int HW, long long capacity, long long n_kept, float* xyz,
                        unsigned char* rgb, int* count, int* n_frames, int* first_frame, int* last_frame, int* first_point,
                        long long* key, int* voxel_id);

/* ------------------------------------------------------------------------------------------------
 * Moving objects (csrc/objects.hip; this project's own, the reference thresholds the motion mask for a picture and stops; DESIGN.md
 * "Moving objects"): connected-component labelling of the motion mask over (t, y, x), the frames linked through the backward flow, and
 * the per-object tables that follow from the labels.  One clip (batch size 1).  All arithmetic is f32 and every operation is rounded
 * on its own.  Inputs, with linear index m = (t H + y) W + x, T H W <= 2^30:
 *   mask_logit [T][H][W] float;  depth [T][H][W] float or NULL;  flow [2][T][H][W] float or NULL: backward flow, channel 0 = x (pixel p
 *   of frame t is found at p + flow in frame t - 1, as l4p_scene_flow reads it);  keep [T][H][W] uchar or NULL.
 * Foreground: m is foreground iff mask_logit[m] > 0 (a NaN is not > 0), and keep is NULL or keep[m] != 0, and depth is NULL or
 *   depth[m] is finite and > 0.
 * Spatial edges: a foreground pixel (t, y, x) has an edge to (t, y, x-1) and (t, y-1, x); with connectivity == 8 also to (t, y-1, x-1)
 *   and (t, y-1, x+1).  An edge exists where the neighbour is inside the frame and foreground and the depth gate passes.  The gate
 *   passes when depth is NULL, or max_depth_ratio <= 0, or fmaxf(da, db) <= max_depth_ratio * fminf(da, db).
 * Temporal edge, for t >= 1: one edge to (t-1, yq, xq) if that pixel is foreground.  Without flow (yq, xq) = (y, x).  With flow:
 *   u = flow[0][m], v = flow[1][m]; no edge if either is not finite; gx = floorf(((float)x + u) + 0.5f), gy = floorf(((float)y + v) +
 *   0.5f); no edge unless gx >= 0 && gx < (float)W && gy >= 0 && gy < (float)H, compared in float, before the conversion to int;
 *   (xq, yq) = ((int)gx, (int)gy).  Temporal edges carry no depth gate: camera and object both move between frames.
 * Component: a connected set under these edges; its label is the smallest m among its members, so no output depends on the order in
 *   which edges are processed.  label [M] int = that value, -1 for background.  Per component: n_pixels, first_frame = label / (H W),
 *   last_frame.  Edges change t by at most one, so a component's frames are contiguous: n_frames = last_frame - first_frame + 1.
 * Filter and order: a component is kept iff n_pixels >= min_pixels and n_frames >= min_frames; kept components are numbered 0..K-1 by
 *   ascending label, the order of first appearance.  object_id [M] int = that number, or -1.
 * counters [6] unsigned long long on the device = n_pixels (T H W), n_foreground, n_components, n_kept, n_kept_pixels, n_guard.
 *   Every find and union loop of the labelling is finite (parent[i] <= i from the first write on, only smaller values are written);
 *   each still carries a cap on its steps (T H W on the global array), and a loop that hits it gives up and counts in n_guard
 *   instead of spinning: n_guard != 0 means the labels are not to be used.
 * Calls: l4p_objects_label (ws of l4p_objects_ws_bytes(T, H, W) bytes, 0 for sizes the entries refuse; every byte of ws that is read
 *   is written by the call first) writes label, object_id and counters; the caller reads counters back to size the tables;
 *   l4p_objects_roots (same ws, label and object_id, n_kept as counted) writes root, n_pixels, first_frame, last_frame [K] int.
 *
 * Per-object tables, l4p_objects_tables (ws of l4p_objects_tables_ws_bytes(K, T) bytes, K T <= 2^27), one launch over the pixels and
 * one over (k, t).  From integers only: count [K][T] int; bbox [K][T][4] int = x0, y0, x1, y1 inclusive, (0, 0, -1, -1) where count is
 *   0; centroid_px [K][T][2] float = (float)((double)sum / (double)count) of the integer sums of x and of y, 0 where count is 0.
 * With points [T H W][3] float (NULL: no 3D tables, the five 3D outputs are not written) and grid [4] float = (ox, oy, oz, v): a pixel's
 *   point is valid iff v > 0 and v is finite, every coordinate is finite, and per axis, with q = (p - o) / v, s = floorf(q * 256.0f)
 *   lies in [-2^28, 2^28).  The three sums of (long long)s are 64-bit integer atomics.  count3d [K][T] int = n, the valid points;
 *   centroid_xyz [K][T][3] float = (float)((double)o + (((double)sum + 0.5 * (double)n) / ((double)n * 256.0)) * (double)v), in f64,
 *   every operation rounded on its own, 0 where n = 0;  box3d [K][T][6] float = per-axis minimum (3) and maximum (3) of the valid
 *   points (-0 orders below +0), 0 where n = 0;  step [K][T][3] = the f32 difference of the rounded centroids of frames t and t - 1, 0
 *   where either has n = 0 and on frame 0;  speed [K][T] = sqrtf((dx * dx + dy * dy) + dz * dz).
 *   No float sum is accumulated by atomics anywhere.
 *
 * Tracks on objects, l4p_objects_tracks, one thread per track: traj [N][2][T] float (x, y), vis [N][T] float (visibility logits).
 *   Track n is sampled at frame t iff vis > 0, x and y are finite, and gx = floorf(x + 0.5f), gy = floorf(y + 0.5f) lie inside the
 *   frame by the float comparison above.  track_object_nt [N][T] int = object_id under that pixel, or -1;  track_object [N] int = the
 *   non-negative id with the most sampled frames, ties to the smallest id, -1 when there is none;  votes [N] int = that count.
 *
 * Overlay, l4p_objects_overlay: frames, out [T][H][W][3] uchar, lut [K][3] uchar, alpha in [0, 256].  A pixel with id k in [0, K) becomes
 *   (rgb * (256 - alpha) + lut[k] * alpha + 128) >> 8 per channel; other pixels are copied.
 *
 * Every entry returns L4P_E_INVALID, with nothing launched, for a size it refuses or a null pointer it needs; K = 0 and N = 0 are
 * accepted and launch nothing.
 * ---------------------------------------------------------------------------------------------- */
size_t l4p_objects_ws_bytes(int T, int H, int W);
int l4p_objects_label(l4p_stream stream, const float* mask_logit, const float* depth, const float* flow, const unsigned char* keep, int T,
                      int H, int W, int connectivity, float max_depth_ratio, int min_pixels, int min_frames, void* ws, int* label,
                      int* object_id, unsigned long long* counters);
int l4p_objects_roots(l4p_stream stream, const void* ws, const int* label, const int* object_id, int T, int H, int W, long long n_kept,
                      int* root, int* n_pixels, int* first_frame, int* last_frame);
size_t l4p_objects_tables_ws_bytes(int K, int T);
int l4p_objects_tables(l4p_stream stream, const int* object_id, const float* points, const float* grid, int T, int H, int W, int K,
                       void* ws, int* count, int* bbox, float* centroid_px, int* count3d, float* centroid_xyz, float* box3d, float* step,
                       float* speed);
int l4p_objects_tracks(l4p_stream stream, const int* object_id, const float* traj, const float* vis, int N, int T, int H, int W,
                       int* track_object_nt, int* track_object, int* votes);
int l4p_objects_overlay(l4p_stream stream, const unsigned char* frames, const int* object_id, const unsigned char* lut, int T, int H,
                        int W, int K, int alpha, unsigned char* out);

/* ------------------------------------------------------------------------------------------------
 * Object motion and models (csrc/object_motion.hip; this project's own; DESIGN.md "Object motion and models"): per object and frame
 * the rigid motion from frame t - 1 to frame t in the world frame, the poses composed from it, and the object's points carried into
 * the pose of its first frame.  One clip (batch size 1).  Inputs, with m = (t H + y) W + x, H W <= 2^20, T H W <= 2^30, K T <= 2^27:
 *   object_id [T][H][W] int and K as l4p_objects_label writes them (ids outside [0, K) are background);  points [T H W][3] float, the
 *   world points, frame-major;  flow [2][T][H][W] float or NULL, backward flow, channel 0 = x;  grid [4] float = (ox, oy, oz, v).
 * Pairs.  For t >= 1, pixel m of frame t with object_id[m] = k in [0, K) has the predecessor m' = ((t-1) H + yq) W + xq, found exactly
 *   as the temporal edge of l4p_objects_label: without flow (xq, yq) = (x, y); with flow u = flow[0][m], v = flow[1][m], no pair if
 *   either is not finite, gx = floorf(((float)x + u) + 0.5f), gy = floorf(((float)y + v) + 0.5f), no pair unless gx >= 0 && gx <
 *   (float)W && gy >= 0 && gy < (float)H compared in float, (xq, yq) = ((int)gx, (int)gy).  The pair exists iff object_id[m'] == k and
 *   both points are valid by the rule of l4p_objects_tables: v > 0 and finite, every coordinate finite and per axis
 *   s = floorf(((p - o) / v) * 256.0f) in [-2^28, 2^28), f32, every operation rounded on its own.  a = the triple (long long)s of
 *   points[m'] (frame t - 1), b = that of points[m] (frame t).  The motion of row (k, t) is b ~ R a + t, no scale.
 * Moments: 64-bit integer sums by integer atomics (a wave first adds up runs of lanes on one (k, t) by shuffles); no float is summed
 *   by atomics.  2 + n_refits passes over the pixels.
 *   1. Centres: per (k, t) n_pairs = n, sum a [3], sum b [3] (and the row's pixels, pairs or not: an object's first frame is the first
 *      t with a pixel).  c_a = floor(sum a / n), c_b = floor(sum b / n), integer floor division per axis; 0 with n = 0.
 *   2. Fit: d_a = a - c_a, d_b = b - c_b.  A pair with any |d| >= 2^21 is dropped and counted in n_far (every product is then below
 *      2^42 and a sum of products over at most H W <= 2^20 pairs below 2^62; the two sums of squares, three products a pair, stay
 *      below 3 * 2^62 < 2^64: they are accumulated and read as unsigned 64-bit, and moments holds their bit pattern).  moments [18] = n, sum d_a [3], sum d_b [3], sum d_b d_a^T [9]
 *      (row-major: entry 3 i + j = sum d_b[i] d_a[j]), sum |d_a|^2, sum |d_b|^2.
 *   3. Refit, n_refits times: the same moments about the same centres over the pairs that are not far and pass, with the previous
 *      round's emitted f32 motion (R, t) and the raw f32 points pa = points[m'], pb = points[m], all f32, each operation rounded:
 *        pred_i = ((R[i][0] pa.x + R[i][1] pa.y) + R[i][2] pa.z) + t[i];   d = pred - pb;   tau = inlier_voxels * v;
 *        (d.x d.x + d.y d.y) + d.z d.z <= tau tau        (a NaN fails).
 *   n_inliers = n of the last round; n_far is the same in every round.
 * Solve, per (k, t) after each fit pass, f64, every operation rounded on its own, S = (double) of a moment, q = (double)v / 256.0:
 *   C[i][j] = S_ba[i][j] - (S_b[i] S_a[j]) / n;   Saa = S_aa - ((S_a.x S_a.x + S_a.y S_a.y) + S_a.z S_a.z) / n;   Sbb likewise;
 *   valid = n_inliers >= min_pairs (min_pairs >= 3);   R = the rotation of the closed form of csrc/umeyama_moments.hpp
 *   (umeyama_rotation) on cov = C / n when valid, else I;
 *   A[i] = (double)o[i] + (((double)c_a[i] + S_a[i] / n) + 0.5) q,  B likewise (the half is the bias of the floor, as in the tables'
 *   centroid);   t[i] = B[i] - ((R[i][0] A.x + R[i][1] A.y) + R[i][2] A.z);
 *   rms = q sqrt(fmax(0, ((Sbb + Saa) - 2 tr) / n)),  tr = sum over i, j in row-major order of R[i][j] C[i][j].
 *   A row with n_inliers = 0 (no pairs, frame 0, every frame up to the object's first) gets R = I, t = 0, rms = 0; a row with
 *   1 <= n_inliers < min_pairs gets R = I and hence t = B - A, the step of the pairs' centroid.
 * Outputs: motion [K][T][12] float = R row-major, then t, each rounded once from f64;  n_pairs, n_inliers, n_far [K][T] int;
 *   rms [K][T] float;  valid [K][T] uchar;  moments [K][T][18] long long or NULL: the last round's sums.
 * Composition, one thread per object, f64 over the emitted f32 motions M: first = the first frame with a pixel of k (T if none);
 *   G[t] = I for t <= first, G[t] = M[k][t] G[t - 1] after it (R = (M.R G.R row by column, ((a b + c d) + e f)), t = ((M.R G.t)) +
 *   M.t).  pose [K][T][12] float = G rounded;  pose_valid [K][T] uchar = 1 iff valid[k][u] for every first < u <= t.
 * Canonical points, l4p_objects_canonical (needs the ws that l4p_objects_motion left, same K and T): for a pixel of object k,
 *   canonical[m] = (float)(((Ri[i][0] (double)p.x + Ri[i][1] (double)p.y) + Ri[i][2] (double)p.z) + ti[i]) with the inverse of
 *   G[k][t] formed in f64: Ri = G.R^T, ti[i] = -((G.R[0][i] G.t.x + G.R[1][i] G.t.y) + G.R[2][i] G.t.z); every other pixel gets NaN
 *   (l4p_static_map_insert drops it as non-finite).
 * Placement, l4p_objects_place: rows xyz [V][3] float with object [V] int carried to frame t by the f32 pose, in f32:
 *   out[i] = ((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i] of pose[object][t]; NaN for an object outside [0, K).
 * ws: l4p_objects_motion_ws_bytes(K, T) bytes (0 for sizes the entries refuse); every byte that is read is written by
 *   l4p_objects_motion first.  Every entry returns L4P_E_INVALID, with nothing launched, for a size or value it refuses or a null
 *   pointer it needs; K = 0 launches nothing in l4p_objects_motion (l4p_objects_canonical then writes NaN everywhere), V = 0 nothing.
 * ---------------------------------------------------------------------------------------------- */
size_t l4p_objects_motion_ws_bytes(int K, int T);
int l4p_objects_motion(l4p_stream stream, const int* object_id, const float* points, const float* flow, const float* grid, int T, int H,
                       int W, int K, int n_refits, float inlier_voxels, int min_pairs, void* ws, float* motion, int* n_pairs,
                       int* n_inliers, int* n_far, float* rms, unsigned char* valid, long long* moments, float* pose,
                       unsigned char* pose_valid);
int l4p_objects_canonical(l4p_stream stream, const int* object_id, const float* points, const void* ws, int T, int H, int W, int K,
                          float* canonical);
int l4p_objects_place(l4p_stream stream, const float* xyz, const int* object, const float* pose, long long V, int K, int T, int t,
                      float* out);

/* ------------------------------------------------------------------------------------------------
 * Native-resolution results (csrc/upsample.hip; this project's own, the reference stops at 224 x 224; DESIGN.md "Native-resolution
 * results"): joint bilateral up-sampling (Kopf et al. 2007) of low-resolution fields to the pixel grid of the decoded frames.
 *   guide_hi    device uint8 [B][Tg][H][W][3]: the decoded source frames
 *   frame_index device int[T]: source frame of every output frame (stride, mirror padding, temporal crop: the table of
 *               l4p_clip_resize_normalize); NULL = identity, which needs Tg == T
 *   guide_lo    device f32 [B][3][T][h][w]: rgb_b3thw as the network saw it (normalised); mean3 / std3: HOST float[3], read at call time
 *   src         device f32 [B][C][T][h][w]: the low-resolution fields, packed; scale: HOST float[C] or NULL (= all 1)
 *   out         device f32 [B][C][T][H][W];  valid  device uint8 [B][1][T][H][W]
 * Geometry: the frame H x W was resized to res_h x res_w with half-pixel centres and cropped at (crop_i0, crop_j0) to h x w.  For the
 * column X of a full-resolution pixel, in f32, every operation rounded on its own:
 *   sx = float(res_w) / float(W);   x = (float(X) + 0.5f) * sx - 0.5f - float(crop_j0)
 * and y likewise from Y, res_h / H and crop_i0.  inside = -0.5 <= x < w - 0.5 and -0.5 <= y < h - 0.5; the window centre is
 * cx = (int)floorf(x + 0.5f), cy likewise.
 * Taps: the low-resolution pixels (qx, qy) with |qx - cx| <= radius and |qy - cy| <= radius; a tap outside [0, w) x [0, h) is skipped,
 * and so is a tap for which any of the C values src[b][c][t][qy][qx] is not finite.
 * Weights: w_tap = f max(g, range_floor) with
 *   f = exp(-((x - qx)^2 + (y - qy)^2) / (2 sigma_s^2))    (evaluated as the product of its two one-axis factors)
 *   g = exp(-|I_hi - I_lo|^2 / (2 sigma_r^2)), the squared distance summed over the three channels,
 *   I_hi = guide_hi[b][frame_index[t]][Y][X][:] / 255,   I_lo[k] = guide_lo[b][k][t][qy][qx] * std3[k] + mean3[k] (unfused).
 * range_floor > 0 keeps the sum of the weights positive whenever one tap is usable: a pixel whose colour matches no tap degrades to
 * the spatial Gaussian.
 * Result: out[c] = scale[c] (sum w_tap src[c][tap]) / (sum w_tap), f32, the taps added in row-major order of the window (hardware
 * exp2 with pre-scaled constants; no atomics: two runs give the same bits).
 * valid = inside and 0 <= frame_index[t] < Tg and at least one tap was usable; where valid is 0 every channel of out is 0 and
 * nothing is read out of range.
 * L4P_E_INVALID, with nothing launched: a size < 1, C > 8, radius outside 1..3, sigma_s <= 0 or sigma_r <= 0, range_floor outside
 * (0, 1], res_h > H or res_w > W (this is an up-sampler), crop_i0 + h > res_h or crop_j0 + w > res_w or a negative crop, Tg != T with
 * a NULL frame_index, a NULL pointer it needs (all but frame_index and scale).
 * ---------------------------------------------------------------------------------------------- */
int l4p_guided_upsample(l4p_stream stream, const unsigned char* guide_hi, const int* frame_index, const float* guide_lo,
                        const float* mean3, const float* std3, const float* src, const float* scale, int B, int C, int T, int Tg, int H,
                        int W, int res_h, int res_w, int crop_i0, int crop_j0, int h, int w, int radius, float sigma_s, float sigma_r,
                        float range_floor, float* out, unsigned char* valid);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics: what a metrics_module(batch, out, metadata) of L4PLitModule.step computes (l4p/l4p.py:74-78; the reference
 * ships none, the definitions are the benchmarks' own).  B clips per call, results as doubles on the device, nothing synchronises.
 * Per-element arithmetic is f32, one rounding per operation in the order written (tests/metrics_restate.py restates it in numpy);
 * sums are f64, added in a fixed order (no float atomics: a second run gives the same bits); counts are integers.  A metric whose
 * denominator count is 0 is NaN.  Every "valid" pointer may be NULL: all valid.  Every entry refuses B < 1, n < 1, index ranges of
 * 2^31 or more, an unknown mode and a NULL required pointer with L4P_E_INVALID and a text that names the entry.
 * ---------------------------------------------------------------------------------------------- */
#define L4P_DEPTH_ALIGN_NONE 0
#define L4P_DEPTH_ALIGN_MEDIAN 1
#define L4P_DEPTH_ALIGN_LSTSQ 2
#define L4P_METRIC_DENSE_OUT 16   /* doubles per clip of the depth, flow and mask entries */
#define L4P_METRIC_TRACKS_OUT 32  /* doubles per clip of the tracks entry */
#define L4P_METRIC_TRACKS_COUNTS 18
#define L4P_METRIC_CAMERAS_OUT 8  /* doubles per clip of the cameras entry */
/* bytes of workspace of the depth entry for (B, n, mode); the flow and mask entries need what L4P_DEPTH_ALIGN_NONE asks for.  0 for
 * arguments the entries refuse. */
size_t l4p_metric_ws_bytes(int B, long long n, int mode);
/* Depth: est, gt, valid [B][n] (n = T H W).  Element i is valid when valid > 0.5, gt is finite with dmin < gt < dmax, est is finite
 * and > 0.  One alignment (s, t) per clip over all its frames:
 *   L4P_DEPTH_ALIGN_NONE    (1, 0);
 *   L4P_DEPTH_ALIGN_MEDIAN  s = the lower median (rank (c - 1) / 2 of the c valid elements, torch.median) of the f32 quotients
 *                           gt / est, t = 0; NaN when c = 0;
 *   L4P_DEPTH_ALIGN_LSTSQ   argmin over the valid elements of sum (s est + t - gt)^2: the sums in f64 from the f32 inputs, the 2 x 2
 *                           normal equations solved in f64, s and t rounded to f32; NaN when c < 2 or the determinant is <= 0.
 * Then a = min(max(s * est + t, dmin), dmax) (multiply, then add, unfused); a NaN alignment scores no element.  Per clip
 * out[0..5] = c, sum |a - gt| / gt, sum (a - gt) * (a - gt), the counts of max(a / gt, gt / a) < 1.25f, 1.5625f, 1.953125f;
 * out[6..10] = abs_rel, rmse (the f64 square root of the mean), delta1, delta2, delta3; out[11], out[12] = s, t.
 * 0 < dmin < dmax.  Inverse-depth alignment and log-space errors: l4p_metric_depth_full below. */
int l4p_metric_depth(l4p_stream stream, const float* est, const float* gt, const float* valid, int B, long long n, int mode,
                     float dmin, float dmax, void* ws, size_t ws_bytes, double* out);
/* Depth with every alignment and the log-space errors: the arguments of l4p_metric_depth, out [B][L4P_METRIC_DEPTH_FULL_OUT].
 * Element validity, dmin / dmax and the alignments L4P_DEPTH_ALIGN_NONE / _MEDIAN / _LSTSQ with their aligned value a are those of
 * l4p_metric_depth, and out[0..12] are its columns bit for bit.  The fourth alignment is scale and shift in inverse depth:
 *   L4P_DEPTH_ALIGN_LSTSQ_INV  x = 1.f / est, y = 1.f / gt; (s, t) = argmin over the valid elements of sum (s x + t - y)^2: the sums
 *                              in f64 from the f32 x and y, the 2 x 2 normal equations solved in f64, s and t rounded to f32; NaN
 *                              when c < 2 or the determinant is <= 0.  Aligned value: p = s * x + t (multiply, then add, unfused),
 *                              pc = fminf(fmaxf(p, 1.f / dmax), 1.f / dmin), a = fminf(fmaxf(1.f / pc, dmin), dmax).
 * A NaN alignment scores no element.  Errors of a scored element: d = a - gt in f32, and the log error in f64,
 * l = log((double)a) - log((double)gt) (an f32 logf would tie the result to one math library's last bit).  Per clip
 *   out[0..12]   as l4p_metric_depth: c, two sums, three delta counts, abs_rel, rmse, delta1..3, s, t;
 *   out[13..16]  sum (d * d) / gt (f32 terms), sum l, sum l * l, sum |l|  (f64 sums in a fixed order);
 *   out[17]      sq_rel = out[13] / c;
 *   out[18]      rmse_log = sqrt(out[15] / c);
 *   out[19]      log10 = (out[16] / c) / ln 10;
 *   out[20]      silog = 100 sqrt(max(out[15] / c - (out[14] / c)^2, 0));
 *   out[21..23]  NaN (reserved).
 * out[17..20] are NaN when c = 0.  The workspace is l4p_metric_depth_full_ws_bytes(B, n, align) bytes (0 for arguments the entry
 * refuses). */
#define L4P_DEPTH_ALIGN_LSTSQ_INV 3
#define L4P_METRIC_DEPTH_FULL_OUT 24
size_t l4p_metric_depth_full_ws_bytes(int B, long long n, int align);
int l4p_metric_depth_full(l4p_stream stream, const float* est, const float* gt, const float* valid, int B, long long n, int align,
                          float dmin, float dmax, void* ws, size_t ws_bytes, double* out);
/* Optical flow: est, gt, valid [B][2][n].  An element is valid when both valid channels are > 0.5 and both gt channels are finite;
 * epe = sqrtf(du * du + dv * dv).  out[0..4] = c, sum epe, the counts of epe < 1, 3, 5; out[5..8] = epe (mean), 1px, 3px, 5px (the
 * shares below the threshold). */
int l4p_metric_flow(l4p_stream stream, const float* est, const float* gt, const float* valid, int B, long long n, void* ws,
                    size_t ws_bytes, double* out);
/* Motion mask: logit, gt, valid [B][n].  Predicted positive is logit > 0: the reference's sigmoid(logit) > 0.5 without the rounding
 * of the sigmoid; gt positive is gt > 0.5; over the elements with valid > 0.5: out[0..3] = TP, FP, FN, TN; out[4..8] = iou =
 * TP / (TP + FP + FN), precision, recall, f1 = 2 TP / (2 TP + FP + FN), accuracy. */
int l4p_metric_mask(l4p_stream stream, const float* logit, const float* gt, const float* valid, int B, long long n, void* ws,
                    size_t ws_bytes, double* out);
/* Tracks, the TAP-Vid measures: traj_est, traj_gt [B][N][2][T], vis_logit [B][N][T], vis_gt and valid [B][N][T] bytes (non-zero =
 * set), queries [B][N][3] = (t + 0.5, x, y) as sample_tracks writes them.  Frame t of track i is scored when valid is set and
 * t != floor(query t); datasets that clear valid before the query frame give TAP-Vid's "first" protocol.  Distances are taken in
 * TAP-Vid's 256 x 256 frame: sx = 256.f / W, sy = 256.f / H, dx = (xe - xg) * sx, dy likewise, d2 = dx * dx + dy * dy, and for thr
 * in {1, 2, 4, 8, 16} within = d2 < thr * thr; predicted visible is vis_logit > 0.  counts [B][L4P_METRIC_TRACKS_COUNTS] (workspace,
 * cleared here) and out[0..17] = scored frames, frames with predicted == gt visibility, gt-visible frames, then per threshold:
 * within & gt visible [3..7], TP = within & predicted visible & gt visible [8..12], FP = predicted visible & !(gt visible & within)
 * [13..17].  out[18] = occlusion_accuracy, out[19..23] = pts_within_thr, out[24..28] = jaccard_thr = TP / (gt visible + FP),
 * out[29] = average_pts_within_thresh, out[30] = average_jaccard (the means over the five thresholds). */
int l4p_metric_tracks(l4p_stream stream, const float* traj_est, const float* traj_gt, const float* vis_logit,
                      const unsigned char* vis_gt, const unsigned char* valid, const float* queries, int B, int N, int T, int H, int W,
                      unsigned long long* counts, double* out);
/* 3D tracks, the TAP-Vid measures on camera-space points with depth-adaptive thresholds: traj_est, traj_gt [B][N][2][T] and
 * depth_est, depth_gt [B][N][T] (track_2d_depth_est_bn1t / track_2d_depth_bn1t: (x, y, z) of frame t), vis_logit [B][N][T], vis_gt
 * and valid [B][N][T] bytes (valid may be NULL), queries [B][N][3], intrinsics [B][4][4][T] (intrinsics_b44t in the pixel units of
 * the clip; only fx = K[0][0][t], fy = K[1][1][t], cx = K[0][2][t], cy = K[1][2][t] are read).  All f32, one rounding per operation:
 *   unprojection (unproject_2d_track_to_3d, geometry_utils.py:69-78): X = ((x - cx) * z) / fx, Y = ((y - cy) * z) / fy, Z = z;
 *     G from the gt, E from the estimate WITH THE GT INTRINSICS;
 *   scored:    valid set, t != floor(query t), zg finite and > 0;
 *   eligible:  scored, gt visible, ze finite and > 0;
 *   ratio:     r = |G| / |E| with |P| = sqrtf((X * X + Y * Y) + Z * Z);
 *   scale s of track i:
 *     L4P_TRACK3D_SCALE_NONE          s = 1;
 *     L4P_TRACK3D_SCALE_MEDIAN        the lower median (rank (c - 1) / 2, torch.median) of r over the c eligible frames of the
 *                                     clip, NaN when c = 0;
 *     L4P_TRACK3D_SCALE_TRACK_MEDIAN  the lower median of r over the eligible frames of track i alone, NaN when it has none;
 *     L4P_TRACK3D_SCALE_QUERY         zg / ze at frame floor(query t): that frame must lie in [0, T), have valid set (NULL = set)
 *                                     and both depths finite and > 0, otherwise NaN;
 *   distance:  dx = s * Ex - Gx, dy, dz likewise, d = sqrtf((dx * dx + dy * dy) + dz * dz);
 *   thresholds, depth-adaptive in TAP-Vid's 256 x 256 frame: sx = 256.f / W, sy = 256.f / H, f = sqrtf((fx * sx) * (fy * sy)),
 *     u = zg / f, and for thr in {1, 2, 4, 8, 16} within = d < (float)thr * u.
 * A NaN scale (or a NaN distance: a missing estimate) makes every `within` of the frame false; the frame stays in the
 * denominators - a miss, not an exclusion.  Predicted visible is vis_logit > 0.  counts [B][L4P_METRIC_TRACKS_COUNTS] (workspace,
 * cleared here) and out[0..30] have exactly the layout and the formulas of l4p_metric_tracks.  out[31] = the clip's s for
 * L4P_TRACK3D_SCALE_NONE / _MEDIAN, the number of tracks with a finite scale for _TRACK_MEDIAN / _QUERY.  The ratios are expected
 * not to be NaN (finite coordinates); a NaN ratio sorts above every other.
 * Refused: B, N, T, H or W < 1, B * N * T >= 2^31, an unknown scale, a NULL pointer other than valid, ws_bytes below
 * l4p_metric_tracks3d_ws_bytes(B, N, T, scale) (0 for arguments the entry refuses). */
#define L4P_TRACK3D_SCALE_NONE 0
#define L4P_TRACK3D_SCALE_MEDIAN 1
#define L4P_TRACK3D_SCALE_TRACK_MEDIAN 2
#define L4P_TRACK3D_SCALE_QUERY 3
size_t l4p_metric_tracks3d_ws_bytes(int B, int N, int T, int scale);
int l4p_metric_tracks3d(l4p_stream stream, const float* traj_est, const float* traj_gt, const float* depth_est, const float* depth_gt,
                        const float* vis_logit, const unsigned char* vis_gt, const unsigned char* valid, const float* queries,
                        const float* intrinsics, int B, int N, int T, int H, int W, int scale, void* ws, size_t ws_bytes,
                        unsigned long long* counts, double* out);
/* Cameras, ATE / RPE with the RMSE statistic: pose_est [B][16][T] row-major world_T_cam (traj3d_est_b16t), extr_gt [B][4][4][T]
 * cam_T_world (extrinsics_b44t, inverted in f64: G).  f64 throughout.  The closed-form similarity (s, R, t) of the estimated onto
 * the gt camera centres over all T frames (Umeyama, reflection case included, no RANSAC), then out[0] = ate = RMSE of
 * |s R c_est + t - c_gt|; with the estimate's translations multiplied by s and E = inv(inv(G_i) G_i+1) (inv(P_i) P_i+1) for
 * consecutive frames: out[1] = rpe_trans = RMSE of |trans(E)|, out[2] = rpe_rot = RMSE in degrees of
 * atan2(0.5 |(E32 - E23, E13 - E31, E21 - E12)|, 0.5 (trace - 1)); out[3] = s, out[4..6] = the three sums of squares, out[7] = T.
 * T >= 3.
 * Degenerate centres (the closed form of csrc/umeyama_moments.hpp, shared with l4p_similarity_ransac; ms, md = the means of the
 * estimated and the gt centres, var_s = the variance of the estimated ones, cov = their cross-covariance): R is a proper rotation
 * (R R^T = I, det R = +1) whatever the rank of cov - collinear centres leave the rotation about their line free, and it is fixed by
 * completing the left singular vectors from the right ones: R = I when the gt line is the estimated line in the same sense (to
 * rounding, and R stays near I as one line turns away from the other); cov = 0 gives R = I.  var_s = 0 (a
 * static estimate) gives s = 1 and t = md - R ms; cov = 0 with var_s > 0 (a static gt) gives s = 0, hence t = md.  All finite. */
int l4p_metric_cameras(l4p_stream stream, const float* pose_est, const float* extr_gt, int B, int T, double* out);

/* ------------------------------------------------------------------------------------------------
 * SAM-style point tracker (sparse_heads.py, sam/{prompt_encoder,transformer,mask_decoder}.py).
 * The projections of the two-way transformer run through l4p_gemm; these are the remaining pieces.
 * ---------------------------------------------------------------------------------------------- */

/* LayerNorm with the tracker's fused extras: y = LN(x) [then GELU if act == L4P_ACT_GELU, as in
 * mask_decoder.py:60-62]; out_f32 = y, out_T = T(y), out_T2 = T(y + add[row % add_mod]) — the
 * "queries + query_pe" / "keys + key_pe" operands of sam/transformer.py:166-185. */
int l4p_layernorm_ex(l4p_stream stream, int dtype, const float* x, const float* gamma, const float* beta, float eps,
                     void* out_T, float* out_f32, int M, int C, const float* add, int add_mod, void* out_T2, int act);

/* keys = LayerNorm(keys + attention output) (sam/transformer.py:183-185) with the sum formed in the LayerNorm: the row
 * normalised is x[row % x_mod] (float; x_mod = 0: x[row]) + delta[row] (engine dtype, the out projection's result), outputs as
 * l4p_layernorm_ex.  The float key stream is read once here instead of read + written by the projection's epilogue and read
 * again; out_f32 may alias x when x_mod = 0.  x_shared (may be NULL): rows p = row % x_period with p >= x_split read
 * x_shared[p - x_split] instead - the part of the key stream that is the same for every track of a later window (encoder
 * feature + the learned mask token: l4p_track_keys_init's k32_shared); x_shared is never written, so out_f32 may still alias x. */
int l4p_layernorm_res(l4p_stream stream, int dtype, const float* x, int x_mod, const void* delta_T, const float* gamma,
                      const float* beta, float eps, void* out_T, float* out_f32, int M, int C, const float* add, int add_mod,
                      void* out_T2, const float* x_shared, int x_period, int x_split, float* out_stats);
/* ... out_stats (may be NULL): float [M][2] = (mean, rstd) of every row, and
 * l4p_layernorm_chain: the NEXT layer's keys = LayerNorm(y_prev + delta) where y_prev - the float result of an l4p_layernorm_res launch
 * over x_shared_rows[row % x_mod] + delta_prev[row] that stored only its engine-dtype outputs and out_stats - is re-derived from those
 * inputs, bit for bit (same affine form, same statistics).  The tracker's second layer in a first window: the float key master
 * [N * P][C] is neither written by layer 0 nor read by layer 1 (1.1 GB of 3.7 GB per 64 tracks).  Outputs as l4p_layernorm_ex. */
int l4p_layernorm_chain(l4p_stream stream, int dtype, const float* x_shared_rows, int x_mod, const void* delta_prev_T, const float* stats_prev,
                        const float* gamma_prev, const float* beta_prev, const void* delta_T, const float* gamma, const float* beta, float eps,
                        void* out_T, float* out_f32, int M, int C, const float* add, int add_mod, void* out_T2);

/* The same LayerNorm (+ optional GELU) for rows that are STORED in the engine dtype: x_T, out_T are T [M][C] and may be the
 * same buffer.  Used for LayerNorm3d + GELU after the first up-scaling ConvTranspose (mask_decoder.py:60-62), whose 1M x 352
 * activation per clip is then never held in float (the reference holds it in fp16 under autocast).  L4P_F32: T = float. */
int l4p_layernorm_t(l4p_stream stream, int dtype, const void* x_T, const float* gamma, const float* beta, float eps,
                    void* out_T, int M, int C, int act);

/* PromptEncoder (prompt_encoder.py:78-121,196-203) + token concat (mask_decoder.py:107-113):
 * tokens float [N][6][C] = 3 mask tokens | point PE + label embedding | not-a-point | feature prompt. */
int l4p_track_tokens(l4p_stream stream, const float* queries, const float* labels, const float* pfeat,
                     const float* plabel, const float* gauss, const float* mask_tokens, const float* point_emb0,
                     const float* point_emb1, const float* not_a_point, const float* feat_emb0, const float* feat_emb1,
                     float* tokens, int N, int C, int T, int H, int W);

/* keys = enc_features[-1] (broadcast over queries) + per-query history (sparse_heads.py:341-346):
 * k32 float, kT = T(keys), kP = T(keys + dense_pe), each [N][P][C].
 * shared_from > 0 (later windows of a long clip: the history rows [shared_from, P) of every track are the learned mask token
 * again, sparse_heads.py:418-427): those rows are formed for track 0 only - hist rows past shared_from of the other tracks
 * are not read, their k32 / kT / kP rows not written - and track 0's float rows are also stored in k32_shared
 * [P - shared_from][C] (the residual master l4p_layernorm_res reads for those rows of every track).  shared_from = 0: every
 * row of every track (k32_shared ignored). */
int l4p_track_keys_init(l4p_stream stream, int dtype, const float* enc, const float* hist, const float* pos,
                        float* k32, void* kT, void* kP, int N, int P, int C, int shared_from, float* k32_shared);

/* Broadcast a C-vector into `rows` rows of a float matrix (row map as in l4p_gemm_desc.a_*): the learned
 * mask token of the memory mechanism (sparse_heads.py:262-265,418-427). */
int l4p_fill_rows(l4p_stream stream, float* out, const float* v, long long rows, int C, long long group_rows,
                  long long group_stride, long long group_off);

/* Copies the `bytes` bytes at base + off to the same offset of the following n - 1 groups (group g starts at base + g * stride;
 * all multiples of 16).  Later tracker windows (sparse_heads.py:406-448): the second temporal half of every track's keys is
 * encoder feature + the same learned mask token, so what layer 0 derives from it (rows [P/2, P) of t2i.k, t2i.v, i2t.q) is
 * computed for track 0 and copied to the other tracks' rows. */
int l4p_broadcast_block(l4p_stream stream, void* base, long long off, long long bytes, long long stride, int n);

/* Attention of sam/transformer.py:223-245 after the projections. kind 0: 6 prompt tokens among themselves
 * (q,k,v,out [N][6][D]); kind 1: tokens -> image (q [N][6][D], k,v [N][P][D], out [N][6][D]);
 * kind 2: image -> tokens (q [N][P][D], k,v [N][6][D], out [N][P][D]);
 * kind 3 / 4: kinds 1 / 2 when every track still has the SAME image-side operand (first window, first layer: the
 * keys have not been touched by a query yet): k,v [P][D] resp. q [P][D] are shared, outputs stay per track. */
int l4p_small_attn(l4p_stream stream, int dtype, int kind, const void* q, const void* k, const void* v, void* out,
                   int N, int P, int D, int heads);

/* masks[n][m][vox] = hyper[n][m][:] . up[n][vox][:]  (mask_decoder.py:139); up channels-last T. */
int l4p_mask_product(l4p_stream stream, int dtype, const void* up, const float* hyper, float* masks, int N,
                     long long vox, int C);

/* masks[n][i][t][y][x] (the [N][3][T][2h][2w] logits of mask_decoder.py:139) from the L4P_EPI_MASKDOT partial sums of
 * the (1,2,2) ConvTranspose over M = N*T*h*w rows: row m = ((n*T + t)*h + y/2)*w + x/2, tap = (y%2)*2 + x%2, chunks_per_tap
 * chunks each. */
int l4p_mask_gather(l4p_stream stream, const float* partial, float* masks, int N, int T, int h, int w, int chunks_per_tap);

/* Folded image -> token attention of the tracker (sam/transformer.py:180-185,223-245; the projections of the 2048 x N image
 * tokens are folded into the 6 prompt tokens of each track, l4p_amd/models/task_heads/sparse_heads.py "folded i2t"):
 * l4p_i2t_probs: scores float [M][ld_scores], column t * heads + h = scaled score of image token m against prompt token t in head h
 *   (pairs != 0: columns tokens * heads + t * heads + h hold a second addend - the scores against the low halves of the folded key
 *   matrix; cbias != NULL: + cbias[(m / rows_per_group) * tokens * heads + t * heads + h], the track's query-bias term)
 *   -> probs T [M][ld_probs]: softmax over t for every h, same column order, columns tokens * heads .. ld_probs - 1 zero.
 * l4p_split_hilo: in float [G][R][C] -> out T [G][2 R][C], rows [0, R) = T(x), rows [R, 2 R) = T(x - T(x)): a folded key matrix as a
 *   PAIR of engine-dtype matrices (an option for its 1408-term products with the keys; off by default: no measurable effect).
 * l4p_transpose_pad: in T [G][R][C] -> out T [G][C][Rp] (k index padded with zeros): a track's folded value matrix in the
 *   k-contiguous form l4p_gemm reads weights in. */
int l4p_i2t_probs(l4p_stream stream, int dtype, const float* scores, long long ld_scores, int pairs, const float* cbias, int rows_per_group,
                  void* probs_T, int ld_probs, long long M, int heads, int tokens);
int l4p_split_hilo(l4p_stream stream, int dtype, const float* in, void* out_T, int G, int R, long long C);
/* Token -> image attention (l4p_small_attn kind 1) from scores formed elsewhere: scores float [N * P][ld_scores], column t * heads + h
 * = scaled score of prompt token t against image token p in head h (the keys' projection folded into the tokens: scores = kP x Q'^T,
 * Q' = q W_k per head; the key bias shifts all P scores of a (t, h) alike and drops out of the softmax); v T [N][P][D];
 * out T [N][6][D] = softmax over p, then P.V. */
int l4p_t2i_attn_scores(l4p_stream stream, int dtype, const float* scores, long long ld_scores, const void* v_T, void* out_T, int N, int P,
                        int D, int heads);
int l4p_transpose_pad(l4p_stream stream, int dtype, const void* in_T, void* out_T, int G, int R, int C, int Rp);
/* Token -> image attention with the value projection folded away as well (sam/transformer.py:168-173,223-245):
 *   out[t, head h] = sum_p prob[t,h,p] (keys[p] Wv_h^T + bv_h) = (sum_p prob[t,h,p] keys[p]) Wv_h^T + bv_h.
 * l4p_t2i_probs: scores float [N][P][ld_scores] (column t * heads + h, 48 of them) -> e T [N][P][48] = exp(score - m) with m the column
 *   maximum over the SPLIT of 256 keys the row belongs to, and stats float [N][ceil(P / 256)][2][48]: those maxima, and the splits'
 *   sums of e AS ROUNDED to T (the weights the context product applies then sum to one exactly).  (One coalesced pass over 8 x N workgroups; the softmax over all P keys is assembled by l4p_t2i_context: a split's
 *   terms carry exp(m_split - M) / Z.)
 * l4p_t2i_context: ctx T [(h * Rg + n * tokens + t)][C] = sum_p softmax_p[n][p][t * heads + h] * keys[n][p][C] (keys T [N][P][C] WITHOUT
 *   the positional term; rows grouped by head with Rg >= N * tokens rows per group, a multiple of 128, rows past N * tokens untouched):
 *   the A operand of the row-grouped-weights GEMM against the head blocks of W_v (w_gr = Rg, w_gs = hd * C, b_gs = o_gs = hd, c_gr = Rg).
 *   heads * tokens == 48, C % 64 == 0, P % 32 == 0, 96 <= P <= 4096.  bf16: MFMA kernel bound by one read of the keys.
 *   shared_from (a multiple of 32; >= P: none): key rows p >= shared_from of EVERY track are read from track 0's block - later windows of
 *   the recursion, layer 0: the second temporal half of every track's keys is still the same (l4p_track_keys_init(shared_from)). */
/* delta = P x V' + b of the folded image -> token attention as a streaming kernel (bf16, K == 64, C % 128 == 0, P % 16 == 0): probs T
 * [N][P][64] (l4p_i2t_probs), vt T [N][C][64] (l4p_transpose_pad), bias float [C] or NULL -> delta T [N][P][C].  Bit-identical to
 * l4p_gemm with w_gr = P, w_gs = C * 64 on the same operands, which serves every other shape / dtype. */
int l4p_i2t_delta(l4p_stream stream, int dtype, const void* probs_T, const void* vt_T, const float* bias, void* delta_T, int N, int P, int C,
                  int K);
int l4p_t2i_probs(l4p_stream stream, int dtype, const float* scores, long long ld_scores, void* probs_T, float* stats, int N, int P, int HT);
int l4p_t2i_context(l4p_stream stream, int dtype, const void* probs_T, const float* stats, const void* keys_T, void* ctx_T, int N, int P,
                    int C, int heads, int tokens, long long Rg, int shared_from);

/* Fused read-out (sparse_heads.py:572-589,645-647): trilinear (align_corners=False) resize of masks
 * [N][3][T][h][w] to H x W, soft-argmax of channel 0 (traj [N][2][T]), spatial mean of channel 1
 * (vis [N][T]) and exp(mean) of channel 2 (depth [N][T]); the up-sampled logits are never stored.  The soft-argmax is the
 * reference's (torch.softmax of the up-sampled map) for any finite logits, however peaked.  L4P_E_INVALID, with nothing
 * launched, for a null pointer, a size < 1, or source maps (3 h w + w + h floats) that do not fit one workgroup's LDS. */
int l4p_track_readout(l4p_stream stream, const float* masks, float* traj, float* vis, float* depth, int N, int T,
                      int h, int w, int H, int W);

/* Sliding-window state of forward_windowed_core (sparse_heads.py:303-335 prepare; :366-393,:455-486 commit).
 * Integer / boolean results (valid masks, labels {0,1,2}, argmax index) are bit-exact w.r.t. the reference. */
int l4p_track_prepare(l4p_stream stream, const float* cur_q, const float* orig_q, int start, int ws, float* q_off,
                      float* labels, unsigned char* valid_t, unsigned char* valid_n, int N);
int l4p_track_commit(l4p_stream stream, const float* w_traj, const float* w_vis, const float* w_depth,
                     const unsigned char* valid_t, const unsigned char* valid_n, float* traj, float* vis, float* depth,
                     int T, int start, int ws, int next_start, int last_window, float* cur_q, float* plabel,
                     const float* new_pfeat, float* pfeat, int* best_out, int N, int C);

/* Tracking in both time directions (estimation_directions [1, -1]).  The reference's recursion is causal - a frame is estimated iff
 * frame centre - query time >= 0 (sparse_heads.py:306-316) - and its assert names the recipe for the frames before a query
 * (sparse_heads.py:242-245): "Run twice, with and without video flipping, and then combine outputs".  The reversed pass is the same
 * recursion on the time-flipped clip (frame f' of it is frame T-1-f' of the input) with the queries ((float)T - tq, x, y); output frame g
 * of a track is the forward pass's iff ((float)g + 0.5f) - tq >= 0 in f32 (the expression l4p_track_prepare evaluates), else the reversed
 * pass's at frame T-1-g: traj (both channels), vis and depth alike.  At the query frame the forward value wins.
 * Each entry returns L4P_E_INVALID, with nothing launched, for a null pointer it needs, a size < 1, or src == dst in the first.
 *   l4p_time_reverse       : float [outer][T][inner] -> the same shape with the T axis reversed; src != dst.  16-byte accesses when
 *                            inner % 4 == 0 and both pointers are 16-byte aligned, scalar ones otherwise.  (rgb_b3thw: outer = 3 B, inner = H W)
 *   l4p_track_bidir_queries: q_rev [BN][3] = the flipped queries; ADDS to the device int need_count (zeroed by the caller) the number of
 *                            queries with at least one frame before them, (0.5f - tq) < 0: 0 means the reversed pass owns no frame.
 *   l4p_track_bidir_merge  : traj [B][N][2][T], vis / dep [B][N][T] by the rule above; the reversed buffers are read mirrored (they are
 *                            never flipped in memory).  mode 0: both passes; the outputs may be the forward buffers themselves.  mode 1: no
 *                            forward pass (directions [-1]): forward-owned frames get the fill values 0 / -10 / 0, traj_f / vis_f / dep_f
 *                            may be NULL. */
int l4p_time_reverse(l4p_stream stream, const float* src, float* dst, int outer, int T, long long inner);
int l4p_track_bidir_queries(l4p_stream stream, const float* q_bn3, int T, float* q_rev_bn3, int* need_count, int BN);
int l4p_track_bidir_merge(l4p_stream stream, const float* q_bn3, const float* traj_f, const float* vis_f, const float* dep_f,
                          const float* traj_r, const float* vis_r, const float* dep_r, float* traj, float* vis, float* dep, int B, int N,
                          int T, int mode);

/* ------------------------------------------------------------------------------------------------
 * Engine: holds the table of packed device weights and runs whole sub-networks with one call.
 * ---------------------------------------------------------------------------------------------- */

int l4p_create(int device, int dtype, l4p_engine** out);
int l4p_destroy(l4p_engine* e);

/* Register a packed weight that lives in caller-owned device memory (the Python host packs the
 * reference state_dict — models/utils.py:52-53 — into kernel layouts and keeps the arena alive). */
int l4p_bind_weight(l4p_engine* e, const char* name, const void* dev_ptr, long long numel);

typedef struct l4p_encoder_cfg {
    int dim, depth, heads, head_dim, mlp_hidden;
    int in_chans, frames, img_h, img_w, pt, ph, pw; /* tubelet */
    int patch_kp;                                    /* padded gather width (multiple of 64) */
    float ln_eps;
} l4p_encoder_cfg;

int l4p_encoder_configure(l4p_engine* e, const l4p_encoder_cfg* cfg);
size_t l4p_encoder_workspace_bytes(const l4p_engine* e, int B);

/* VideoMAEEncoder.forward (l4p_videomae.py:80-122): patch embed + sinusoid pos + `depth` pre-LN
 * blocks + final norm.  The reference returns all depth+1 features; here the caller names the taps
 * it wants: tap_layer[i] in [0, depth] (0 = embeddings, k = after k blocks, depth = norm(x_depth)),
 * written as float to tap_f32[i] and/or as T to tap_T[i] (either may be NULL), each [B*tokens][dim].
 * Blocks after the highest requested tap are not executed. */
int l4p_encoder_forward(l4p_engine* e, l4p_stream stream, const float* rgb, int B, void* workspace, size_t ws_bytes,
                        int n_taps, const int* tap_layer, float* const* tap_f32, void* const* tap_T);

/* DPTOutputAdapter_fix.forward (dpt_head.py:41-86) of one dense head as a single call: act_postprocess (1x1x1 conv +
 * ConvTranspose / strided conv), layer_rn, four FeatureFusion blocks, head1, trilinear resize, head2, output
 * projection (+exp).  hooks[i]: T [B][nt*nh*nw][dim] features of the head's hook layers; out: float
 * [B][out_ch][out_t][out_h][out_w].  Weights "dpt.<task>.*" must have been bound with l4p_bind_weight.
 * actpost / fusion are the reference's scale-factor tuples (dense_heads.py:30-31, :269-271). */
typedef struct l4p_dpt_cfg {
    int dim, nt, nh, nw;
    int layer_dims[4];
    int feature_dim, last_dim, out_ch;
    int actpost[4][3];
    int fusion[4][3];
    int out_t, out_h, out_w;
    int post_exp;
} l4p_dpt_cfg;

size_t l4p_dpt_workspace_bytes(const l4p_engine* e, const l4p_dpt_cfg* cfg, int B);
int l4p_dpt_forward(l4p_engine* e, l4p_stream stream, const char* task, const l4p_dpt_cfg* cfg, const void* const* hooks,
                    int B, void* workspace, size_t ws_bytes, float* out);

/* One window of the SAM-style tracker for the N queries of ONE clip as a single call (VideoMAETrack2DSamHead.forward /
 * forward_single_batch, sparse_heads.py:497-667, with PromptEncoder, TwoWayTransformer and MaskDecoder.predict_masks):
 * prompt tokens, key initialisation, sam_depth two-way layers + final attention, hyper-network MLPs, prompt feature for
 * the next window, memory tokens (need_history), up-scaling fused with the mask product, fused up-sample + soft-argmax.
 * enc_last float [P][C] (enc_features[-1] of the clip); hist float [N][P][C] per-query history tokens (read; rewritten in
 * place for the next window when need_history: the second temporal half of the processed tokens projected into rows
 * [0, P/2), rows [P/2, P) set to the learned mask token; need_history == 2: the caller guarantees that rows [P/2, P) already
 * hold the mask token - true for a buffer that was filled with it once and only ever passed to this function, which writes
 * nothing else there - and the fill is skipped; need_history == 3: hist [N][P][C] receives the projection of ALL P processed
 * tokens of every track, the reference's <task>_enc_features_with_track_history_bnpc of a plain single-window forward) — or, with hist_uniform (every track still has the same history rows: the
 * first window / the plain single-window forward), only its first P rows are read; hist_uniform == 2: rows [P/2, P) of every
 * track's history are identical (the state need_history leaves behind: the learned mask token), so the layer-0 projections
 * of those rows are computed once and copied (l4p_broadcast_block) — same values, half the key-side projection work of
 * layer 0; hist_uniform == 2 or 4 name a LATER window of a recursion (4: without the half-sharing of 2, every track on its own rows -
 * the equality check of that shortcut): layer 0's token -> image attention then takes the folded form of the later layers
 * (packing.py fold_t2i: scores against the folded prompt tokens, softmax x keys on the matrix pipe, the head blocks of W_v on the 48
 * context rows) instead of projecting N x P key rows twice and attending per (track, head) - L4P_TRACK_FOLD_L0=0: the projected
 * form; hist_uniform == 0 (a window evaluated out of context) keeps the projected form, bit-identical to the first window's shortcut;
 * q_off float [N][3] (t, x, y) relative
 * to the window; labels, plabel float [N]; pfeat float [N][C].  Outputs: traj float [N][2][T], vis, depth float [N][T],
 * new_pfeat float [N][C].  Weights "trk.*" must have been bound with l4p_bind_weight. */
typedef struct l4p_track_cfg {
    int dim, tokens, nt, nh, nw; /* key geometry: tokens = nt * nh * nw */
    int sam_depth, sam_heads, sam_mlp, out_dim_factor;
    int T, H, W; /* window / image size the masks are read out at */
} l4p_track_cfg;
size_t l4p_track_window_workspace_bytes(const l4p_engine* e, const l4p_track_cfg* cfg, int N, int hist_uniform);
int l4p_track_window_forward(l4p_engine* e, l4p_stream stream, const l4p_track_cfg* cfg, const float* enc_last, float* hist,
                             const float* q_off, const float* labels, const float* pfeat, const float* plabel, int N,
                             int need_history, int hist_uniform, void* workspace, size_t ws_bytes, float* traj, float* vis,
                             float* depth, float* new_pfeat);

/* ------------------------------------------------------------------------------------------------
 * Clip preparation (the caller side of the hot path): decoded uint8 frames in HBM ->
 * the network's input tensor.  Replaces VideoDataset.getitem_helper's per-frame PIL resize-blur-resize +
 * to_tensor (l4p/data/video_dataset.py:86-93) and L4PDataset.__getitem__'s mirror-pad / resize / crop /
 * normalise (l4p/data/l4p_dataset_mini.py:543-587, :126-190, :236-288, :290-391).
 * ------------------------------------------------------------------------------------------------ */

/* HOST function (no GPU work): Pillow's coefficient tables for one axis of Image.resize(BILINEAR) over the
 * full axis (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc: triangle filter, support scaled
 * by the down-scale factor, 22-bit fixed point).  bounds: host int[2*out_size] (first tap, tap count);
 * coeffs: host int[out_size * ksize].  With bounds == NULL or coeffs == NULL only *ksize is written. */
int l4p_pil_coeffs(int in_size, int out_size, int* bounds, int* coeffs, int coeffs_cap, int* ksize);

/* One 8-bit pass of Pillow's resampler on n_img images [in_h][in_w][channels] (uint8, device):
 * axis 1 = horizontal (in_w -> out_size), axis 0 = vertical (in_h -> out_size).  bounds / coeffs: the tables of
 * l4p_pil_coeffs copied to the device.  Integer arithmetic, bit-exact with Pillow. */
int l4p_pil_resample_u8(l4p_stream stream, const unsigned char* src, unsigned char* dst, long long n_img, int in_h,
                        int in_w, int channels, int axis, int out_size, const int* bounds, const int* coeffs, int ksize);

/* rgb_out[c][t][y][x] (float, [3][T_out][out_h][out_w]) =
 *   (bilinear(frame[frame_index[t]] / 255 resized to res_h x res_w)[y + crop_i0][x + crop_j0] - mean[c]) / std[c]
 * with F.interpolate(align_corners=False) arithmetic (skipped, as in the reference, when res == in).  frame_index
 * (device int[T_out]) carries stride, temporal mirror-padding and the temporal crop.  mean3 / std3: HOST float[3],
 * read at call time.  frames: uint8 [n][in_h][in_w][3]; OR, when vbounds != NULL, [n][src_h][in_w][3] = the frames
 * before a final vertical Pillow pass src_h -> in_h (tables vbounds / vcoeffs / vksize on the device), which is then
 * evaluated on the fly for the <= 4 pixels an output pixel needs instead of being written out.
 * Compact rows (x_lambda != NULL): an output column j only reads source columns i0[j], i1[j] (l4p_resize_index_table),
 * so the caller may produce just those — frames is then [n][src_h][2*out_w][3] with columns (i0[0], i1[0], i0[1], ...)
 * and x_lambda the device copy of lambda1[out_w]; the previous horizontal pass shrinks accordingly. */
int l4p_clip_resize_normalize(l4p_stream stream, const unsigned char* frames, const int* frame_index, float* rgb_out,
                              int T_out, int in_h, int in_w, int res_h, int res_w, int crop_i0, int crop_j0, int out_h,
                              int out_w, const float* mean3, const float* std3, int src_h, const int* vbounds,
                              const int* vcoeffs, int vksize, const float* x_lambda);

/* HOST function: the source indices / weight of F.interpolate(align_corners=False) along one axis, exactly as the
 * kernel evaluates them (float32, source coordinate = one fma): output j (0 <= j < out_size) of the crop starting at
 * crop0 of the axis resized in_size -> res_size reads i0[j], i1[j] with weights 1 - lambda1[j], lambda1[j]. */
int l4p_resize_index_table(int in_size, int res_size, int crop0, int out_size, int* i0, int* i1, float* lambda1);

/* ------------------------------------------------------------------------------------------------
 * DAVIS / DyCheck datasets: the per-pixel work the instance masks add (l4p/data/davis.py:96-110) and the query
 * selection of sample_tracks, version "uniform_over_seg" (l4p/data/l4p_dataset_mini.py:450-465).
 * ------------------------------------------------------------------------------------------------ */

/* HOST function: the source index of every output position of PIL.Image.resize(..., NEAREST) along one full axis
 * (what Image.resize does to mode "P" / "1" images whatever filter is asked for: davis.py:101-102 on a palette
 * annotation).  _imaging.c _resize + libImaging/Geometry.c ImagingScaleAffine: the source coordinate starts at
 * half a step and is accumulated in double.  idx: host int[out_size]. */
int l4p_pil_nearest_table(int in_size, int out_size, int* idx);

/* HOST function: the source index of F.interpolate(mode="nearest") given `size` along one axis
 * (l4p_dataset_mini.py:266 for instanceseg_b1thw; ATen nearest_idx, float32 scale).  idx: host int[out_size]. */
int l4p_torch_nearest_table(int in_size, int out_size, int* idx);

/* mask_out[t][y][x] (float, [T_out][out_h][out_w] = instanceseg_b1thw) =
 *   float(src[frame_index[t]][ytab[y]][xtab[x]] > 0)
 * src: uint8 annotation frames [n_src][in_h][in_w] with pix_stride bytes between pixels (3 reads the first channel
 * of an RGB annotation in place).  Replaces davis.py:98-110 (Pillow round trip of a palette mask, to_tensor[:1],
 * mean over the size-1 dimension > 0), the mirror padding, F.interpolate(nearest) (l4p_dataset_mini.py:266) and the
 * centre crop (:315-337): frame_index (device int[T_out]) is the table of l4p_clip_resize_normalize; ytab / xtab
 * (device int[out_h] / int[out_w]) are the index maps of those stages composed on the host.  An entry outside the
 * source gives NaN. */
int l4p_instance_mask_clip(l4p_stream stream, const unsigned char* src, int n_src, int in_h, int in_w, int pix_stride,
                           const int* frame_index, const int* ytab, const int* xtab, float* mask_out, int T_out,
                           int out_h, int out_w);

/* Query selection of sample_tracks "uniform_over_seg" (l4p_dataset_mini.py:450-465): candidate m with cell
 * (cells[2m], cells[2m+1]) = (x_id, y_id) is kept iff the 3x3 erosion of mask [h][w] (float; neighbours outside
 * the image ignored, kornia's default border) is > 0 there.  sel (device int[M]) receives the kept m in ascending
 * order, *count (device int) their number; when none is kept, sel = 0..M-1 and *count = M (:462-463). */
int l4p_seg_query_select(l4p_stream stream, const float* mask, int h, int w, const int* cells, int M, int* sel, int* count);

/* ------------------------------------------------------------------------------------------------
 * L4PDataset base class: ground-truth clips (l4p/data/l4p_dataset_mini.py:126-395, 499-519, 576-580).  Raw float32
 * tensors of one sample in HBM -> the sample dict's tensors, three launches (csrc/gt_prep.hip).  The file is built
 * without floating-point contraction: every operation named below rounds on its own, as the reference's separate
 * torch operations do.
 * ------------------------------------------------------------------------------------------------ */

#define L4P_GT_MAX_FIELDS 10
#define L4P_GT_NEAREST 0
#define L4P_GT_BILINEAR 1

/* One dense field of a sample (rgb_b3thw, depth_b1thw, the flows, the masks and their valid masks). */
typedef struct l4p_gt_field {
    const float* src;      /* device [channels][T0][H][W] */
    const float* src_swap; /* flow fields: the opposite direction's tensor (same layout), read where the frame table's
                            * swap flag is 1 (mirror_and_pad, :132-162); NULL for every other field (the flag is ignored) */
    float* out;            /* device [channels][Tn][Hn][Wn] */
    int channels;          /* 1..3 */
    int mode;              /* L4P_GT_NEAREST: F.interpolate(mode="nearest"), :266; L4P_GT_BILINEAR: mode="trilinear" with
                            * the frame count unchanged = bilinear per frame, w0 * v0 + w1 * v1 per axis (ATen's order), then
                            * 1 * v + 0 * v for the time axis (ATen copies an axis of unchanged size with weights (1, 0) on one
                            * index: finite values pass, inf becomes nan) */
    int apply_scale;       /* 1: multiply channel c by scale[c] after the interpolation (:267-269, flow u by
                            * float32(res_w / W), flow v by float32(res_h / H)) */
    int normalize;         /* 1: then (x - mean[c]) / stdv[c], IEEE subtract and divide (:576-580, rgb) */
    float scale[3];
    float mean[3];
    float stdv[3];
} l4p_gt_field;

/* Every dense field of one sample in one launch, parallel over (field, channel, frame) x pixel tiles.  fields: HOST
 * array, copied into the kernel arguments at call time.  All sources are [channels][T0][H][W].
 * frame_table: device int[Tn][2] = (source frame, swap flag) of every output frame: mirror_and_pad (:126-190)
 * iterated as :558-560 iterates it, or repeat_single_frame (:192-235), with the temporal crop (:337) applied; the
 * swap flag is the flow-direction parity of the mirror rounds.
 * ynear / xnear: device int[Hn] / int[Wn], l4p_torch_nearest_table with the crop offset folded in (identity + offset
 * when the reference skips the resize, :247-248).  yi0, yi1, ylam / xi0, xi1, xlam: device tables of
 * l4p_resize_index_table for the bilinear fields (for an axis of unchanged size the caller passes i1 = i0, lambda = 0, ATen's
 * rule for such an axis); may be NULL when no field is bilinear.
 * A frame or table entry outside the source writes NaN, never reads out of range. */
int l4p_gt_dense_clip(l4p_stream stream, const l4p_gt_field* fields, int n_fields, int T0, int H, int W,
                      const int* frame_table, const int* ynear, const int* xnear, const int* yi0, const int* yi1,
                      const float* ylam, const int* xi0, const int* xi1, const float* xlam, int Tn, int Hn, int Wn);

/* The bounds filter of crop (:356-365): query n of queries (device float [N][3] = t, x, y) is kept iff
 * t0 < q_t < t0 + Tn, j0 < q_x < j0 + Wn and i0 < q_y < i0 + Hn (strict float32 compares against the integer bounds).
 * sel (device int[N]) receives the kept n in ascending order, *count (device int) their number - the 4 bytes the
 * host reads back.  One workgroup.  scale_queries = 1 (this engine's scale_queries_on_resize extension): q_x and q_y are
 * first multiplied by fw = float32(res_w / W) and fh = float32(res_h / H). */
int l4p_gt_query_select(l4p_stream stream, const float* queries, int N, int t0, int Tn, int i0, int Hn, int j0, int Wn,
                        int scale_queries, float fw, float fh, int* sel, int* count);

/* The track tensors of the M kept rows (sel: device int[M], NULL = rows 0..M-1; frame_table as above, no swap):
 *   gather through sel and the frame table (:175-186, :347, :365-374);
 *   scale_traj = 1: x *= fw, y *= fh (:270-272);
 *   cropped = 1 (0: the crop was a no-op and the reference returned at :308-309): x -= j0, y -= i0 (:377-379);
 *     vis cleared where x >= Wn, x < 0, y >= Hn or y < 0 (:381-384); queries -= (t0, j0, i0) (:390-393);
 *   causal = 1: valid &= (t + 0.5 >= q_t), causal = -1: valid &= (t + 0.5 <= q_t), 0: unchanged (:499-519).
 * traj [N][2][T0] -> traj_out [M][2][Tn]; vis / valid: uint8 [N][T0] -> [M][Tn] (bool tensors cross as uint8);
 * depth [N][T0] -> depth_out [M][Tn], both NULL when the sample has no track depth; queries [N][3] -> queries_out
 * [M][3]; labels [N] -> labels_out [M].  M == 0 launches nothing. */
int l4p_gt_tracks_clip(l4p_stream stream, const float* traj, const unsigned char* vis, const unsigned char* valid,
                       const float* depth, const float* queries, const float* labels, int N, int T0, const int* sel, int M,
                       const int* frame_table, int Tn, int scale_traj, int scale_queries, float fw, float fh, int cropped,
                       int t0, int i0, int j0, int Hn, int Wn, int causal, float* traj_out, unsigned char* vis_out,
                       unsigned char* valid_out, float* depth_out, float* queries_out, float* labels_out);

#ifdef __cplusplus
}
#endif
#endif /* L4P_HIP_H */
