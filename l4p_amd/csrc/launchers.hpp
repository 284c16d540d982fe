// Every launch_* that one translation unit of libl4p_hip.so defines and another calls, declared once (launch_gemm / launch_gemm_group:
// gemm.hpp, beside GemmParams).  The defining files include this header too, so a definition that drifts from its declaration is a
// compile error or - a new overload - an undefined symbol at the link (-Wl,--no-undefined), not at the first import.  Default
// arguments appear here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include "attn_select.hpp"
#include "ln_select.hpp"
#include "track_select.hpp"

// elementwise.hip
int launch_layernorm(int dtype, const LnParams& p, hipStream_t stream);
int launch_cast(int dtype, const float* x, void* y, long long n, hipStream_t stream);
int launch_patch_gather(int dtype, const float* rgb, void* out, int B, int Cin, int T, int H, int W, int pt, int ph,
                        int pw, int Kp, hipStream_t stream);

// attention.hip: attn_select (attn_select.hpp) decides, launch_attn_form launches the form it names under one profiler tag
int launch_attention(int dtype, const void* q, const void* kt, const void* vt, void* out, int B, int S, int H, int Dh, float scale,
                     hipStream_t stream);
int launch_attn_form(int dtype, const AttnChoice& c, const void* q, const void* kt, const void* vt, void* out, int B, int S, int H, int Dh,
                     hipStream_t stream);
// attention64.hip: the ATTN_ROWS64 arm of launch_attn_form (16-bit dtype, Dh 88 / 64)
int launch_attn_rows64(int dtype, const AttnChoice& c, const void* q, const void* kt, const void* vt, void* out, int S, int H, int Dh,
                       hipStream_t stream);

// dpt_ops.hip
int launch_upsample(int dtype, const void* x, void* y, int B, int Ti, int Hi, int Wi, int To, int Ho, int Wo, int C,
                    int align, hipStream_t stream);
int launch_head_out(int dtype, const void* x, const float* w, const float* bias, float* y, long long vox_per_b, int B,
                    int C, int Cout, int post_exp, hipStream_t stream);

// geom.hip
int launch_affine_solve(const float* pred, const float* tgt, long long n, int inverse, double* scratch, float* sol,
                        hipStream_t stream);
int launch_affine_apply(const float* x, float* y, long long n, int inverse, const float* sol, hipStream_t stream);
int launch_rays_to_pose_rot(const float* rays, const float* R, float* out, int B, int T, int h, int w, hipStream_t stream);
int launch_rays_to_pose(const float* rays, const float* K, float* out, int B, int T, int h, int w, int H, int W,
                        hipStream_t stream);

// track.hip: the tracker's kernels but its output tail.  A launcher that chooses anything calls its *_select (track_select.hpp: form,
// grid, block, LDS size - pure, checked on the host), refuses with the selection's text, and launches the form it names
static inline dim3 grid_of(const TrackChoice& c) { return dim3(c.gx, c.gy, c.gz); }
int launch_track_tokens(const float* queries, const float* labels, const float* pfeat, const float* plabel,
                        const float* gauss, const float* mask_tokens, const float* pe0, const float* pe1,
                        const float* nap, const float* fe0, const float* fe1, float* tokens, int N, int C, int T, int H,
                        int W, hipStream_t stream, int dtype = 0, void* tokens_T = nullptr);
int launch_track_keys_init(int dtype, const float* enc, const float* hist, const float* pos, float* k32, void* kT,
                           void* kP, int N, int P, int C, int shared_from, float* k32_shared, hipStream_t stream);
int launch_fill_rows(float* out, const float* v, long long rows, int C, long long group_rows, long long group_stride,
                     long long group_off, hipStream_t stream);
int launch_broadcast_block(void* base, long long off, long long bytes, long long stride, int n, hipStream_t stream);
int launch_small_attn(int dtype, int kind, const void* q, const void* k, const void* v, void* out, int N, int P, int D,
                      int heads, hipStream_t stream);
int launch_i2t_probs(int dtype, const float* s, long long lds_, int pairs, const float* cbias, int rows_per_group, void* p, int ldp,
                     long long M, int heads, int tokens, hipStream_t stream);
int launch_split_hilo(int dtype, const float* in, void* out, int G, int R, long long C, hipStream_t stream);
int launch_t2i_attn_scores(int dtype, const float* scores, long long ld_scores, const void* v, void* out, int N, int P, int D, int heads,
                           hipStream_t stream);
int launch_transpose_pad(int dtype, const void* in, void* out, int G, int R, int C, int Rp, hipStream_t stream);
int launch_i2t_delta(int dtype, const void* probs, const void* vt, const float* bias, void* delta, int N, int P, int C, int K,
                     hipStream_t stream);
int launch_t2i_probs(int dtype, const float* scores, long long ld_scores, void* probs, float* stats, int N, int P, int HT, hipStream_t stream);
int launch_t2i_context(int dtype, const void* probs, const float* stats, const void* keys, void* ctx, int N, int P, int C, int heads,
                       int tokens, long long Rg, int shared_from, hipStream_t stream);
int launch_track_prepare(const float* cur_q, const float* orig_q, int start, int ws, float* q_off, float* labels,
                         unsigned char* valid_t, unsigned char* valid_n, int N, hipStream_t stream);
int launch_track_commit(const float* w_traj, const float* w_vis, const float* w_depth, const unsigned char* valid_t,
                        const unsigned char* valid_n, float* traj, float* vis, float* depth, int T, int start, int ws,
                        int next_start, int last_window, float* cur_q, float* plabel, const float* new_pfeat, float* pfeat,
                        int* best_out, int N, int C, hipStream_t stream);

// track_readout.hip: the tracker's output tail - hyper-network mask product (LDS-staged or direct: mask_product_select), gather of the
// mask up-scaling's partial sums, fused read-out (1024-thread or column form, or the LDS refusal: track_readout_select)
int launch_mask_product(int dtype, const void* up, const float* hyper, float* masks, int N, long long vox, int Cc,
                        hipStream_t stream);
int launch_mask_gather(const float* partial, float* masks, int N, int T, int h, int w, int cpt, hipStream_t stream);
int launch_track_readout(const float* masks, float* traj, float* vis, float* depth, int N, int T, int h, int w, int H,
                         int W, hipStream_t stream);
