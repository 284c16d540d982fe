// HBM-bound kernels of the encoder path: LayerNorm, tubelet im2col (patch embed gather), casts.
// All are one-pass, 16-byte vectorised, one wave per row where a row reduction is needed.
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "launchers.hpp"

// ---------------------------------------------------------------------------------------------
// LayerNorm over the last dim of a float [M][C] residual stream (reference: nn.LayerNorm eps=1e-6
// in the encoder, l4p_videomae.py:177; eps=1e-5 in the SAM two-way transformer, transformer.py:145-153;
// LayerNorm3d over channels, mask_decoder.py:145-157 == the same row LN in channels-last layout).
// Two-pass in registers (mean, then centred variance) like ATen.  ln_select.hpp: the parameters of a launch (LnParams) and which of
// the kernels below it gets; launch_layernorm at the end of this section starts it.
// ---------------------------------------------------------------------------------------------
// ---- what the forms share: the affine, a typed quad, the wave's row statistics, the tail ----
// y = (v - mean) * rstd * g + b, written ONCE: the chained key LayerNorm below re-derives another launch's float result from its
// inputs and stored statistics, bit for bit - both must round the same way whatever the compiler would contract in each context
__device__ __forceinline__ float ln_affine(float v, float mean, float rstd, float g, float b) {
    return __builtin_fmaf((v - mean) * rstd, g, b);
}
// where quad idx of a row of T lies (indexed as a quad, so that idx folds into the memory instruction's offset)
template <typename T>
__device__ __forceinline__ T* ln_quad_at(T* row, int idx) {
    return (T*)((typename Vec4<std::remove_const_t<T>>::raw_t*)row + idx);
}
// quad idx of a row stored as T, as floats; zero when it lies outside the row (branch-free: the load is clamped, not predicated, so
// all slots of a lane are requested at once)
template <typename T>
__device__ __forceinline__ f32x4 ln_quad(const T* row, int idx, bool in) {
    float t[4];
    Vec4<T>::load(ln_quad_at(row, in ? idx : 0), t);
    return (f32x4){in ? t[0] : 0.f, in ? t[1] : 0.f, in ? t[2] : 0.f, in ? t[3] : 0.f};
}
// (mean, rstd) of the row a wave holds as v[i] = quad lane + 64 i (zero outside the row): slot sums in slot order, the xor butterfly,
// then the centred squares.  A macro, not a function: behind a call boundary the compiler moved the variance blocks out of line
// (taken branches in every wave; the encoder's residual LayerNorm measured 27.3 -> 28.3 us).  It declares `mean` and `rstd` in the
// caller's scope.  (Tried: a __forceinline__ function taking the array by reference.  Not tried: a lambda, the array in a struct.)
#define LN_WAVE_STATS(v, MAXV, lane, nv, C, eps, mean, rstd)                                                                        \
    float mean, rstd;                                                                                                               \
    {                                                                                                                               \
        float s_ = 0.f;                                                                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < MAXV; ++i_) s_ += v[i_][0] + v[i_][1] + v[i_][2] + v[i_][3];                        \
        mean = wave_sum(s_) / (float)C;                                                                                             \
        float q_ = 0.f;                                                                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < MAXV; ++i_) {                                                                       \
            if (lane + i_ * 64 < nv) {                                                                                              \
                _Pragma("unroll") for (int k_ = 0; k_ < 4; ++k_) {                                                                  \
                    const float d_ = v[i_][k_] - mean;                                                                              \
                    { /* (product rounded, then added - never contracted: the chained LayerNorm must round like the plain one in  \
                          every instantiation; left to the compiler the f32 kernels fused it and the bf16 ones did not) */         \
                        _Pragma("clang fp contract(off)") q_ += d_ * d_;                                                            \
                    }                                                                                                               \
                }                                                                                                                   \
            }                                                                                                                       \
        }                                                                                                                           \
        rstd = rsqrtf(wave_sum(q_) / (float)C + eps);                                                                               \
    }
// Quad idx of the row that starts at element `row_at`: y = affine (+ GELU) of v, then every output that is given - T(y + add), y as
// float, the float row itself (the residual sum), y as T
template <typename T>
__device__ __forceinline__ void ln_finish(f32x4 v, float mean, float rstd, f32x4 g, f32x4 b, int act, f32x4 add, long long row_at, int idx,
                                          T* out_T2, float* out_f32, float* out_sum, T* out_T) {
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = ln_affine(v[k], mean, rstd, g[k], b[k]);
    if (act == L4P_ACT_GELU) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = gelu_for<T>(y[k]);
    }
    if (out_T2) {
        f32x4 y2;
#pragma unroll
        for (int k = 0; k < 4; ++k) y2[k] = y[k] + add[k];
        Vec4<T>::store(ln_quad_at(out_T2 + row_at, idx), (const float*)&y2);
    }
    if (out_f32) ((f32x4*)(out_f32 + row_at))[idx] = y;
    if (out_sum) ((f32x4*)(out_sum + row_at))[idx] = v;
    if (out_T) Vec4<T>::store(ln_quad_at(out_T + row_at, idx), (const float*)&y);
}

// One wave per row, MAXV float4 slots per lane.
// XT: the input row is stored as T (the bf16 engine's activations) instead of float - half the bytes in; it may alias
// out_T (a wave holds its row in registers before it stores anything).
// (More rows per wave, all requested before the first is reduced, measured on the 1M x 352 LayerNorm + GELU of the tracker: 1 row
//  556 us, 2 rows 696 us, 4 rows 889 us - that launch is VALU-bound (GELU on 369 M elements), not latency-bound.)
// RES: the row normalised is x[row % x_mod] + delta[row] (delta in the engine dtype): the tracker's "keys += attention
// output; keys = LayerNorm(keys)" (sam/transformer.py:183-185) with the sum formed HERE instead of in the projection's
// epilogue - the float key stream is read once by this kernel instead of read + written by the GEMM and read again.
// out_sum (may alias x when x_mod = 0): the float sum itself - the encoder's pre-norm residual stream, where y is only the next
// linear's input.  PART: the addend is pbias + nsplit float partials [nsplit][M][C] of a split-K projection instead of delta.
template <typename T, int MAXV, bool XT = false, bool RES = false, bool PART = false>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, T* out_T, float* out_f32, int M,
                                                        int C, const float* __restrict__ add, int add_mod, T* out_T2, int act,
                                                        const T* __restrict__ delta, int x_mod, const float* __restrict__ x_shared,
                                                        int x_period, int x_split, float* out_sum, const float* __restrict__ part,
                                                        int nsplit, const float* __restrict__ pbias, float* __restrict__ out_stats) {
    // (x and the outputs are NOT restrict-qualified: the tracker normalises its key stream and the up-scaled activation in
    //  place; a wave has its whole row in registers - every store depends on the row statistics - before it writes)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = C >> 2;
    // every load of the row is issued up front (x, gamma, beta, the optional addend): ONE exposed memory round trip per
    // wave instead of three dependent ones (x -> statistics -> gamma/beta/add) - the kernel is latency-, not bandwidth-bound
    f32x4 v[MAXV], g[MAXV], bb[MAXV], av[MAXV];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    // (RES, x_shared: rows p = row % x_period >= x_split come from the shared set x_shared[p - x_split] - the part of the
    //  tracker's key stream that is still the same for every track)
    const int prow = RES && x_shared ? row % x_period : 0;
    const f32x4* xr = RES && x_shared && prow >= x_split ? (const f32x4*)(x_shared + (long long)(prow - x_split) * C)
                                                         : (const f32x4*)(x + (long long)(RES && x_mod > 0 ? row % x_mod : row) * C);
    const f32x4* ar = out_T2 ? (const f32x4*)(add + (long long)(row % add_mod) * C) : nullptr;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        const bool in = idx < nv;
        if constexpr (XT)
            v[i] = ln_quad((const T*)x + (long long)row * C, idx, in);
        else
            v[i] = in ? xr[idx] : z;
        if constexpr (PART) {  // the addend is bias + the float partials of a split-K projection, summed in slice order
            f32x4 d = pbias ? ((const f32x4*)pbias)[in ? idx : 0] : z;
            // (four slices requested at a time - a slice past the last is a clamped duplicate that is not added: with a plain
            //  loop over a run-time nsplit every slice was its own memory round trip, 24 in a row per lane at batch 1)
            for (int sl = 0; sl < nsplit; sl += 4) {
                f32x4 t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int su = sl + u < nsplit ? sl + u : sl;
                    t[u] = ((const f32x4*)(part + ((long long)su * M + row) * C))[in ? idx : 0];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (sl + u < nsplit) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) d[k] += t[u][k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[i][k] += in ? d[k] : 0.f;
        } else if constexpr (RES) {
            const f32x4 d = ln_quad(delta + (long long)row * C, idx, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[i][k] += d[k];
        }
        av[i] = (in && ar) ? ar[idx] : z;
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        const bool in = idx < nv;
        g[i] = in ? ((const f32x4*)gamma)[idx] : z;
        bb[i] = in ? ((const f32x4*)beta)[idx] : z;
    }
    LN_WAVE_STATS(v, MAXV, lane, nv, C, eps, mean, rstd)
    if constexpr (RES) {  // (mean, rstd) of the row: what the chained forms re-derive this launch's float result from
        if (out_stats && lane == 0) {
            out_stats[2ll * row] = mean;
            out_stats[2ll * row + 1] = rstd;
        }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        // (RES, out_sum: the pre-norm residual stream of the encoder - the SUM x + delta is what lives on, y is only xn)
        if (idx < nv) ln_finish<T>(v[i], mean, rstd, g[i], bb[i], act, av[i], (long long)row * C, idx, out_T2, out_f32, RES ? out_sum : nullptr, out_T);
    }
}

// Chained key LayerNorm (the tracker's second layer in a FIRST window, sam/transformer.py:183-185): the layer before normalised
// xs[row % x_mod] + dprev[row] - float rows common to all tracks plus that layer's update in the engine dtype - and stored only its
// engine-dtype outputs and (mean, rstd) per row.  Its float result, the residual this layer adds to, is re-derived here from those
// (ln_affine: bit for bit what it would have stored), so the float key master [N * P][C] is neither written nor read: 1.1 GB of
// 3.7 GB per 64 tracks.  One wave per row, every load of the row's operands issued before the first use, C <= 1536.  (Its own kernel
// beside layernorm_kernel<RES>: it holds two updates instead of one and so reads the four parameter vectors where it uses them.
// Folded into layernorm_kernel as a CHAIN parameter, with that kernel's up-front gamma / beta, it takes 154 (f16) and 178 (f32)
// registers against 106 and 128 here: 3 and 2 waves per SIMD instead of 4.)
template <typename T>
__global__ __launch_bounds__(256) void layernorm_chain_kernel(const float* __restrict__ xs, int x_mod, const T* __restrict__ dprev,
                                                              const float* __restrict__ stats, const float* __restrict__ g0,
                                                              const float* __restrict__ b0, const T* __restrict__ delta,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              T* __restrict__ out_T, float* __restrict__ out_f32, int M, int C,
                                                              const float* __restrict__ add, int add_mod, T* __restrict__ out_T2) {
    constexpr int MAXV = 6;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = C >> 2;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[MAXV], d1[MAXV], av[MAXV];
    const f32x4* xr = (const f32x4*)(xs + (long long)(row % x_mod) * C);
    const f32x4* ar = out_T2 ? (const f32x4*)(add + (long long)(row % add_mod) * C) : nullptr;
    const float mean0 = stats[2ll * row], rstd0 = stats[2ll * row + 1];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        const bool in = idx < nv;
        v[i] = in ? xr[idx] : z;
        const f32x4 t = ln_quad(dprev + (long long)row * C, idx, in);
        d1[i] = ln_quad(delta + (long long)row * C, idx, in);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] += t[k];
        av[i] = (in && ar) ? ar[idx] : z;
    }
    // the previous layer's float result (its out_f32, had it stored one) + this layer's update
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        if (idx < nv) {
            const f32x4 gg = ((const f32x4*)g0)[idx], bb = ((const f32x4*)b0)[idx];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[i][k] = ln_affine(v[i][k], mean0, rstd0, gg[k], bb[k]) + d1[i][k];
        } else {
            v[i] = z;
        }
    }
    LN_WAVE_STATS(v, MAXV, lane, nv, C, eps, mean, rstd)
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        if (idx < nv)
            ln_finish<T>(v[i], mean, rstd, ((const f32x4*)gamma)[idx], ((const f32x4*)beta)[idx], L4P_ACT_NONE, av[i], (long long)row * C, idx,
                         out_T2, out_f32, nullptr, out_T);
    }
}
// ---------------------------------------------------------------------------------------------
// The two key LayerNorms of a FIRST window again (layer 0: layernorm_kernel<RES> with every float row shared; layer 1:
// layernorm_chain_kernel), with the work laid out by TOKEN instead of by row (round 5).  In the row kernels a wave reads, beside
// the 5.6 - 11 KB that belong to its (track, token) row, the token's shared float key row and positional row (11 KB, from L2 /
// the Infinity Cache: the 2 x 11.5 MB sets do not fit the 4 MB L2) and two or four parameter vectors (11 - 22 KB through the
// vector L1): three to five times the unique bytes through the CU's 64 B/clk memory pipe.  tools/probes/stream_bw: the unique
// traffic alone streams in 183 / 250 us, with the two shared rows per row 301 / 371 us; the row kernels took 474 / 495 us.
// Here a wave owns ONE token p and walks tracks n0 .. n0 + nt - 1 of it (rows n * P + p): the shared rows are loaded ONCE into
// registers, the parameter vectors ONCE per workgroup into LDS, and the per-track operands of track n + 1 are requested before
// track n is reduced.  Per-row arithmetic is the row kernels' statement for statement (ln_affine, the uncontracted variance,
// the same summation order): bit-identical outputs (tests/test_track_gpu.py).
// This kernel is NOT written on the helpers above: on them (with either store order of the tail) the own-master form normalised in
// place was 0.7 % slower in three calls (262144 rows: 878.5 -> 885.0, 877.6 -> 882.9, 874.3 -> 880.9 us), so it keeps the body it
// had, and compiles to the same instructions as before.
// ---------------------------------------------------------------------------------------------
// XT (later windows, layernorm_kernel<RES> with x_mod = 0): the float rows are the tracks' own key master x_track[row] (normalised
// in place when out_f32 aliases it) - or, for tokens p >= x_split of a half-shared layer 0, still the common rows x_half[p - x_split]:
// a wave-uniform choice, its token decides.  Per-track float rows travel with the track's update.
template <typename T, bool CHAIN, bool XT = false>
__global__ __launch_bounds__(256) void key_ln_tracks_kernel(const float* xs, int P, const T* __restrict__ dprev,
                                                            const float* __restrict__ stats_in, const float* __restrict__ g0,
                                                            const float* __restrict__ b0, const T* __restrict__ delta,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            T* __restrict__ out_T, float* out_f32, int N, int C,
                                                            const float* __restrict__ add, T* __restrict__ out_T2,
                                                            float* __restrict__ out_stats, int tpw, const float* x_track = nullptr,
                                                            const float* __restrict__ x_half = nullptr, int x_split = 0) {
    static_assert(!(CHAIN && XT), "the chained form exists for first windows only");
    constexpr int MAXV = 6;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [gamma | beta | g0 | b0][C] floats
    f32x4* const sp = (f32x4*)smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = C >> 2;
    const int ptiles = P >> 2;
    const int p = ((int)blockIdx.x % ptiles) * 4 + wave;
    const int n0 = ((int)blockIdx.x / ptiles) * tpw;
    const int n1 = n0 + tpw < N ? n0 + tpw : N;
    for (int i = threadIdx.x; i < nv; i += 256) {
        sp[i] = ((const f32x4*)gamma)[i];
        sp[nv + i] = ((const f32x4*)beta)[i];
        if constexpr (CHAIN) {
            sp[2 * nv + i] = ((const f32x4*)g0)[i];
            sp[3 * nv + i] = ((const f32x4*)b0)[i];
        }
    }
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 xv[MAXV], av[MAXV];
    typedef typename std::conditional<sizeof(T) == 2, vec4h<T>, f32x4>::type op_t;
    op_t dp[MAXV], dl[MAXV];
    float mean0 = 0.f, rstd0 = 0.f;
    const float* xsrc = XT ? (x_half && p >= x_split ? x_half + (long long)(p - x_split) * C : nullptr) : xs + (long long)p * C;
    const bool per_track = XT && xsrc == nullptr;  // (wave-uniform)
    const f32x4* xr = (const f32x4*)xsrc;
    const f32x4* ar = (const f32x4*)(add + (long long)p * C);
    auto request = [&](int n, op_t* dpv, op_t* dlv, float& m0, float& r0) {
        const long long row = (long long)n * P + p;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int idx = lane + i * 64;
            const int ci = idx < nv ? idx : 0;
            if constexpr (CHAIN) dpv[i] = ((const op_t*)(dprev + row * C))[ci];
            dlv[i] = ((const op_t*)(delta + row * C))[ci];
            if constexpr (XT) {
                if (per_track) xv[i] = idx < nv ? ((const f32x4*)(x_track + row * C))[idx] : z;
            }
        }
        if constexpr (CHAIN) m0 = stats_in[2 * row], r0 = stats_in[2 * row + 1];
    };
    request(n0, dp, dl, mean0, rstd0);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int idx = lane + i * 64;
        if (!per_track) xv[i] = idx < nv ? xr[idx] : z;
        av[i] = idx < nv ? ar[idx] : z;
    }
    __syncthreads();
    for (int n = n0; n < n1; ++n) {
        const long long row = (long long)n * P + p;
        f32x4 v[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int idx = lane + i * 64;
            const bool in = idx < nv;
            if constexpr (CHAIN) {
                // the previous layer's float result (x + its update, normalised with the stored statistics) + this layer's update
                f32x4 t = xv[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] += in ? (float)dp[i][k] : 0.f;
                if (in) {
                    const f32x4 gg = sp[2 * nv + idx], bb = sp[3 * nv + idx];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[i][k] = ln_affine(t[k], mean0, rstd0, gg[k], bb[k]) + (float)dl[i][k];
                } else {
                    v[i] = z;
                }
            } else {
                v[i] = xv[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[i][k] += in ? (float)dl[i][k] : 0.f;
            }
        }
        // (the operand registers are free once the row is formed: the next track's operands travel under this track's
        //  reductions and stores)
        if (n + 1 < n1) request(n + 1, dp, dl, mean0, rstd0);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            if (lane + i * 64 < nv) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = v[i][k] - mean;
                    {
#pragma clang fp contract(off)
                        q += d * d;
                    }
                }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
        if constexpr (!CHAIN) {
            if (out_stats && lane == 0) {
                out_stats[2 * row] = mean;
                out_stats[2 * row + 1] = rstd;
            }
        }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int idx = lane + i * 64;
            if (idx < nv) {
                const f32x4 gg = sp[idx], bb = sp[nv + idx];
                f32x4 y;
#pragma unroll
                for (int k = 0; k < 4; ++k) y[k] = ln_affine(v[i][k], mean, rstd, gg[k], bb[k]);
                if (out_f32) ((f32x4*)(out_f32 + row * C))[idx] = y;
                if (sizeof(T) == 2) {
                    vec4h<T> o, o2;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = (vec4e<T>)y[k], o2[k] = (vec4e<T>)(y[k] + av[i][k]);
                    ((vec4h<T>*)((vec4e<T>*)out_T + row * C))[idx] = o;
                    ((vec4h<T>*)((vec4e<T>*)out_T2 + row * C))[idx] = o2;
                } else {
                    ((f32x4*)((float*)out_T + row * C))[idx] = y;
                    f32x4 o2;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o2[k] = y[k] + av[i][k];
                    ((f32x4*)((float*)out_T2 + row * C))[idx] = o2;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm (+ GELU) of SHORT rows stored in the engine dtype, C <= 512 (round 5): the tracker's LayerNorm3d after its first
// up-scaling, [N * 8 P][352] in place.  One wave per row leaves 20 of 64 lanes idle in the second slot of a 352-wide row, pays
// two 6-step wave reductions per row and reads gamma / beta (2.8 KB) through the L1 for every 1.4 KB row.  Here a row belongs to
// ONE DPP ROW of 16 lanes (lane k holds the quads k, k + 16, ...: 88 quads = 5.5 slots, 92 % of the lanes busy), the statistics are
// two 4-step rotations inside the DPP row, a wave works on 4 rows at a time and walks RPW / 4 such groups with gamma / beta in
// registers, the next group's rows requested as soon as the current ones are converted.  Row sums are formed in a different
// order than layernorm_kernel's (and the variance product is left to the compiler to contract): equal to it to float rounding, not
// bit for bit - the statistics stay this kernel's own.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float row16_sum(float v) {
    // rotations inside a row of 16 lanes: every lane ends with the row's sum (same order in every lane's view up to rotation)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
    return v;
}
template <typename T, int SLOTS, int RPW>
__global__ __launch_bounds__(256) void ln_rows16_kernel(const T* x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        T* out, long long M, int C, int act) {
    static_assert(sizeof(T) == 2 && RPW % 4 == 0, "16-bit rows, four at a time");
    const int lane = threadIdx.x & 63, k = lane & 15, sub = lane >> 4;
    const int nv = C >> 2;
    const long long row_base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    if (row_base >= M) return;
    f32x4 g[SLOTS], bb[SLOTS];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int q = k + 16 * j;
        g[j] = q < nv ? ((const f32x4*)gamma)[q] : z;
        bb[j] = q < nv ? ((const f32x4*)beta)[q] : z;
    }
    typedef typename Vec4<T>::raw_t raw_t;
    raw_t raw[SLOTS];
    auto request = [&](long long row) {
        const long long rr = row < M ? row : M - 1;  // (a clamped duplicate row is loaded but never stored)
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int q = k + 16 * j;
            raw[j] = ((const raw_t*)(x + rr * C))[q < nv ? q : 0];
        }
    };
    request(row_base + sub);
    for (int it = 0; it < RPW / 4; ++it) {
        const long long row = row_base + 4 * it + sub;
        f32x4 v[SLOTS];
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const bool in = k + 16 * j < nv;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = in ? (float)raw[j][e] : 0.f;
        }
        if (it + 1 < RPW / 4 && row_base + 4 * (it + 1) < M) request(row + 4);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) s += v[j][0] + v[j][1] + v[j][2] + v[j][3];
        const float mean = row16_sum(s) / (float)C;
        float qq = 0.f;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            if (k + 16 * j < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = v[j][e] - mean;
                    qq += d * d;
                }
            }
        }
        const float rstd = rsqrtf(row16_sum(qq) / (float)C + eps);
        if (row < M) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int q = k + 16 * j;
                if (q < nv) {
                    float o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        o[e] = ln_affine(v[j][e], mean, rstd, g[j][e], bb[j][e]);
                        if (act == L4P_ACT_GELU) o[e] = gelu_for<T>(o[e]);
                    }
                    Vec4<T>::store(ln_quad_at(out + row * C, q), o);
                }
            }
        }
    }
}

// ---- the one launcher: ln_select names the form, this starts it ----
template <typename T, int MAXV, bool XT, bool RES, bool PART>
static void launch_ln_row(const LnParams& p, hipStream_t stream) {
    hipLaunchKernelGGL((layernorm_kernel<T, MAXV, XT, RES, PART>), dim3((p.M + 3) / 4), dim3(256), 0, stream, (const float*)p.x, p.gamma, p.beta,
                       p.eps, (T*)p.out_T, p.out_f32, p.M, p.C, p.add, p.add_mod, (T*)p.out_T2, p.act, (const T*)p.delta_T, p.x_mod, p.x_shared,
                       p.x_period, p.x_split, p.out_sum, p.part, p.nsplit, p.pbias, p.out_stats);
}
template <typename T, bool XT, bool RES, bool PART>
static void launch_ln_row_slots(int slots, const LnParams& p, hipStream_t stream) {
    if (slots == 2) return launch_ln_row<T, 2, XT, RES, PART>(p, stream);
    if (RES || slots == 6) return launch_ln_row<T, 6, XT, RES, PART>(p, stream);
    if constexpr (!RES) launch_ln_row<T, 8, XT, RES, PART>(p, stream);
}
template <typename T, bool CHAIN, bool XT>
static void launch_ln_tokens(const LnParams& p, hipStream_t stream) {
    // tracks per wave: 8 (4096 workgroups for 64 tracks of 2048 tokens; 4 / 8 / 16 measure the same: c3 LayerNorm class 6.38 / 6.38 / 6.41 ms)
    const int P = p.add_mod, N = p.M / P, tpw = N < 8 ? N : 8;
    const dim3 grid((P / 4) * ((N + tpw - 1) / tpw));
    hipLaunchKernelGGL((key_ln_tracks_kernel<T, CHAIN, XT>), grid, dim3(256), (size_t)(CHAIN ? 4 : 2) * p.C * sizeof(float), stream,
                       XT ? nullptr : (const float*)p.x, P, (const T*)p.dprev_T, p.stats_in, p.g0, p.b0, (const T*)p.delta_T, p.gamma, p.beta, p.eps,
                       (T*)p.out_T, p.out_f32, N, p.C, p.add, (T*)p.out_T2, p.out_stats, tpw, XT ? (const float*)p.x : nullptr, p.x_shared, p.x_split);
}
template <typename T>
static int launch_ln_form(LnChoice c, const LnParams& p, hipStream_t stream) {
    switch (c.form) {
        case LN_ROW: launch_ln_row_slots<T, false, false, false>(c.slots, p, stream); return 0;
        case LN_ROW_RES: launch_ln_row_slots<T, false, true, false>(c.slots, p, stream); return 0;
        case LN_ROW_PART: launch_ln_row_slots<T, false, true, true>(c.slots, p, stream); return 0;
        case LN_ROW_CHAIN:
            hipLaunchKernelGGL(layernorm_chain_kernel<T>, dim3((p.M + 3) / 4), dim3(256), 0, stream, (const float*)p.x, p.x_mod, (const T*)p.dprev_T,
                               p.stats_in, p.g0, p.b0, (const T*)p.delta_T, p.gamma, p.beta, p.eps, (T*)p.out_T, p.out_f32, p.M, p.C, p.add, p.add_mod,
                               (T*)p.out_T2);
            return 0;
        case LN_TOKEN_SHARED: launch_ln_tokens<T, false, false>(p, stream); return 0;
        case LN_TOKEN_OWN: launch_ln_tokens<T, false, true>(p, stream); return 0;
        case LN_TOKEN_CHAIN: launch_ln_tokens<T, true, false>(p, stream); return 0;
        case LN_ROW_T:  // rows stored in the engine dtype: the 16-bit types only
            if constexpr (sizeof(T) == 2) {
                launch_ln_row_slots<T, true, false, false>(c.slots, p, stream);
                return 0;
            }
            break;
        case LN_ROWS16:
            if constexpr (sizeof(T) == 2) {
                constexpr int RPW = 16;
                const dim3 grid16((unsigned)(((long long)p.M + 4 * RPW - 1) / (4 * RPW)));
                auto kern = c.slots == 6 ? ln_rows16_kernel<T, 6, RPW> : ln_rows16_kernel<T, 8, RPW>;
                hipLaunchKernelGGL(kern, grid16, dim3(256), 0, stream, (const T*)p.x, p.gamma, p.beta, p.eps, (T*)p.out_T, (long long)p.M, p.C, p.act);
                return 0;
            }
            break;
        default: break;
    }
    l4p_set_error("layernorm: no kernel for form %d of dtype %d", (int)c.form, (int)sizeof(T));
    return L4P_E_INVALID;
}
// (the tags key the committed per-shape profiles: they name the entry, not the form)
static ProfScope ln_prof(LnForm form, hipStream_t stream, const LnParams& p) {
    switch (form) {
        case LN_ROW:
            return ProfScope(PROF_LAYERNORM, stream, "M%d C%d add%d T2%d act%d f32%d", p.M, p.C, p.add != nullptr, p.out_T2 != nullptr, p.act,
                             p.out_f32 != nullptr);
        case LN_ROW_T:
        case LN_ROWS16: return ProfScope(PROF_LAYERNORM, stream, "M%d C%d inT act%d", p.M, p.C, p.act);
        case LN_ROW_CHAIN:
        case LN_TOKEN_CHAIN: return ProfScope(PROF_LAYERNORM, stream, "M%d C%d chain T2%d f32%d", p.M, p.C, p.out_T2 != nullptr, p.out_f32 != nullptr);
        default: return ProfScope(PROF_LAYERNORM, stream, "M%d C%d res T2%d f32%d", p.M, p.C, p.out_T2 != nullptr, p.out_f32 != nullptr);
    }
}

int launch_layernorm(int dtype, const LnParams& p_in, hipStream_t stream) {
    LnParams p = p_in;
    if (p.kind == LN_ROWS && p.x_is_T) p.out_f32 = nullptr, p.add = nullptr, p.add_mod = 0, p.out_T2 = nullptr;  // (out_T and act only)
    if (p.kind != LN_ROWS) p.act = L4P_ACT_NONE;
    const char* err = nullptr;
    const LnChoice c = ln_select(dtype, p, LnKnobs{knob(KNOB_LN_TRACKS), knob(KNOB_LN_ROWS16)}, &err);
    if (c.form == LN_FORM_INVALID) {
        l4p_set_error(err, p.C);
        return L4P_E_INVALID;
    }
    ProfScope prof = ln_prof(c.form, stream, p);
    int rc = 0;
    L4P_WITH_T(dtype, T, rc = launch_ln_form<T>(c, p, stream));
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// float -> T cast (hook features handed to the DPT decoders), 16 bytes in per lane.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void cast_kernel(const float* __restrict__ x, T* __restrict__ y, long long n4) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 v = ((const f32x4*)x)[i];
        if (sizeof(T) == 2) {
            vec4h<T> o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (vec4e<T>)v[k];
            ((vec4h<T>*)y)[i] = o;
        } else {
            ((f32x4*)y)[i] = v;
        }
    }
}

int launch_cast(int dtype, const float* x, void* y, long long n, hipStream_t stream) {
    if (n % 4) {
        l4p_set_error("cast: n must be a multiple of 4");
        return L4P_E_INVALID;
    }
    const long long n4 = n / 4;
    const int grid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    ProfScope prof(PROF_ELEMENTWISE, stream, "cast");
    L4P_WITH_T(dtype, T, hipLaunchKernelGGL(cast_kernel<T>, dim3(grid), dim3(256), 0, stream, x, (T*)y, n4));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Tubelet gather for the patch-embed conv (reference PatchEmbed, modeling_finetune.py:269-283):
// Conv3d(3 -> C, kernel = stride = (pt, ph, pw)) == gather + GEMM.  Row = token (t', h', w')
// row-major, column k = ((c*pt + dt)*ph + dh)*pw + dw, zero-padded to Kp columns.
// rgb: [B][3][T][H][W] float.  One thread per output element; writes are fully coalesced, reads
// are pw-float runs that stay inside L2 (the whole clip is 9.6 MB).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void patch_gather_kernel(const float* __restrict__ rgb, T* __restrict__ out, int B, int Cin, int Tt, int Hh,
                                    int Ww, int pt, int ph, int pw, int Kp) {
    const int nT = Tt / pt, nH = Hh / ph, nW = Ww / pw;
    const int K = Cin * pt * ph * pw;
    const long long total = (long long)B * nT * nH * nW * Kp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kp);
        long long tok = i / Kp;
        float v = 0.f;
        if (k < K) {
            const int dw = k % pw;
            int r = k / pw;
            const int dh = r % ph;
            r /= ph;
            const int dt = r % pt;
            const int c = r / pt;
            const int w = (int)(tok % nW);
            long long r2 = tok / nW;
            const int hh = (int)(r2 % nH);
            r2 /= nH;
            const int t = (int)(r2 % nT);
            const int b = (int)(r2 / nT);
            v = rgb[((((long long)b * Cin + c) * Tt + (t * pt + dt)) * Hh + (hh * ph + dh)) * Ww + (w * pw + dw)];
        }
        out[i] = from_f32<T>(v);
    }
}

int launch_patch_gather(int dtype, const float* rgb, void* out, int B, int Cin, int T, int H, int W, int pt, int ph,
                        int pw, int Kp, hipStream_t stream) {
    if (T % pt || H % ph || W % pw || Kp < Cin * pt * ph * pw) {
        l4p_set_error("patch_gather: bad geometry");
        return L4P_E_INVALID;
    }
    const long long total = (long long)B * (T / pt) * (H / ph) * (W / pw) * Kp;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    ProfScope prof(PROF_ELEMENTWISE, stream, "patch_gather");
    L4P_WITH_T(dtype, TT, hipLaunchKernelGGL(patch_gather_kernel<TT>, dim3(grid), dim3(256), 0, stream, rgb, (TT*)out, B, Cin, T, H, W, pt, ph, pw,
                                             Kp));
    HIP_TRY(hipGetLastError());
    return 0;
}
