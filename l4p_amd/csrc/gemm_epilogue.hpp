// The epilogues of the GEMM / implicit-conv kernels (gemm.hpp, gemm8p.hpp, gemm4w.hpp, conv3_halo.hpp, gemm_skinny.hpp): what a lane
// does with its accumulators - bias, activation, residuals, the scatter forms (QKV tile order, ConvTranspose / sub-pixel pixel
// shuffle), the mask product - and the run-time choice between the generic row body and the lean specialisations.
// Included by gemm.hpp behind GemmParams and the EPI_* / ACT_* enums; not meant to be included on its own.
#pragma once
#include <type_traits>

#include "gemm_tile.hpp"
#include "static_for.hpp"

// ---- epilogue shared by every GEMM kernel: the lane (li, kg) owns rows m_wave0 + 16*i + li and the 4*TN consecutive
//      columns n_wave0 + 4*TN*kg + [0, 4*TN) of its wave's tile (acc[i][j][r] = column 4*TN*kg + 4*j + r) -------------
// One row (16*i + li) of the lane's tile: bias, activation, residuals, scatter / store.
template <typename T, int NV>
__device__ __forceinline__ void gemm_epilogue_row(const GemmParams& p, float (&v)[NV], const float (&bv)[NV],
                                                  const long long (&coff)[NV / 8], int m, int nb);

// L4P_EPI_MASKDOT epilogue (see include/l4p_hip.h): activated outputs x the three hyper-network vectors of the row's
// query, summed over the 32-column chunk the lane shares with 1 (NV = 16) or 3 (NV = 8) neighbours.  Kept apart from
// gemm_epilogue so that its 3 x NV hyper-vector registers never weigh on the ordinary epilogues.
// 16-bit engines, NV = 16 (the 8-phase / two-workgroup kernels' wave tile of 64 columns), GELU: the form the tracker runs a
// million rows through per clip.  Round 5: (1) the activation is compile time (the generic form tested p.act per VALUE: ~115
// scalar branches per 16-row block); (2) GELU is the clamped polynomial evaluated on PAIRS (v_pk_fma_f32: 7 issues per value
// against 13; the clamp is a bare v_med3_f32 - fmed3 through the compiler canonicalises its operand first, two more v_max per
// value); (3) the 3 x 64 dot products of a row with its query's hyper-network vectors are a matrix product and run on the matrix
// pipe: the activated row, rounded to T as the reference's autocast holds it (mask_decoder.py:136-139), IS an MFMA operand
// fragment - lane (row li, column group kg) holds 16 consecutive channels = two 8-element fragments under the k-slot map
// (kg, e) <-> channel 16 kg + e (+ 8) - and hyper^T [16 (3 used) x 64 channels] the other operand under the same map, so
// D = hyper^T x G^T leaves d0..d2 of row li in ONE lane (kg = 0) with no cross-lane sum.  The two 32-column chunks of the
// contract (include/l4p_hip.h) come from two products whose hyper operand is zeroed for the other chunk's lanes: 4 MFMAs
// 16x16x32 per 16 rows replace 48 FMAs + 6 lane exchanges per lane.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float med3_bare(float x, float lo, float hi) {
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "s"(hi));
    return r;
}
// gelu_poly (common.hpp) on NP pairs at once, coefficient by coefficient: a pair's Horner chain is serially dependent and a dependent
// packed op needs a wait state (one pair at a time the compiler emitted an s_nop behind each of its 12 packed ops); NP independent
// chains interleaved fill those slots.  xc = x clamped to [-4.5, 4.5].
template <int NP>
__device__ __forceinline__ void gelu_poly2(f32x2_t (&x)[NP], const f32x2_t (&xc)[NP]) {
    f32x2_t u[NP], q[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) u[k] = xc[k] * xc[k];
#pragma unroll
    for (int k = 0; k < NP; ++k) q[k] = __builtin_elementwise_fma((f32x2_t){-1.405532334e-12f, -1.405532334e-12f}, u[k], (f32x2_t){1.702386847e-10f, 1.702386847e-10f});
    constexpr float cf[8] = {-9.213366003e-09f, 2.962938120e-07f, -6.369978978e-06f, 9.790158587e-05f, -1.122762531e-03f, 9.833131509e-03f,
                             -6.633633733e-02f, 3.988829162e-01f};
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < NP; ++k) q[k] = __builtin_elementwise_fma(q[k], u[k], (f32x2_t){cf[c], cf[c]});
#pragma unroll
    for (int k = 0; k < NP; ++k) q[k] = __builtin_elementwise_fma(xc[k], q[k], (f32x2_t){0.5f, 0.5f});
#pragma unroll
    for (int k = 0; k < NP; ++k) x[k] = x[k] * q[k];
}
template <typename T, int TM>
__device__ __forceinline__ void gemm_epilogue_maskdot_mfma(const GemmParams& p, f32x4 (&acc)[TM][4], int m_wave0, int n_wave0, int li,
                                                           int kg) {
    static_assert(sizeof(T) == 2, "16-bit engines");
    if (n_wave0 >= p.N) return;  // (N % 64 == 0 is checked by the launcher: a wave's 64 columns are in or out together)
    const int nb = n_wave0 + 16 * kg;
    const int co = n_wave0 % p.Cout;  // first channel of the wave's 64 columns inside their tap (Cout % 64 == 0)
    f32x2_t bv[8];
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b4 = p.bias ? *(const f32x4*)(p.bias + nb + c) : z;
        bv[c / 2] = (f32x2_t){b4[0], b4[1]};
        bv[c / 2 + 1] = (f32x2_t){b4[2], b4[3]};
    }
    const float neg = -4.5f;
    int hq = -1;
    vec8<T> he[2], ho[2];  // hyper^T fragments (row h = li of hyper^T, channels co + 16 kg + 8 ks + e): chunk 0 (kg < 2) / chunk 1
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mb = m_wave0 + i * 16;  // (hyper_rows % 16 == 0, checked by the launcher: one query per 16-row block)
        const int qn = (mb < p.M ? mb : p.M - 1) / p.hyper_rows;
        if (qn != hq) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
                if (li < 3) {
                    const float* hp = p.hyper + ((long long)qn * 3 + li) * p.Cout + co + 16 * kg + 8 * ks;
                    a = *(const f32x4*)hp;
                    b = *(const f32x4*)(hp + 4);
                }
                vec8<T> f;
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = (T)a[e], f[4 + e] = (T)b[e];
                const vec8<T> zf = {};
                he[ks] = kg < 2 ? f : zf;
                ho[ks] = kg < 2 ? zf : f;
            }
            hq = qn;
        }
        vec8<T> g[2];
#pragma unroll
        for (int jh = 0; jh < 2; ++jh) {  // 8 values = 4 pairs = one operand fragment at a time
            f32x2_t x[4], xc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 2 * jh + (k >> 1), h2 = k & 1;
                x[k] = (f32x2_t){acc[i][j][2 * h2], acc[i][j][2 * h2 + 1]} + bv[2 * j + h2];
                xc[k] = (f32x2_t){med3_bare(x[k][0], neg, 4.5f), med3_bare(x[k][1], neg, 4.5f)};
            }
            // (the polynomial's 8e-5 absolute error is below a bf16 ulp but a sixth of a half ulp at 1: the half engine evaluates its
            //  own GELU - gelu_for<f16_t>, the erfc form - as every other f16 kernel and the all-VALU form of this epilogue do)
            if constexpr (std::is_same<T, bf16_t>::value) {
                gelu_poly2<4>(x, xc);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = (f32x2_t){gelu_for<T>(x[k][0]), gelu_for<T>(x[k][1])};
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) g[jh][2 * k] = (T)x[k][0], g[jh][2 * k + 1] = (T)x[k][1];
        }
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
        d0 = mma16(he[0], g[0], d0);
        d0 = mma16(he[1], g[1], d0);
        d1 = mma16(ho[0], g[0], d1);
        d1 = mma16(ho[1], g[1], d1);
        const int m = mb + li;
        if (kg == 0 && m < p.M) {  // D[h][row]: lane (column = row li, kg = 0) holds h = 0 .. 3
            float* op = p.out_f32 + (long long)(n_wave0 >> 5) * 3 * p.M + m;  // [chunk][i][m]: 16 consecutive rows per store
            op[0] = d0[0];
            op[(long long)p.M] = d0[1];
            op[2 * (long long)p.M] = d0[2];
            op[3 * (long long)p.M] = d1[0];
            op[4 * (long long)p.M] = d1[1];
            op[5 * (long long)p.M] = d1[2];
        }
    }
}

template <typename T, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue_maskdot(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li,
                                                      int kg) {
    constexpr int NV = 4 * TN;
    if constexpr (sizeof(T) == 2 && TN == 4) {
        // (wave uniform; Cout % 64: a wave's 64 columns lie inside one tap; hyper_rows % 16: one query per 16-row block)
        if (p.act == ACT_GELU && p.Cout % 64 == 0 && p.N % 64 == 0 && p.hyper_rows % 16 == 0 && !(p.tuning & 4)) {
            gemm_epilogue_maskdot_mfma<T, TM>(p, acc, m_wave0, n_wave0, li, kg);
            return;
        }
    }
    const int nb = n_wave0 + NV * kg;
    if (nb >= p.N) return;  // (N % 32 == 0: the lanes sharing a chunk leave together)
    const int co = nb % p.Cout;
    float bv[NV], hv[3][NV];
#pragma unroll
    for (int c = 0; c < NV; c += 4) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b4 = p.bias ? *(const f32x4*)(p.bias + nb + c) : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[c + e] = b4[e];
    }
    int hq = -1;
    const bool writer = NV == 16 ? (kg & 1) == 0 : kg == 0;
    // fully unrolled over the rows (static accumulator indexing; rolled with a row switch it measured 8 % slower: 1123 vs 1032 us
    // on the c3 shape)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        float v[NV];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r];
        const int m = m_wave0 + i * 16 + li;
        const bool ok = m < p.M;
        const int qn = (ok ? m : p.M - 1) / p.hyper_rows;
        if (qn != hq) {  // (a tile normally lies inside one query: loaded once)
#pragma unroll
            for (int h = 0; h < 3; ++h)
#pragma unroll
                for (int c = 0; c < NV; c += 4) {
                    const f32x4 h4 = *(const f32x4*)(p.hyper + ((long long)qn * 3 + h) * p.Cout + co + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[h][c + e] = h4[e];
                }
            hq = qn;
        }
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            float x = v[c] + bv[c];
            if (p.act == ACT_GELU)
                x = gelu_for<T>(x);
            else if (p.act == ACT_RELU)
                x = fmaxf(x, 0.f);
            d0 += x * hv[0][c];
            d1 += x * hv[1][c];
            d2 += x * hv[2][c];
        }
        // sum over the lane groups that share the 32-column chunk: v_permlane16_swap / v_permlane32_swap (gfx950 VALU lane
        // exchanges; [0] + [1] = own + partner in every lane, the same two addends as a shuffle) instead of __shfl_xor, which
        // is a ds_bpermute round trip through the LDS crossbar per value (24 dependent ones per wave and tile)
        auto xsum16 = [](float d) {
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(d), __float_as_uint(d), false, false);
            return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
        };
        auto xsum32 = [](float d) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d), __float_as_uint(d), false, false);
            return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
        };
        d0 = xsum16(d0);
        d1 = xsum16(d1);
        d2 = xsum16(d2);
        if (NV == 8) {
            d0 = xsum32(d0);
            d1 = xsum32(d1);
            d2 = xsum32(d2);
        }
        if (writer && ok) {
            float* op = p.out_f32 + (long long)(nb >> 5) * 3 * p.M + m;  // [chunk][i][m]: 16 consecutive rows per store
            op[0] = d0;
            op[(long long)p.M] = d1;
            op[2 * (long long)p.M] = d2;
        }
    }
}

// ROLLED = false: the row loop is fully unrolled (registers die row by row: 120 VGPRs for the 128x128 kernel, which
// keeps 2-3 workgroups per CU).  ROLLED = true (gemm8p.hpp, alone on its CU with registers to spare): the row body -
// ~1k instructions with every epilogue flavour and the integer divisions of the scatter paths - exists ONCE; TM
// unrolled copies overflow the instruction cache (measured: 15 us per 256x256 tile) and nothing hides those misses.
template <typename T, int TM, int TN, bool ROLLED = false>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li,
                                              int kg) {
    constexpr int ES = sizeof(T);
    constexpr int NV = 4 * TN;
    const int nb = n_wave0 + NV * kg;
    // the lane's bias values are row independent: fetch them once, ahead of the row loop (a load inside the loop
    // costs one exposed L2 round trip per row when the workgroup is alone on its CU)
    float bv[NV];
#pragma unroll
    for (int g8 = 0; g8 < NV; g8 += 8) {
        const bool ok = p.bias && nb + g8 < p.N;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b0 = ok ? *(const f32x4*)(p.bias + nb + g8) : z, b1 = ok ? *(const f32x4*)(p.bias + nb + g8 + 4) : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bv[g8 + q] = b0[q];
            bv[g8 + 4 + q] = b1[q];
        }
    }
    // column part of the output offset (row independent: the ConvTranspose tap decomposition costs five integer
    // divisions, which used to be repeated for every row)
    long long coff[NV / 8];
#pragma unroll
    for (int g8 = 0; g8 < NV; g8 += 8) {
        const int n = nb + g8;
        if (p.epi == EPI_CONVT) {
            const int tap = n / p.Cout, co = n - tap * p.Cout;
            const int dw = tap % p.kw, dh = (tap / p.kw) % p.kh, dt = tap / (p.kw * p.kh);
            coff[g8 / 8] = (((long long)dt * (p.Hi * p.kh) + dh) * (p.Wi * p.kw) + dw) * p.Cout + co;
        } else {
            coff[g8 / 8] = n;
        }
    }
    if (ROLLED) {
#pragma nounroll
        for (int i = 0; i < TM; ++i) {
            float v[NV];
#define L4P_ACC_ROW(I)                                                                                   \
    case I:                                                                                              \
        if (I < TM) {                                                                                    \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                               \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[I < TM ? I : 0][j][r]; \
        }                                                                                                \
        break;
            switch (i) {  // wave-uniform: keeps the accumulators statically indexed
                L4P_ACC_ROW(0) L4P_ACC_ROW(1) L4P_ACC_ROW(2) L4P_ACC_ROW(3) L4P_ACC_ROW(4) L4P_ACC_ROW(5) L4P_ACC_ROW(6) L4P_ACC_ROW(7)
            }
#undef L4P_ACC_ROW
            static_assert(TM <= 8, "extend the accumulator row switch");
            const int m = m_wave0 + i * 16 + li;
            if (m < p.M) gemm_epilogue_row<T, NV>(p, v, bv, coff, m, nb);
        }
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float v[NV];
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r];
            const int m = m_wave0 + i * 16 + li;
            if (m < p.M) gemm_epilogue_row<T, NV>(p, v, bv, coff, m, nb);
        }
    }
}

template <typename T, int NV>
__device__ __forceinline__ void gemm_epilogue_row(const GemmParams& p, float (&v)[NV], const float (&bv)[NV],
                                                  const long long (&coff)[NV / 8], int m, int nb) {
    constexpr int ES = sizeof(T);
    {
        // float residuals of the whole row segment, loaded before any of its outputs is stored (in-place updates alias)
        float rv[NV], rv2[NV];
        const bool res32 = p.res1 && p.res_f32;
        // row of the residual: the broadcast table's, else the output's row map (l4p_gemm_desc.c_*: "rows of out / residual", as the
        // lean bodies read it through EpiRowMapDesc)
        const long long mres = p.res_mod > 0 ? (m % p.res_mod) : (p.c_gr > 0 ? (long long)(m / p.c_gr) * p.c_gs + p.c_go + (m % p.c_gr) : m);
        if (res32) {
            const long long rrow = mres * p.ldr;
#pragma unroll
            for (int g8 = 0; g8 < NV; g8 += 8) {
                const int n = nb + g8;
                f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0, s0 = r0, s1 = r0;
                if (n < p.N) {
                    r0 = *(const f32x4*)((const float*)p.res1 + rrow + n);
                    r1 = *(const f32x4*)((const float*)p.res1 + rrow + n + 4);
                    if (p.res2) {
                        s0 = *(const f32x4*)((const float*)p.res2 + rrow + n);
                        s1 = *(const f32x4*)((const float*)p.res2 + rrow + n + 4);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    rv[g8 + q] = r0[q];
                    rv[g8 + 4 + q] = r1[q];
                    rv2[g8 + q] = s0[q];
                    rv2[g8 + 4 + q] = s1[q];
                }
            }
        }
        // row part of the output offset
        long long rowoff;
        if (p.epi == EPI_CONVT) {
            int wi, hi, ti, b;
            if (((p.Wi & (p.Wi - 1)) | (p.Hi & (p.Hi - 1)) | (p.Ti & (p.Ti - 1))) == 0) {  // power-of-two grid: shifts
                const int sw = __builtin_ctz(p.Wi), sh = __builtin_ctz(p.Hi), st = __builtin_ctz(p.Ti);
                wi = m & (p.Wi - 1);
                hi = (m >> sw) & (p.Hi - 1);
                ti = (m >> (sw + sh)) & (p.Ti - 1);
                b = m >> (sw + sh + st);
            } else {
                wi = m % p.Wi;
                int r = m / p.Wi;
                hi = r % p.Hi;
                r /= p.Hi;
                ti = r % p.Ti;
                b = r / p.Ti;
            }
            rowoff = ((((long long)b * p.Ti + ti) * p.kt * (p.Hi * p.kh) + hi * p.kh) * (p.Wi * p.kw) + wi * p.kw) * p.Cout;
        } else {
            const long long pm = p.c_gr > 0 ? (long long)(m / p.c_gr) * p.c_gs + p.c_go + (m % p.c_gr) : m;
            rowoff = pm * p.ldc;
        }
#pragma unroll
        for (int g8 = 0; g8 < NV; g8 += 8) {
            const int n = nb + g8;
            if (n >= p.N) continue;  // N % 8 == 0 is required
            float* vv = v + g8;
#pragma unroll
            for (int q = 0; q < 8; ++q) vv[q] += bv[g8 + q];
            if (p.act == ACT_GELU) {
#pragma unroll
                for (int q = 0; q < 8; ++q) vv[q] = gelu_for<T>(vv[q]);
            } else if (p.act == ACT_RELU) {
#pragma unroll
                for (int q = 0; q < 8; ++q) vv[q] = fmaxf(vv[q], 0.0f);
            }
            if (p.epi == EPI_QKV && n < p.H * p.Dp && p.q_scale != 0.f) {  // q = q * scale (modeling_finetune.py:180)
#pragma unroll
                for (int q = 0; q < 8; ++q) vv[q] *= p.q_scale;
            }
            const long long off = rowoff + coff[g8 / 8];  // element offset of the 8 outputs
            if (res32) {
#pragma unroll
                for (int q = 0; q < 8; ++q) vv[q] += rv[g8 + q];
                if (p.res2) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) vv[q] += rv2[g8 + q];
                }
            } else if (p.res1) {
                const long long roff = mres * p.ldr + n;
                const T* rp = (const T*)p.res1 + roff;
#pragma unroll
                for (int q = 0; q < 8; ++q) vv[q] += to_f32<T>(rp[q]);
                if (p.res2) {
                    const T* sp = (const T*)p.res2 + roff;
#pragma unroll
                    for (int q = 0; q < 8; ++q) vv[q] += to_f32<T>(sp[q]);
                }
            }
            if (p.epi == EPI_QKV && n >= p.H * p.Dp && n < 2 * p.H * p.Dp) {
                // K, stored in the attention kernel's LDS tile order (attention.hip): 8-element groups
                // [b][h][kv block][k-step][key][half ^ ((key >> 3) & 1)], KVB keys per block
                constexpr int KVB = 128 / ES;
                const int nk = n - p.H * p.Dp;
                const int h = nk / p.Dp, d0 = nk - h * p.Dp;
                const int ks = d0 >> 4, half = (d0 >> 3) & 1;
                const int b = m / p.S, s = m - b * p.S;
                const int kb = s / KVB, key = s - kb * KVB;
                const long long g8 =
                    ((((long long)(b * p.H + h) * (p.S / KVB) + kb) * (p.Dp / 16) + ks) * KVB + key) * 2 + (half ^ ((key >> 3) & 1));
                T* kp = (T*)p.k_tiled + g8 * 8;
                if (ES == 2) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)vv[q];
                    *(vec8h<T>*)kp = o;
                } else {
                    *(f32x4*)kp = (f32x4){vv[0], vv[1], vv[2], vv[3]};
                    *(f32x4*)((float*)kp + 4) = (f32x4){vv[4], vv[5], vv[6], vv[7]};
                }
                continue;
            }
            if (p.epi == EPI_QKV && n >= 2 * p.H * p.Dp) {
                // V, stored transposed: vt[((b*H + h)*Dp + d)*S + s]
                const int nv = n - 2 * p.H * p.Dp;
                const int h = nv / p.Dp, d = nv - h * p.Dp;
                const int b = m / p.S, s = m - b * p.S;
                T* vp = (T*)p.vt + ((long long)(b * p.H + h) * p.Dp + d) * p.S + s;
#pragma unroll
                for (int q = 0; q < 8; ++q) vp[(long long)q * p.S] = from_f32<T>(vv[q]);
                continue;
            }
            if (p.out_f32) {
                float* op = p.out_f32 + off;
                *(f32x4*)op = (f32x4){vv[0], vv[1], vv[2], vv[3]};
                *(f32x4*)(op + 4) = (f32x4){vv[4], vv[5], vv[6], vv[7]};
            }
            if (p.out_relu_T) {  // second output: relu(v) as T (pre-activated input of the next ResidualConvUnit conv)
                T* op = (T*)p.out_relu_T + off;
                if (ES == 2) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)fmaxf(vv[q], 0.f);
                    *(vec8h<T>*)op = o;
                } else {
                    *(f32x4*)op = (f32x4){fmaxf(vv[0], 0.f), fmaxf(vv[1], 0.f), fmaxf(vv[2], 0.f), fmaxf(vv[3], 0.f)};
                    *(f32x4*)((float*)op + 4) = (f32x4){fmaxf(vv[4], 0.f), fmaxf(vv[5], 0.f), fmaxf(vv[6], 0.f), fmaxf(vv[7], 0.f)};
                }
            }
            if (p.out_T) {
                T* op = (T*)p.out_T + off;
                if (ES == 2) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)vv[q];
#ifdef GEMM_DBG_NOSTORE  // (tools/probes: epilogue arithmetic without the output traffic)
                    asm volatile("" ::"v"(o), "v"(op));
#else
                    *(vec8h<T>*)op = o;
#endif
                } else {
                    *(f32x4*)op = (f32x4){vv[0], vv[1], vv[2], vv[3]};
                    *(f32x4*)((float*)op + 4) = (f32x4){vv[4], vv[5], vv[6], vv[7]};
                }
            }
        }
    }
}

// logical row m -> physical row of the output / residual: the descriptor's optional one-level row map (l4p_gemm_desc.c_*)
struct EpiRowMapDesc {
    const GemmParams& p;
    __device__ __forceinline__ long long operator()(int m) const {
        return p.c_gr > 0 ? (long long)(m / p.c_gr) * p.c_gs + p.c_go + (m % p.c_gr) : m;
    }
};

// Lean epilogue for the plain dense family (L4P_EPI_DENSE, no row maps, no broadcast residual): what the large GEMMs and
// convs of the 8-phase kernel mostly run.  The generic row body above decides every flavour (scatter forms, row maps,
// residual kinds, activations) at run time inside the row loop - ~600 issued instructions per row with SGPR spills,
// measured at 9 us per 256 x 256 tile for a bias + bf16 store (27 of fc1's 157 us at batch 4).  Here activation and
// residual kind are template parameters, the loop body is a few dozen instructions, and the residual of row i + 1 is
// requested before row i is finished (one exposed round trip per tile instead of one per row).
// RES: 0 none, 1 float (p.res1 [+ p.res2]), 2 T.
// RowMap: any callable int -> long long (conv3_halo.hpp passes the voxel-tile map of its 3-D output tiles)
template <typename T, int TM, int TN, int ACT, int RES, class RowMap>
__device__ __forceinline__ void gemm_epilogue_dense(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li,
                                                    int kg, const RowMap& crow) {
    constexpr int ES = sizeof(T);
    constexpr int NV = 4 * TN, NG = NV / 8;
    const int nb = n_wave0 + NV * kg;
    bool gok[NG];
    float bv[NV];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        gok[g] = nb + 8 * g < p.N;  // N % 8 == 0
        const bool ok = p.bias && gok[g];
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b0 = ok ? *(const f32x4*)(p.bias + nb + 8 * g) : z, b1 = ok ? *(const f32x4*)(p.bias + nb + 8 * g + 4) : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bv[8 * g + q] = b0[q];
            bv[8 * g + 4 + q] = b1[q];
        }
    }
    const bool two = RES == 2 && p.res2 != nullptr;  // (a second residual only exists in the engine dtype: the DPT fusion convs)
    // Residual registers: a ring of RD rows (float: NV values per residual and row; T: NV / 2 dwords).  The rows of a lane are
    // 16 apart, every row is its own HBM round trip, and nothing else runs on the CU while its workgroup is in the epilogue: with
    // one row of look-ahead the 8 rows of a wave were 8 dependent round trips (the tall tracker GEMM with a float residual
    // in + out spent more time here than in its main loop).  RD rows are requested before the first one is needed.
#ifndef GEMM_EPI_RES_DEPTH
#define GEMM_EPI_RES_DEPTH 4
#endif
    constexpr int RD = RES == 0 ? 1 : RES == 2 ? 2 : (GEMM_EPI_RES_DEPTH < TM ? GEMM_EPI_RES_DEPTH : TM);
    f32x4 rf[RD][RES == 1 ? 2 * NG : 1][1];
    u32x4 rt[RD][RES == 2 ? NG : 1][2];
    // (row map of the output and the residual: logical row m lives at physical row crow(m))
    auto load_res = [&](int m, auto slot_) {
        constexpr int sl = decltype(slot_)::value;
        const long long roff = crow(m) * p.ldr + nb;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (!gok[g]) continue;
            if (RES == 1) {
                rf[sl][2 * g][0] = *(const f32x4*)((const float*)p.res1 + roff + 8 * g);
                rf[sl][2 * g + 1][0] = *(const f32x4*)((const float*)p.res1 + roff + 8 * g + 4);
            } else if (RES == 2) {
                rt[sl][g][0] = *(const u32x4*)((const T*)p.res1 + roff + 8 * g);
                if (two) rt[sl][g][1] = *(const u32x4*)((const T*)p.res2 + roff + 8 * g);
            }
        }
    };
    if (RES != 0) {
        static_for<0, RD>([&](auto d_) {
            constexpr int d = decltype(d_)::value;
            if (m_wave0 + d * 16 + li < p.M) load_res(m_wave0 + d * 16 + li, d_);
        });
    }
    // fully unrolled over the TM rows: the body is lean enough for that (~40 instructions a row), and a rolled loop makes
    // hipcc index the accumulator rows through scratch memory (one round trip per row: measured slower than the generic body)
    static_for<0, TM>([&](auto i_) {
        constexpr int i = decltype(i_)::value, sl = i % RD;
        float v[NV];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r];
        const int m = m_wave0 + i * 16 + li;
        if (m >= p.M) return;  // (rows only run out at the bottom of the matrix: nothing after this row either)
        if constexpr (ACT == ACT_GELU && std::is_same<T, bf16_t>::value && NV % 8 == 0) {
            // gelu_poly on four interleaved pairs (gelu_poly2: same operations per element, bit for bit; one pair at a time the
            // compiler put a wait state behind every packed op of the serial Horner chain)
#pragma unroll
            for (int c = 0; c < NV; c += 8) {
                f32x2_t x[4], xc[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[k] = (f32x2_t){v[c + 2 * k] + bv[c + 2 * k], v[c + 2 * k + 1] + bv[c + 2 * k + 1]};
                    xc[k] = (f32x2_t){med3_bare(x[k][0], -4.5f, 4.5f), med3_bare(x[k][1], -4.5f, 4.5f)};
                }
                gelu_poly2<4>(x, xc);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c + 2 * k] = x[k][0], v[c + 2 * k + 1] = x[k][1];
            }
        } else {
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                float x = v[c] + bv[c];
                if (ACT == ACT_GELU)
                    x = gelu_for<T>(x);
                else if (ACT == ACT_RELU)
                    x = fmaxf(x, 0.f);
                v[c] = x;
            }
        }
        if (RES == 1) {
#pragma unroll
            for (int g = 0; g < 2 * NG; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[4 * g + q] += rf[sl][g][0][q];
        } else if (RES == 2) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (ES == 2) {
                        const vec8h<T> a = __builtin_bit_cast(vec8h<T>, rt[sl][g][0]), b = __builtin_bit_cast(vec8h<T>, rt[sl][g][1]);
                        v[8 * g + q] += two ? (float)a[q] + (float)b[q] : (float)a[q];
                    }
                }
        }
        // row i + RD's residual is requested now, into the slot this row has just released: its values are copies in
        // registers, so an in-place update of THIS row (out aliasing res1) cannot reach them, and rows never overlap
        if constexpr (RES != 0 && i + RD < TM) {
            if (m + 16 * RD < p.M) load_res(m + 16 * RD, std::integral_constant<int, sl>{});
        }
        const long long off = crow(m) * p.ldc + nb;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (!gok[g]) continue;
            const float* vv = v + 8 * g;
            if (p.out_f32) {
                float* op = p.out_f32 + off + 8 * g;
                *(f32x4*)op = (f32x4){vv[0], vv[1], vv[2], vv[3]};
                *(f32x4*)(op + 4) = (f32x4){vv[4], vv[5], vv[6], vv[7]};
            }
            if (ES == 2) {
                if (p.out_relu_T) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)fmaxf(vv[q], 0.f);
                    *(vec8h<T>*)((T*)p.out_relu_T + off + 8 * g) = o;
                }
                if (p.out_T) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)vv[q];
#ifdef GEMM_DBG_NOSTORE
                    asm volatile("" ::"v"(o));
#else
                    *(vec8h<T>*)((T*)p.out_T + off + 8 * g) = o;
#endif
                }
            }
        }
    });
}

template <typename T, int TM, int TN, int ACT, int RES>
__device__ __forceinline__ void gemm_epilogue_dense(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li,
                                                    int kg) {
    gemm_epilogue_dense<T, TM, TN, ACT, RES>(p, acc, m_wave0, n_wave0, li, kg, EpiRowMapDesc{p});
}

// Lean form of the L4P_EPI_QKV epilogue (bf16): what a lane's two 8-column groups are (q / k / v, head, dim) does not
// depend on the row, so it is decided once; a row costs one division (m -> batch, token), the bias, the q scale and its stores.
template <typename T, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue_qkv(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li, int kg) {
    static_assert(sizeof(T) == 2, "bf16 kernels only");
    constexpr int NV = 4 * TN, NG = NV / 8, KVB = 64;
    const int nb = n_wave0 + NV * kg, HD = p.H * p.Dp;
    int kind[NG];          // 0 q, 1 k, 2 v, -1 out of range
    long long cbase[NG];   // column part of the element offset
    int kflip[NG];
    float bv[NV], qs[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int n = nb + 8 * g;
        kind[g] = n >= p.N ? -1 : (n < HD ? 0 : (n < 2 * HD ? 1 : 2));
        qs[g] = (kind[g] == 0 && p.q_scale != 0.f) ? p.q_scale : 1.f;
        kflip[g] = 0;
        cbase[g] = n;
        if (kind[g] == 1) {  // K tile order: 8-element groups [b][h][kv block][k-step][key][half ^ ((key >> 3) & 1)]
            const int nk = n - HD, h = nk / p.Dp, d0 = nk - h * p.Dp;
            kflip[g] = (d0 >> 3) & 1;
            cbase[g] = ((long long)h * (p.S / KVB) * (p.Dp / 16) + (d0 >> 4)) * KVB;  // + (b*H*(S/KVB) + kb)*(Dp/16)*KVB + key
        } else if (kind[g] == 2) {  // V^T: vt[((b*H + h)*Dp + d)*S + s]
            const int nv = n - 2 * HD, h = nv / p.Dp, d = nv - h * p.Dp;
            cbase[g] = ((long long)h * p.Dp + d) * p.S;
        }
        const bool ok = p.bias && kind[g] >= 0;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b0 = ok ? *(const f32x4*)(p.bias + n) : z, b1 = ok ? *(const f32x4*)(p.bias + n + 4) : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bv[8 * g + q] = b0[q];
            bv[8 * g + 4 + q] = b1[q];
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m_wave0 + i * 16 + li;
        if (m >= p.M) continue;
        const int b = m / p.S, s_ = m - b * p.S;
        const int kb = s_ / KVB, key = s_ - kb * KVB;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (kind[g] < 0) continue;
            vec8h<T> o;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = (T)((acc[i][2 * g + q / 4][q % 4] + bv[8 * g + q]) * qs[g]);
            if (kind[g] == 0) {
                *(vec8h<T>*)((T*)p.out_T + (long long)m * p.ldc + cbase[g]) = o;
            } else if (kind[g] == 1) {
                const long long g8 = (cbase[g] + ((long long)b * p.H * (p.S / KVB) + kb) * (p.Dp / 16) * KVB + key) * 2 + (kflip[g] ^ ((key >> 3) & 1));
                *(vec8h<T>*)((T*)p.k_tiled + g8 * 8) = o;
            } else {
                T* vp = (T*)p.vt + (long long)b * p.H * p.Dp * p.S + cbase[g] + s_;
#pragma unroll
                for (int q = 0; q < 8; ++q) vp[(long long)q * p.S] = o[q];
            }
        }
    }
}

// Lean form of the L4P_EPI_CONVT epilogue (ConvTranspose3d with kernel == stride, bf16 output, bias, no activation):
// the tap / output-channel part of the scatter offset is per column group, the voxel part per row.
template <typename T, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue_convt(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li, int kg) {
    static_assert(sizeof(T) == 2, "bf16 kernels only");
    constexpr int NV = 4 * TN, NG = NV / 8;
    const int nb = n_wave0 + NV * kg;
    bool gok[NG];
    long long coff[NG];
    float bv[NV];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int n = nb + 8 * g;
        gok[g] = n < p.N;
        const int tap = n / p.Cout, co = n - tap * p.Cout;
        const int dw = tap % p.kw, dh = (tap / p.kw) % p.kh, dt = tap / (p.kw * p.kh);
        coff[g] = (((long long)dt * (p.Hi * p.kh) + dh) * (p.Wi * p.kw) + dw) * p.Cout + co;
        const bool ok = p.bias && gok[g];
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b0 = ok ? *(const f32x4*)(p.bias + n) : z, b1 = ok ? *(const f32x4*)(p.bias + n + 4) : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bv[8 * g + q] = b0[q];
            bv[8 * g + 4 + q] = b1[q];
        }
    }
    const bool pow2 = ((p.Wi & (p.Wi - 1)) | (p.Hi & (p.Hi - 1)) | (p.Ti & (p.Ti - 1))) == 0;
    const int sw = __builtin_ctz(p.Wi), sh = __builtin_ctz(p.Hi), st = __builtin_ctz(p.Ti);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m_wave0 + i * 16 + li;
        if (m >= p.M) continue;
        int wi, hi, ti, b;
        if (pow2) {
            wi = m & (p.Wi - 1);
            hi = (m >> sw) & (p.Hi - 1);
            ti = (m >> (sw + sh)) & (p.Ti - 1);
            b = m >> (sw + sh + st);
        } else {
            wi = m % p.Wi;
            int r = m / p.Wi;
            hi = r % p.Hi;
            r /= p.Hi;
            ti = r % p.Ti;
            b = r / p.Ti;
        }
        const long long rowoff = ((((long long)b * p.Ti + ti) * p.kt * (p.Hi * p.kh) + hi * p.kh) * (p.Wi * p.kw) + wi * p.kw) * p.Cout;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (!gok[g]) continue;
            vec8h<T> o;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = (T)(acc[i][2 * g + q / 4][q % 4] + bv[8 * g + q]);
            *(vec8h<T>*)((T*)p.out_T + rowoff + coff[g]) = o;
        }
    }
}

// Epilogue of the sub-pixel conv: the L4P_EPI_CONVT scatter (pixel shuffle) + the border-class bias row + the optional relu copy.
// p.bias is a table [27][Cout]: row ((c_t * 3 + c_h) * 3 + c_w), c = 0 / 1 / 2 where the up-scaled position p has p - 1 outside the
// grid / both neighbours inside / p + 1 outside (the ConvTranspose bias exists inside the up-scaled grid and is zero in the conv's
// padding; every up-scaled axis is at least 2 long - checked by the launcher - so the three cases are exclusive).  The interior row
// is fetched once per lane; a border row of the tile fetches its own.
template <typename T, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue_subpixel(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0, int li, int kg) {
    constexpr int ES = sizeof(T), NV = 4 * TN, NG = NV / 8;
    const int nb = n_wave0 + NV * kg;
    const int s = n_wave0 / p.Cout, co = nb - s * p.Cout;  // (a wave's columns lie inside one sub-position: Cout % tile width == 0)
    const int s_w = s % p.kw, s_h = (s / p.kw) % p.kh, s_t = s / (p.kw * p.kh);
    const int To = p.Ti * p.kt, Ho = p.Hi * p.kh, Wo = p.Wi * p.kw;
    const long long coff = (((long long)s_t * Ho + s_h) * Wo + s_w) * p.Cout + co;
    float bv[NV];
#pragma unroll
    for (int c = 0; c < NV; c += 4) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 b4 = p.bias ? *(const f32x4*)(p.bias + 13 * p.Cout + co + c) : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[c + q] = b4[q];
    }
    const bool pow2 = ((p.Wi & (p.Wi - 1)) | (p.Hi & (p.Hi - 1)) | (p.Ti & (p.Ti - 1))) == 0;
    const int sw = __builtin_ctz(p.Wi), sh = __builtin_ctz(p.Hi), st = __builtin_ctz(p.Ti);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m_wave0 + i * 16 + li;
        if (m >= p.M) continue;
        int wi, hi, ti, b;
        if (pow2) {
            wi = m & (p.Wi - 1);
            hi = (m >> sw) & (p.Hi - 1);
            ti = (m >> (sw + sh)) & (p.Ti - 1);
            b = m >> (sw + sh + st);
        } else {
            wi = m % p.Wi;
            int r = m / p.Wi;
            hi = r % p.Hi;
            r /= p.Hi;
            ti = r % p.Ti;
            b = r / p.Ti;
        }
        const int pt = ti * p.kt + s_t, ph = hi * p.kh + s_h, pw = wi * p.kw + s_w;
        const int cls = ((pt == 0 ? 0 : pt == To - 1 ? 2 : 1) * 3 + (ph == 0 ? 0 : ph == Ho - 1 ? 2 : 1)) * 3 + (pw == 0 ? 0 : pw == Wo - 1 ? 2 : 1);
        float v[NV];
        if (p.bias && cls != 13) {
            const float* bp = p.bias + cls * p.Cout + co;
#pragma unroll
            for (int c = 0; c < NV; c += 4) {
                const f32x4 b4 = *(const f32x4*)(bp + c);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[c + q] = acc[i][c / 4][q] + b4[q];
            }
        } else {
#pragma unroll
            for (int c = 0; c < NV; ++c) v[c] = acc[i][c / 4][c % 4] + bv[c];
        }
        const long long off = ((((long long)b * To + pt - s_t) * Ho + (ph - s_h)) * Wo + (pw - s_w)) * p.Cout + coff;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* vv = v + 8 * g;
            if (ES == 2) {
                if (p.out_relu_T) {
                    vec8h<T> o;
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = (T)fmaxf(vv[q], 0.f);
                    *(vec8h<T>*)((T*)p.out_relu_T + off + 8 * g) = o;
                }
                vec8h<T> o;
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = (T)vv[q];
                *(vec8h<T>*)((T*)p.out_T + off + 8 * g) = o;
            } else {
                if (p.out_relu_T) {
                    float* op = (float*)p.out_relu_T + off + 8 * g;
                    *(f32x4*)op = (f32x4){fmaxf(vv[0], 0.f), fmaxf(vv[1], 0.f), fmaxf(vv[2], 0.f), fmaxf(vv[3], 0.f)};
                    *(f32x4*)(op + 4) = (f32x4){fmaxf(vv[4], 0.f), fmaxf(vv[5], 0.f), fmaxf(vv[6], 0.f), fmaxf(vv[7], 0.f)};
                }
                float* op = (float*)p.out_T + off + 8 * g;
                *(f32x4*)op = (f32x4){vv[0], vv[1], vv[2], vv[3]};
                *(f32x4*)(op + 4) = (f32x4){vv[4], vv[5], vv[6], vv[7]};
            }
        }
    }
}

// the plain dense family (activation x residual kind); false = a combination that has no lean body.  Host-side twin of the
// condition: dense_epilogue_is_lean() in gemm_select.hpp.
template <typename T, int TM, int TN, class RowMap>
__device__ __forceinline__ bool gemm_epilogue_dense_cases(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0,
                                                          int li, int kg, const RowMap& crow) {
    if (p.epi != EPI_DENSE || p.res_mod > 0) return false;
    const int res = !p.res1 ? 0 : (p.res_f32 ? 1 : 2);
    if (res == 1 && p.res2) return false;  // (two float residuals: no caller; the generic body handles it)
#define L4P_EPI_CASE(A, R)                                                                    \
    if (p.act == A && res == R) {                                                             \
        gemm_epilogue_dense<T, TM, TN, A, R>(p, acc, m_wave0, n_wave0, li, kg, crow);         \
        return true;                                                                          \
    }
    L4P_EPI_CASE(ACT_NONE, 0)
    L4P_EPI_CASE(ACT_GELU, 0)
    L4P_EPI_CASE(ACT_RELU, 0)
    L4P_EPI_CASE(ACT_NONE, 1)
    L4P_EPI_CASE(ACT_NONE, 2)
    L4P_EPI_CASE(ACT_RELU, 2)
#undef L4P_EPI_CASE
    return false;
}

// run-time selection of the specialisation (wave-uniform); false = not a plain dense epilogue, use the generic one
template <typename T, int TM, int TN>
__device__ __forceinline__ bool gemm_epilogue_dense_dispatch(const GemmParams& p, f32x4 (&acc)[TM][TN], int m_wave0, int n_wave0,
                                                             int li, int kg) {
    static_assert(sizeof(T) == 2, "bf16 kernels only");
    if (p.tuning & 1) return false;
    if (p.epi == EPI_QKV && !p.res1 && p.act == ACT_NONE && p.c_gr == 0) {
        gemm_epilogue_qkv<T, TM, TN>(p, acc, m_wave0, n_wave0, li, kg);
        return true;
    }
    if (p.epi == EPI_CONVT && !p.res1 && p.act == ACT_NONE && p.out_T && !p.out_f32 && !p.out_relu_T) {
        gemm_epilogue_convt<T, TM, TN>(p, acc, m_wave0, n_wave0, li, kg);
        return true;
    }
    return gemm_epilogue_dense_cases<T, TM, TN>(p, acc, m_wave0, n_wave0, li, kg, EpiRowMapDesc{p});
}
