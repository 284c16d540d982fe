// Included by gemm_bf16.hip / gemm_f16.hip / gemm_f32.hip with GEMM_T and GEMM_FN (+ GEMM_GROUP_FN for the 16-bit types) defined.
#include <cstdlib>
#include <cstring>

#include "gemm.hpp"
#include "prof.hpp"

// Second pass of a split-K GEMM / conv: sum the float partials and apply the dense epilogue
// (bias, activation, up to two residuals, T / float / relu-copy outputs).  8 columns per thread.
template <typename T>
__global__ void splitk_finish_kernel(const GemmParams p) {
    const long long total = (long long)p.M * (p.N / 8);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i / (p.N / 8)), n = (int)(i % (p.N / 8)) * 8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < p.splitk; ++s) {
            const float* pp = p.partial + ((long long)s * p.M + m) * p.N + n;
            const f32x4 a = *(const f32x4*)pp, b = *(const f32x4*)(pp + 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] += a[q];
                v[4 + q] += b[q];
            }
        }
        if (p.bias) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] += p.bias[n + q];
        }
        if (p.act == ACT_GELU) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = gelu_for<T>(v[q]);
        } else if (p.act == ACT_RELU) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q], 0.f);
        }
        if (p.res1) {
            const long long roff = (long long)(p.res_mod > 0 ? (m % p.res_mod) : m) * p.ldr + n;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v[q] += p.res_f32 ? ((const float*)p.res1)[roff + q] : to_f32<T>(((const T*)p.res1)[roff + q]);
                if (p.res2) v[q] += p.res_f32 ? ((const float*)p.res2)[roff + q] : to_f32<T>(((const T*)p.res2)[roff + q]);
            }
        }
        const long long off = (long long)m * p.ldc + n;
        if (p.out_f32) {
#pragma unroll
            for (int q = 0; q < 8; ++q) p.out_f32[off + q] = v[q];
        }
        if (p.out_T) {
#pragma unroll
            for (int q = 0; q < 8; ++q) ((T*)p.out_T)[off + q] = from_f32<T>(v[q]);
        }
        if (p.out_relu_T) {
#pragma unroll
            for (int q = 0; q < 8; ++q) ((T*)p.out_relu_T)[off + q] = from_f32<T>(fmaxf(v[q], 0.f));
        }
    }
}

template <int BM, int BN, int MODE, bool GLDS, int STAGES = 2, int WM = 2, int WN = 2, bool GROUPW = false>
static int launch_cfg(const GemmParams& p, hipStream_t stream) {
    const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
    const int nsplit = p.splitk > 1 ? p.splitk : 1;
    const size_t lds = STAGES * (BM + BN) * 128;
    auto kern = gemm_kernel<GEMM_T, BM, BN, WM, WN, MODE, GLDS, STAGES, GROUPW>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof(MODE == 0 ? (p.w_gr > 0 || p.M < 1024 ? PROF_GEMM_SMALL : PROF_GEMM) : PROF_CONV3D, stream, "M%d N%d K%d epi%d act%d sk%d t%dx%d%s%s", p.M, p.N, p.K, p.epi, p.act, nsplit, BM, BN,
                   STAGES > 2 ? " deep" : "", GROUPW ? " wgrp" : "");
    hipLaunchKernelGGL(kern, dim3(ntm * ntn * nsplit), dim3(WM * WN * 64), lds, stream, p);
    if (nsplit > 1 && !(p.tuning & 2)) {  // (tuning bit 1: the caller sums the partials itself)
        const long long total = (long long)p.M * (p.N / 8);
        const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(splitk_finish_kernel<GEMM_T>, dim3(grid), dim3(256), 0, stream, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

#ifdef GEMM_HAS_8P
// 8-phase deep-pipelined kernel (gemm8p.hpp), bf16 only, no fused input ReLU
[[maybe_unused]] static int device_cu_count() {  // (per device: a host may drive several)
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    int n = cus[dev & 63].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = -1;
        cus[dev & 63].store(n, std::memory_order_relaxed);
    }
    return n > 0 ? n : 0;
}
template <int MODE, int WR, int WC, bool SPLITK, int TM, int TN, bool PERSIST>
static int launch_8p_form(const GemmParams& p, hipStream_t stream, int grid) {
    typedef Gemm8pCfg<WR, WC, TM, TN> Cfg;
    constexpr int BM = Cfg::BM, BN = Cfg::BN;
    const int nsplit = SPLITK ? p.splitk : 1;
    const size_t lds = Cfg::LDS_BYTES;
    auto kern = gemm8p_kernel<GEMM_T, MODE, WR, WC, SPLITK, TM, TN, PERSIST>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    char sk[12] = "";
    if (nsplit > 1) snprintf(sk, sizeof sk, " sk%d", nsplit);
    ProfScope prof(MODE == 0 ? PROF_GEMM : PROF_CONV3D, stream, "M%d N%d K%d epi%d act%d 8p%s%s t%dx%d", p.M, p.N, p.K, p.epi, p.act,
                   PERSIST ? " pst" : "", sk, BM, BN);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, p);
    if (nsplit > 1 && !(p.tuning & 2)) {  // (tuning bit 1: the caller sums the partials itself)
        const long long total = (long long)p.M * (p.N / 8);
        const int g2 = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(splitk_finish_kernel<GEMM_T>, dim3(g2), dim3(256), 0, stream, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// sub-pixel conv on the 8-phase kernel (l4p_conv3d_subpixel).  K of the tag = mean executed K of the launch: 2 M N K = executed FLOPs
static int launch_8p_subpixel(const GemmParams& p, hipStream_t stream, int mean_k) {
    typedef Gemm8pCfg<2, 4, 8, 4> Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = p.N / Cfg::BN;
    auto kern = gemm8p_kernel<GEMM_T, 1, 2, 4, false, 8, 4, false, true>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)Cfg::LDS_BYTES));
    ProfScope prof(PROF_CONV3D, stream, "M%d N%d K%d epi%d act%d subpix 8p t%dx%d", p.M, p.N, mean_k, L4P_EPI_CONVT, p.act, Cfg::BM, Cfg::BN);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn), dim3(512), Cfg::LDS_BYTES, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <int MODE, int WR, int WC, bool SPLITK = false, int TM = 8, int TN = 4>
static int launch_8p(const GemmParams& p, hipStream_t stream) {
    typedef Gemm8pCfg<WR, WC, TM, TN> Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
    const int nsplit = SPLITK ? p.splitk : 1;
#ifdef GEMM_8P_PERSIST_EXPERIMENT
    if constexpr (MODE == 0 && !SPLITK) {
        // persistent form (gemm8p.hpp, PERSIST): one workgroup per CU walks the tiles, the next tile's prologue rides under the
        // epilogue.  MEASURED SLOWER (same-call A/B, tools/probes/ab_persist.sh): mask product 1061 -> 1204 us, the tall tracker
        // GEMMs +1..3 %, QKV 115 -> 122 us, c3 829 -> 808 frames/s.  Correct (the 8-phase tests pass on it), but the tile loop
        // keeps ~270 scalars live where the plain kernel keeps ~70: the epilogue re-reads them from VGPR lanes (2 800 v_readlane in
        // the object code) and that costs more per tile than the hardware's workgroup launch + the exposed first round trip did.
        // Compiled only with -DGEMM_8P_PERSIST_EXPERIMENT (L4P_GEMM_PERSIST=0 then selects the plain launch).
        const int persist = knob(KNOB_GEMM_PERSIST);
        const int cus = device_cu_count();
        if (persist && cus >= 8 && cus % 8 == 0 && ntm * ntn > cus)
            return launch_8p_form<MODE, WR, WC, SPLITK, TM, TN, true>(p, stream, cus);
    }
#endif
    return launch_8p_form<MODE, WR, WC, SPLITK, TM, TN, false>(p, stream, ntm * ntn * nsplit);
}
#endif

#if defined(GEMM_HAS_8P) && defined(L4P_PROBE_KERNELS)
// Two-workgroups-per-CU form (gemm4w.hpp): 256 x 128 tiles on 4-wave workgroups, dense GEMM, bf16
static bool gemm4w_fits(const GemmParams& p) {
    if (p.relu_in || p.K % 8 || p.N <= 128) return false;
    const long long pm = p.a_gr > 0 ? (long long)((p.M - 1) / p.a_gr) * p.a_gs + p.a_go + p.a_gr : p.M;
    // (LDS-DMA pieces are addressed through 32-bit buffer offsets)
    return pm * p.lda * 2 < (1ll << 31) && (long long)p.N * p.ldw * 2 < (1ll << 31);
}
template <bool SPLITK>
static int launch_4w(const GemmParams& p, hipStream_t stream) {
    typedef Gemm4wCfg Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
    const int nsplit = SPLITK ? p.splitk : 1;
    auto kern = gemm4w_kernel<GEMM_T, SPLITK>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, Cfg::LDS_BYTES));
    char sk[12] = "";
    if (nsplit > 1) snprintf(sk, sizeof sk, " sk%d", nsplit);
    ProfScope prof(PROF_GEMM, stream, "M%d N%d K%d epi%d act%d 4w%s t%dx%d", p.M, p.N, p.K, p.epi, p.act, sk, Cfg::BM, Cfg::BN);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn * nsplit), dim3(256), Cfg::LDS_BYTES, stream, p);
    if (nsplit > 1 && !(p.tuning & 2)) {
        const long long total = (long long)p.M * (p.N / 8);
        const int g2 = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(splitk_finish_kernel<GEMM_T>, dim3(g2), dim3(256), 0, stream, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

#ifdef GEMM_HAS_8P
// LDS-halo 3x3x3 conv (conv3_halo.hpp): stride 1, bf16, all of N in one tile column, output volume made of whole blocks, and an
// epilogue of the lean dense family (the kernel has no generic epilogue)
static bool dense_epilogue_is_lean(const GemmParams& p) {  // host-side twin of gemm_epilogue_dense_cases (gemm.hpp)
    if ((p.tuning & 1) || p.epi != L4P_EPI_DENSE || p.res_mod > 0 || p.c_gr > 0 || p.a_gr > 0) return false;
    const int res = !p.res1 ? 0 : (p.res_f32 ? 1 : 2);
    if (res == 1 && p.res2) return false;
    return (res == 0) || (res == 1 && p.act == L4P_ACT_NONE) || (res == 2 && (p.act == L4P_ACT_NONE || p.act == L4P_ACT_RELU));
}
// host-side twin of gemm_epilogue_dense_dispatch (gemm.hpp): true when the kernel will take one of the lean epilogues
static bool epilogue_is_lean_8p(const GemmParams& p) {
    if (p.tuning & 1) return false;
    if (p.epi == L4P_EPI_QKV) return !p.res1 && p.act == L4P_ACT_NONE && p.c_gr == 0;
    if (p.epi == L4P_EPI_CONVT) return !p.res1 && p.act == L4P_ACT_NONE && p.out_T && !p.out_f32 && !p.out_relu_T;
    return dense_epilogue_is_lean(p);
}
template <int WR, int WC>
static bool conv_halo_fits(const GemmParams& p) {
    typedef ConvHaloCfg<WR, WC> Cfg;
    if (p.ups_hi > 0 && !(WR == 4 && WC == 2 && p.ups_wi > 0 && (long long)p.ups_hi * p.ups_wi * p.Cin * 2 < (1ll << 31))) return false;
    return p.N == Cfg::BN && p.st == 1 && p.sh == 1 && p.sw == 1 && p.Cin % 32 == 0 && p.To % Cfg::TT == 0 && p.Ho % Cfg::TH == 0 &&
           p.Wo % Cfg::TW == 0 && p.To == p.Ti && p.Ho == p.Hi && p.Wo == p.Wi && p.M / Cfg::BM >= 192 && p.ldc == p.N &&
           (!p.res1 || p.ldr == p.N) && (long long)p.M * p.Cin * 2 < (1ll << 32) && !p.relu_in && p.splitk <= 1 && dense_epilogue_is_lean(p);
}
template <int WR, int WC, bool UPS = false>
static int launch_halo(const GemmParams& p, hipStream_t stream) {
    typedef ConvHaloCfg<WR, WC> Cfg;
    auto kern = conv3_halo_kernel<GEMM_T, WR, WC, UPS>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, Cfg::LDS_BYTES));
    ProfScope prof(PROF_CONV3D, stream, "M%d N%d K%d epi%d act%d halo%s t%dx%d", p.M, p.N, p.K, p.epi, p.act, UPS ? " ups" : "", Cfg::BM, Cfg::BN);
    hipLaunchKernelGGL(kern, dim3(p.M / Cfg::BM), dim3(512), Cfg::LDS_BYTES, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

// Kernel / tile selection (measured, tools/probes/gemm_variants.hip):
//  * the 8-phase 256x256 kernel (gemm8p.hpp) once N > 128 and the problem fills the chip with 256-wide tiles:
//    +10..35 % over the 128x128 kernel on the batch-4 encoder linears, the tracker's tall GEMMs and the DPT convs;
//  * 128x128 (4 waves, 2 workgroups per CU) below that - it quantises better on 256 CUs at batch 1;
//  * 128x64 for narrow or small problems.  (The 8-wave 256x128 form of gemm.hpp never beat both of these.)
// L4P_GEMM_VARIANT (tuning aid): 1 = never use the 8-phase kernel, 10 = always.
static int GEMM_FN_impl(int mode, const GemmParams& p, hipStream_t stream);
int GEMM_FN(int mode, const GemmParams& p_in, hipStream_t stream);
// block-structured weights (l4p_gemm_desc.kw_cols): what gemm_body's per-tile k-window relies on - a tile's columns lie inside one
// column group (kw_cols a multiple of the widest tile) and the window is the tile's whole contraction (no split-K, no row groups).
// One statement for l4p_gemm and l4p_gemm_group: gemm_body honours kw_cols unconditionally.
static bool kw_cols_ok(int mode, const GemmParams& p) {
    if (mode != 0 || p.w_gr > 0 || p.splitk > 1 || p.relu_in || p.kw_cols % 128 || p.kw_len < 1 || p.K % 8) {
        l4p_set_error("l4p_gemm: kw_cols needs a dense GEMM without split-K / row groups, kw_cols a multiple of 128");
        return false;
    }
    return true;
}
#ifdef GEMM_HAS_8P
// A handful of rows (gemm_skinny.hpp: one wave per 16 x 32 output block, operands streamed into fragment registers; bit-identical to
// the LDS-staged kernels).  The wave count bounds it to problems whose weight stream is re-read by few row blocks.
static bool gemm_is_skinny(const GemmParams& p) {
    // (tools/probes/skinny_m_sweep.py, N = 1408, K = 1408: 6.1 us against 13.9 us up to 64 rows, 9.7 against 14.2 at 96 - 128 rows - more than
    //  256 waves, two to a CU; beyond 512 blocks the staged kernel is as fast)
    const int max_m = knob(KNOB_SKINNY_MAX_M);
    return knob(KNOB_GEMM_SKINNY) && p.M >= 1 && p.M <= max_m && p.K >= 64 && p.K % 64 == 0 && p.lda % 8 == 0 && p.ldw % 8 == 0 && p.N % 8 == 0 &&
           p.w_gr == 0 && p.kw_cols == 0 && p.splitk <= 1 && !p.relu_in && p.epi == L4P_EPI_DENSE && !(p.tuning & 4) &&
           (long long)((p.M + 15) / 16) * ((p.N + 31) / 32) <= 512;  // (wider: every row block streams the weights again - measured
                                                                     //  slower than the staged kernel at N = 11264: 14.8 vs 11.5 us)
}
// row-grouped weights (l4p_gemm_desc.w_gr) on few rows: the value projection of the folded token -> image attention - 8 head groups of
// 128 context rows against their head's 88 x 1408 block of W_v: 8 workgroups of the staged kernel, each alone with its 22 k-tiles
static bool gemm_is_skinny_grouped(const GemmParams& p) {
    // (few rows per group only: on the folded score products - 2048 rows per track against 48 folded rows - the one-wave kernel was
    //  measured at 32.7 us against the staged kernel's 12.4 us for 8 tracks, tools/probes/scores_time.py: every 16-row block streams
    //  its track's weights again)
    return knob(KNOB_GEMM_SKINNY) && p.w_gr > 0 && p.w_gr % 16 == 0 && p.M >= 1 && p.M <= 2048 && p.K >= 64 && p.K % 64 == 0 && p.lda % 8 == 0 &&
           p.ldw % 8 == 0 && p.N % 8 == 0 && p.a_gr == 0 && p.splitk <= 1 && !p.relu_in && p.epi == L4P_EPI_DENSE && !(p.tuning & 4) &&
           (long long)((p.M + 15) / 16) * ((p.N + 31) / 32) <= 512;
}
static int launch_skinny(const GemmParams& p, hipStream_t stream) {
    const int grid = ((p.M + 15) / 16) * ((p.N + 31) / 32);
    ProfScope prof(PROF_GEMM_SMALL, stream, "M%d N%d K%d epi%d act%d%s skinny", p.M, p.N, p.K, p.epi, p.act, p.w_gr > 0 ? " wgrp" : "");
    if (p.w_gr > 0)
        hipLaunchKernelGGL((gemm_skinny_kernel<GEMM_T, true>), dim3(grid), dim3(64), 0, stream, p);
    else
        hipLaunchKernelGGL((gemm_skinny_kernel<GEMM_T, false>), dim3(grid), dim3(64), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
// a problem the grouped launch takes: what GEMM_FN_impl would run on the four-stage 128x64 kernel
static bool gemm_is_small_deep(const GemmParams& p) {
    const long long t128 = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128), t64 = (long long)((p.M + 127) / 128) * ((p.N + 63) / 64);
    const bool big = (t128 >= 400 && !(t128 > 512 && t128 < 640)) || (p.splitk > 1 && p.N >= 256);
    return !big && p.splitk <= 1 && !p.relu_in && t64 <= 256 && p.K >= 6 * 64 && !(p.tuning & 1) && p.w_gr == 0;
}
int GEMM_GROUP_FN(const GemmParams* p, int n, hipStream_t stream) {
    for (int i = 0; i < n; ++i)  // (before anything is launched: a refused member leaves every output untouched)
        if (p[i].kw_cols > 0 && !kw_cols_ok(0, p[i])) return L4P_E_INVALID;
    const int deep = knob(KNOB_GEMM_DEEP);
    const int group = knob(KNOB_GEMM_GROUP);
    if (group && n >= 2 && n <= L4P_GEMM_GROUP_MAX) {  // all of them skinny: one launch of the one-wave kernel
        bool sk = true;
        long long waves = 0;
        for (int i = 0; sk && i < n; ++i) {
            sk = gemm_is_skinny(p[i]);
            waves += (long long)((p[i].M + 15) / 16) * ((p[i].N + 31) / 32);
        }
        if (sk && waves <= 1024) {  // (more: four waves and up to a CU - the staged grouped launch below)
            GemmGroupParams g;
            std::memset(&g, 0, sizeof(g));
            int first = 0;
            for (int i = 0; i < L4P_GEMM_GROUP_MAX; ++i) {
                g.first[i] = first;
                if (i < n) {
                    g.p[i] = p[i];
                    first += ((p[i].M + 15) / 16) * ((p[i].N + 31) / 32);
                } else {
                    g.first[i] = 0x7FFFFFFF;  // never selected
                }
            }
            g.first[L4P_GEMM_GROUP_MAX] = first;
            ProfScope prof(PROF_GEMM_SMALL, stream, "group of %d: M%d N%d K%d ... skinny", n, p[0].M, p[0].N, p[0].K);
            hipLaunchKernelGGL(gemm_skinny_group_kernel<GEMM_T>, dim3(first), dim3(64), 0, stream, g);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    bool ok = deep && group && n >= 2 && n <= L4P_GEMM_GROUP_MAX;
    long long total = 0;
    for (int i = 0; ok && i < n; ++i) {
        ok = gemm_is_small_deep(p[i]);
        total += (long long)((p[i].M + 127) / 128) * ((p[i].N + 63) / 64);
    }
    if (!ok || total > 512) {  // (more than two workgroups per CU's worth: nothing left to gain from sharing a launch)
        for (int i = 0; i < n; ++i) {
            const int rc = GEMM_FN(0, p[i], stream);
            if (rc) return rc;
        }
        return 0;
    }
    GemmGroupParams g;
    std::memset(&g, 0, sizeof(g));
    int first = 0;
    for (int i = 0; i < L4P_GEMM_GROUP_MAX; ++i) {
        g.first[i] = first;
        if (i < n) {
            g.p[i] = p[i];
            first += ((p[i].M + 127) / 128) * ((p[i].N + 63) / 64);
        } else {
            g.first[i] = 0x7FFFFFFF;  // never selected
        }
    }
    g.first[L4P_GEMM_GROUP_MAX] = first;
    constexpr int STAGES = 4;
    const size_t lds = STAGES * (128 + 64) * 128;
    auto kern = gemm_group_kernel<GEMM_T, 128, 64, 2, 2, true, STAGES>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof(p[0].M < 1024 ? PROF_GEMM_SMALL : PROF_GEMM, stream, "group of %d: M%d N%d K%d ... t128x64 deep", n, p[0].M, p[0].N, p[0].K);
    hipLaunchKernelGGL(kern, dim3(first), dim3(256), lds, stream, g);
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif
int GEMM_FN(int mode, const GemmParams& p_in, hipStream_t stream) {
    const int epi_generic = knob(KNOB_EPI_GENERIC);
    const bool maskdot_valu = p_in.epi == L4P_EPI_MASKDOT && !knob(KNOB_MASKDOT_MFMA);  // (A/B and parity aid: the all-VALU form)
    if (!epi_generic && !maskdot_valu) return GEMM_FN_impl(mode, p_in, stream);
    GemmParams p = p_in;
    if (epi_generic) p.tuning |= 1;
    if (maskdot_valu) p.tuning |= 4;
    return GEMM_FN_impl(mode, p, stream);
}
// Sub-pixel conv (l4p_conv3d_subpixel; arguments checked by launch_gemm): the 8-phase form where 256 x 256 tiles fill the chip - the
// dense decoders' levels 0 and 1 at batch 4: 32 x 32 and 32 x 8 tiles - else 128 x 128 tiles (gemm_variant: 1 = never 8-phase, 10 = always)
static int launch_subpixel(const GemmParams& p, hipStream_t stream) {
    int cells = 0, min_cells = 27;
    for (int s = 0; s < p.kt * p.kh * p.kw; ++s) {
        const int ks[3] = {p.kt, p.kh, p.kw}, ss[3] = {s / (p.kw * p.kh), (s / p.kw) % p.kh, s % p.kw};
        int n = 1;
        for (int a = 0; a < 3; ++a) n *= ks[a] == 1 ? 3 : (ss[a] == 0 || ss[a] == ks[a] - 1) ? 2 : 1;
        cells += n;
        min_cells = n < min_cells ? n : min_cells;
    }
    const int mean_k = (int)((long long)cells * p.Cin / (p.kt * p.kh * p.kw));
#ifdef GEMM_HAS_8P
    const int variant = knob(KNOB_GEMM_VARIANT);
    const long long t8 = (long long)((p.M + 255) / 256) * (p.N / 256);
    if (p.Cout % 256 == 0 && p.Cin % 64 == 0 && min_cells * (p.Cin / 64) >= 2 && variant != 1 && (variant == 10 || t8 >= 256))
        return launch_8p_subpixel(p, stream, mean_k);
#endif
    constexpr int BM = 128, BN = 128;
    const int ntm = (p.M + BM - 1) / BM, ntn = p.N / BN;
    const size_t lds = 2 * (BM + BN) * 128;
    auto kern = gemm_kernel<GEMM_T, BM, BN, 2, 2, 1, true, 2, false, true>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof(PROF_CONV3D, stream, "M%d N%d K%d epi%d act%d subpix t%dx%d", p.M, p.N, mean_k, L4P_EPI_CONVT, p.act, BM, BN);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn), dim3(256), lds, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int GEMM_FN_impl(int mode, const GemmParams& p, hipStream_t stream) {
    if (mode == 2) return launch_subpixel(p, stream);
    if (p.kw_cols > 0) {  // block-structured weights (l4p_gemm_desc.kw_cols): the LDS-staged kernels, whose k-tile range is per tile
        if (!kw_cols_ok(mode, p)) return L4P_E_INVALID;
        const long long t64 = (long long)((p.M + 127) / 128) * ((p.N + 63) / 64);
        if constexpr (sizeof(GEMM_T) == 2) {
            if (t64 <= 256) return launch_cfg<128, 64, 0, true, 4>(p, stream);
        }
        return launch_cfg<128, 64, 0, true>(p, stream);
    }
    if (p.w_gr > 0) {  // row-grouped weights (l4p_gemm_desc.w_gr): the 128-row-tile kernels, one instantiation per tile width
        if (mode != 0 || p.splitk > 1 || p.relu_in || p.w_gr % 128 || p.K % 8) {
            l4p_set_error("l4p_gemm: row-grouped weights need a dense GEMM without split-K, w_gr a multiple of 128");
            return L4P_E_INVALID;
        }
#ifdef GEMM_HAS_8P
        if (gemm_is_skinny_grouped(p)) return launch_skinny(p, stream);
        // a grid that leaves CUs idle (the folded score products of a rank's 8-track shard: 128 tiles of K = 1408) is bound by the
        // round trips of its k-tiles: four stages (three k-tiles in flight) instead of two; the same sums in the same order
        if (knob(KNOB_TRACK_DEEP) && p.N <= 64 && (long long)((p.M + 127) / 128) <= 256 && p.K >= 6 * 64) {
            // (at most 128 tiles of 128 rows - the 8-track shard: 16384 rows - leave half the chip idle: 64-row tiles)
            if ((p.M + 127) / 128 <= 128 && p.w_gr % 64 == 0) return launch_cfg<64, 64, 0, true, 4, 2, 2, true>(p, stream);
            return launch_cfg<128, 64, 0, true, 4, 2, 2, true>(p, stream);
        }
#endif
        return p.N <= 64 ? launch_cfg<128, 64, 0, true, 2, 2, 2, true>(p, stream) : launch_cfg<128, 128, 0, true, 2, 2, 2, true>(p, stream);
    }
#ifdef GEMM_HAS_8P
    if (mode == 0 && gemm_is_skinny(p)) return launch_skinny(p, stream);
#endif
    const long long t128 = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128);
    // 128x128 runs two workgroups per CU (512 slots on 256 CUs): a grid that spills less than a quarter of a second round
    // (the batch-1 QKV projection: 576 tiles) is better served by 128x64 tiles (measured 46 -> 41 us)
    // split-K problems (the low-resolution DPT convs, N >= 256): always the wider tile.  With 128x64 tiles four
    // co-resident workgroups per CU pull (128 + 64) x 64 operands per k-tile each and the launch is bound by L2
    // bandwidth (M = 8192, N = 256, K = 27648: 2.65 GB of tile loads in 250 us); 128x128 halves the bytes per FLOP
    // (250 -> 147 us, 77 -> 59 us, 133 -> 92 us on the c3 shapes).  The split count (splitk_for) assumes this.
    const bool big = (t128 >= 400 && !(t128 > 512 && t128 < 640)) || (p.splitk > 1 && p.N >= 256);
    const int variant = knob(KNOB_GEMM_VARIANT);
#ifdef GEMM_HAS_8P
    {
        // L4P_CONV_HALO=0: the implicit-GEMM forms for every conv (A/B aid)
        const int halo = knob(KNOB_CONV_HALO);  // (l4p_set_knob("conv_halo", ..): the tests switch forms inside one process)
        if (mode == 1 && p.ups_hi > 0) {  // up-sampling fused into the loader: the LDS-halo kernel or nothing
#ifdef L4P_PROBE_KERNELS
            if (conv_halo_fits<4, 2>(p)) return launch_halo<4, 2, true>(p, stream);
#else
            l4p_set_error("conv3d: the fused up-sampling loader (l4p_gemm_desc.ups_hi) is a measured-and-not-adopted form: build with PROBES=1");
            return L4P_E_INVALID;
#endif
            l4p_set_error("conv3d: the fused up-sampling loader takes N == 128, stride 1, Cin %% 32 == 0, whole 2 x 16 x 16 output blocks");
            return L4P_E_INVALID;
        }
        if (mode == 1 && halo && variant != 1) {
            if (conv_halo_fits<2, 4>(p)) return launch_halo<2, 4>(p, stream);
            if (conv_halo_fits<4, 2>(p)) return launch_halo<4, 2>(p, stream);
        }
    }
    if (p.splitk > 1 && mode == 0 && !p.relu_in && p.K % 8 == 0 && variant != 1 && p.N > 128) {
        // split-K on 256x256 tiles when the slices fill most of the chip exactly once (the batch-1 MLP-out projection:
        // 48 tiles x 4 slices = 192 workgroups of 24 k-tiles each, against 352 half-occupancy workgroups of 128x128 tiles:
        // 76.1 -> 72.0 us including the reduction pass; the float partials cost most of what the main loop gains)
        const long long w8 = (long long)((p.M + 255) / 256) * ((p.N + 255) / 256) * p.splitk;
        // (256 x 192 tiles when they fill the chip better in that one round: the same projection is 64 tiles x 4 slices = 256
        //  workgroups; L4P_GEMM_T192=0: A/B aid)
        const int t192sk = knob(KNOB_GEMM_T192);
        const long long w192 = (long long)((p.M + 255) / 256) * ((p.N + 191) / 192) * p.splitk;
        if (t192sk && w192 > w8 && w192 <= 256 && w8 >= 144 && p.K / p.splitk >= 512) return launch_8p<0, 4, 2, true, 4, 6>(p, stream);
        if (w8 >= 144 && w8 <= 256 && p.K / p.splitk >= 512) return launch_8p<0, 2, 4, true>(p, stream);
    }
    if (p.splitk <= 1 && !p.relu_in && p.K % 8 == 0 && variant != 1 && p.N > 128) {
        const long long t8 = (long long)((p.M + 255) / 256) * ((p.N + 255) / 256);
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
#ifdef L4P_PROBE_KERNELS
            const int g4w = knob(KNOB_GEMM_4W);  // (l4p_set_knob("gemm_4w", ..): the tests switch forms inside one process)
            const long long t4 = (long long)((p.M + 255) / 256) * ((p.N + 127) / 128);
            const bool pays = t4 >= 512 && (p.epi == L4P_EPI_MASKDOT || p.K <= 512 || (p.epi == L4P_EPI_QKV && t4 >= 1024));
            if (g4w && gemm4w_fits(p) && (g4w >= 2 || pays)) return launch_4w<false>(p, stream);
#endif
            // 256 x 192 tiles (wave tile 64 x 96) where they quantise better on the 256 CUs: rounds x outputs per tile
            // (the batch-4 encoder: out projection / MLP-out 192 tiles -> 256, QKV 576 -> 768; L4P_GEMM_T192=0: A/B aid)
            const int t192 = knob(KNOB_GEMM_T192);
            const long long n192 = (long long)((p.M + 255) / 256) * ((p.N + 191) / 192);
            const long long c256 = (t8 + 255) / 256 * 65536, c192 = (n192 + 255) / 256 * 49152;
            if (t192 && c192 < c256 && epilogue_is_lean_8p(p)) return launch_8p<0, 4, 2, false, 4, 6>(p, stream);
            return launch_8p<0, 2, 4>(p, stream);
        }
        if (use8 && mode == 1 && p.Cin % 64 == 0) return launch_8p<1, 2, 4>(p, stream);
    }
#ifdef GEMM_PROBE_VARIANTS
    if (variant == 11 && mode == 0) return launch_8p<0, 4, 2>(p, stream);  // 512x128: no better than 128x128 on the N = 128 convs
#endif
#endif
    if (mode == 0) {
#ifdef GEMM_PROBE_VARIANTS  // extra tile shapes compiled only into tools/probes/gemm_variants.hip
        if (variant == 4) return launch_cfg<256, 128, 0, true, 2, 4, 2>(p, stream);  // 8 waves, wave tile 64x64
        if (variant == 5) return launch_cfg<256, 128, 0, true, 2, 2, 2>(p, stream);  // 4 waves, wave tile 128x64
        if (variant == 9) return launch_cfg<128, 128, 0, true, 2, 2, 2>(p, stream);
#endif
        if (variant == 3) return launch_cfg<128, 64, 0, true>(p, stream);
        // Small problems (the tracker's token-side GEMMs: M = 6 x tracks rows against 1408 x 1408 weights that come from HBM /
        // the Infinity Cache every time): at most one workgroup per CU and a k-tile is a round trip of memory latency, not
        // of bandwidth, so the two-deep ring leaves the launch latency-bound (22 k-tiles x ~1 us).  Four stages keep three
        // k-tiles in flight (96 KB of LDS: irrelevant when the grid does not fill the chip anyway).  L4P_GEMM_DEEP=0: A/B aid.
        if (sizeof(GEMM_T) == 2 && !big && p.splitk <= 1) {
            const long long t64 = (long long)((p.M + 127) / 128) * ((p.N + 63) / 64);
            const int deep = knob(KNOB_GEMM_DEEP);
            if (deep && t64 <= 256 && p.K >= 6 * 64) return launch_cfg<128, 64, 0, true, 4>(p, stream);
            // (between one and two rounds of 128 x 64 tiles - the batch-1 encoder's attention projection, 352 tiles: the four-stage form on
            //  128 x 128 tiles, one workgroup per CU, was measured at +0.2 % on configs[1] (1561 -> 1564 frames/s, two alternations): not kept)
        }
        return big ? launch_cfg<128, 128, 0, true>(p, stream) : launch_cfg<128, 64, 0, true>(p, stream);
    }
    if (p.relu_in) return big ? launch_cfg<128, 128, 1, false>(p, stream) : launch_cfg<128, 64, 1, false>(p, stream);
    return big ? launch_cfg<128, 128, 1, true>(p, stream) : launch_cfg<128, 64, 1, true>(p, stream);
}
