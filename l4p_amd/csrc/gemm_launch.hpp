// The GEMM / conv launches, as templates on the element type: gemm_select.hpp names the kernel form, this file starts it.
// gemm_bf16.hip / gemm_f16.hip / gemm_f32.hip instantiate launch_gemm_typed (and, 16-bit, launch_gemm_group_typed) explicitly.
#pragma once
#include <cstdlib>
#include <cstring>

#include "gemm.hpp"
#include "gemm8p.hpp"
#ifdef L4P_PROBE_KERNELS  // (measured, not adopted: only in a PROBES=1 build)
#include "gemm4w.hpp"
#endif
#include "conv3_halo.hpp"
#include "gemm_select.hpp"
#include "gemm_skinny.hpp"
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
// ... launched behind every split-K form (tuning bit 1: the caller sums the partials itself)
template <typename T>
static void launch_splitk_finish(const GemmParams& p, int nsplit, hipStream_t stream) {
    if (nsplit <= 1 || (p.tuning & 2)) return;
    const long long total = (long long)p.M * (p.N / 8);
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(splitk_finish_kernel<T>, dim3(grid), dim3(256), 0, stream, p);
}

// The profiler scope of a launch: "M%d N%d K%d epi%d act%d " + the form's name (gemm_select.hpp).  K: the sub-pixel forms show their
// mean executed K.  (C++17: the scope is constructed in the caller's frame.  Profiling off: the untagged scope, whose constructor
// inlines - the tagged one is a variadic call.)
static inline ProfScope gemm_prof(int cls, hipStream_t stream, const GemmParams& p, int K, GemmForm form, int nsplit = 1) {
    if (!g_prof_on) return ProfScope(cls, stream);
    char buf[GEMM_TAG_MAX];
    return ProfScope(cls, stream, "M%d N%d K%d epi%d act%d %s", p.M, p.N, K, p.epi, p.act, gemm_form_tag(form, nsplit, buf));
}

// LDS-staged kernel (gemm.hpp)
template <typename T, int BM, int BN, int MODE, bool GLDS, int STAGES = 2, bool GROUPW = false>
static int launch_cfg(const GemmParams& p, hipStream_t stream, GemmForm form) {
    constexpr int WM = 2, WN = 2;
    const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
    const int nsplit = p.splitk > 1 ? p.splitk : 1;
    const size_t lds = STAGES * (BM + BN) * 128;
    auto kern = gemm_kernel<T, BM, BN, WM, WN, MODE, GLDS, STAGES, GROUPW>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof = gemm_prof(MODE == 0 ? (p.w_gr > 0 || p.M < 1024 ? PROF_GEMM_SMALL : PROF_GEMM) : PROF_CONV3D, stream, p, p.K, form, nsplit);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn * nsplit), dim3(WM * WN * 64), lds, stream, p);
    launch_splitk_finish<T>(p, nsplit, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Sub-pixel conv (l4p_conv3d_subpixel) on the staged kernel, 128 x 128 tiles
template <typename T>
static int launch_subpixel(const GemmParams& p, hipStream_t stream, GemmForm form) {
    constexpr int BM = 128, BN = 128;
    const int ntm = (p.M + BM - 1) / BM, ntn = p.N / BN;
    const size_t lds = 2 * (BM + BN) * 128;
    auto kern = gemm_kernel<T, BM, BN, 2, 2, 1, true, 2, false, true>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof = gemm_prof(PROF_CONV3D, stream, p, subpixel_mean_k(p), form);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn), dim3(256), lds, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// 8-phase deep-pipelined kernel (gemm8p.hpp), 16-bit only, no fused input ReLU
template <typename T, int MODE, int WR, int WC, bool SPLITK = false, int TM = 8, int TN = 4, bool TWOPH = false>
static int launch_8p(const GemmParams& p, hipStream_t stream, GemmForm form) {
    typedef Gemm8pCfg<WR, WC, TM, TN> Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
    const int nsplit = SPLITK ? p.splitk : 1;
    const size_t lds = Cfg::LDS_BYTES;
    auto kern = gemm8p_kernel<T, MODE, WR, WC, SPLITK, TM, TN, false, false, TWOPH>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof = gemm_prof(MODE == 0 ? PROF_GEMM : PROF_CONV3D, stream, p, p.K, form, nsplit);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn * nsplit), dim3(512), lds, stream, p);
    launch_splitk_finish<T>(p, nsplit, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
// sub-pixel conv on the 8-phase kernel
template <typename T>
static int launch_8p_subpixel(const GemmParams& p, hipStream_t stream, GemmForm form) {
    typedef Gemm8pCfg<2, 4, 8, 4> Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = p.N / Cfg::BN;
    auto kern = gemm8p_kernel<T, 1, 2, 4, false, 8, 4, false, true>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)Cfg::LDS_BYTES));
    ProfScope prof = gemm_prof(PROF_CONV3D, stream, p, subpixel_mean_k(p), form);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn), dim3(512), Cfg::LDS_BYTES, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

#ifdef L4P_PROBE_KERNELS
// Two-workgroups-per-CU form (gemm4w.hpp)
template <typename T, bool SPLITK>
static int launch_4w(const GemmParams& p, hipStream_t stream, GemmForm form) {
    typedef Gemm4wCfg Cfg;
    const int ntm = (p.M + Cfg::BM - 1) / Cfg::BM, ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
    const int nsplit = SPLITK ? p.splitk : 1;
    auto kern = gemm4w_kernel<T, SPLITK>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, Cfg::LDS_BYTES));
    ProfScope prof = gemm_prof(PROF_GEMM, stream, p, p.K, form, nsplit);
    hipLaunchKernelGGL(kern, dim3(ntm * ntn * nsplit), dim3(256), Cfg::LDS_BYTES, stream, p);
    launch_splitk_finish<T>(p, nsplit, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

// LDS-halo 3x3x3 conv (conv3_halo.hpp)
template <typename T, int WR, int WC, bool UPS = false, bool TWO_PHASE = UPS>
static int launch_halo(const GemmParams& p, hipStream_t stream, GemmForm form) {
    typedef ConvHaloCfg<WR, WC> Cfg;
    typedef ConvHaloTile<WR, WC> Tile;  // (what conv_halo_fits checked the volume against)
    static_assert(Cfg::BM == Tile::BM && Cfg::BN == Tile::BN && Cfg::TT == Tile::TT && Cfg::TH == Tile::TH && Cfg::TW == Tile::TW, "gemm_select.hpp");
    static_assert(TWO_PHASE || !UPS, "the fused up-sampling loader exists on the two-phase body only");
    auto kern = TWO_PHASE ? conv3_halo2p_kernel<T, WR, WC, UPS> : conv3_halo_kernel<T, WR, WC, false>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, Cfg::LDS_BYTES));
    ProfScope prof = gemm_prof(PROF_CONV3D, stream, p, p.K, form);
    hipLaunchKernelGGL(kern, dim3(p.M / Cfg::BM), dim3(512), Cfg::LDS_BYTES, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// one-wave kernel (gemm_skinny.hpp)
template <typename T, bool GROUPW>
static int launch_skinny(const GemmParams& p, hipStream_t stream, GemmForm form) {
    const int grid = ((p.M + 15) / 16) * ((p.N + 31) / 32);
    ProfScope prof = gemm_prof(PROF_GEMM_SMALL, stream, p, p.K, form);
    hipLaunchKernelGGL((gemm_skinny_kernel<T, GROUPW>), dim3(grid), dim3(64), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

static GemmKnobs gemm_knobs() {
    GemmKnobs k;
    k.gemm_variant = knob(KNOB_GEMM_VARIANT), k.conv_halo = knob(KNOB_CONV_HALO), k.gemm_skinny = knob(KNOB_GEMM_SKINNY);
    k.skinny_max_m = knob(KNOB_SKINNY_MAX_M), k.gemm_deep = knob(KNOB_GEMM_DEEP), k.gemm_group = knob(KNOB_GEMM_GROUP);
    k.track_deep = knob(KNOB_TRACK_DEEP), k.gemm_t192 = knob(KNOB_GEMM_T192), k.gemm_4w = knob(KNOB_GEMM_4W);
#ifdef L4P_PROBE_KERNELS
    k.probe_kernels = 1;
#else
    k.probe_kernels = 0;
#endif
    k.gemm_8p_body = knob(KNOB_GEMM_8P_BODY);
    return k;
}

template <typename T>
static int launch_form(GemmForm form, const GemmParams& p, hipStream_t stream) {
    switch (form) {
        case GEMM_STAGED_128x64: return launch_cfg<T, 128, 64, 0, true>(p, stream, form);
        case GEMM_STAGED_128x64_DEEP: return launch_cfg<T, 128, 64, 0, true, 4>(p, stream, form);
        case GEMM_STAGED_128x128: return launch_cfg<T, 128, 128, 0, true>(p, stream, form);
        case GEMM_WGRP_128x64: return launch_cfg<T, 128, 64, 0, true, 2, true>(p, stream, form);
        case GEMM_WGRP_128x128: return launch_cfg<T, 128, 128, 0, true, 2, true>(p, stream, form);
        case GEMM_CONV_128x64: return launch_cfg<T, 128, 64, 1, true>(p, stream, form);
        case GEMM_CONV_128x128: return launch_cfg<T, 128, 128, 1, true>(p, stream, form);
        case GEMM_CONV_RELU_128x64: return launch_cfg<T, 128, 64, 1, false>(p, stream, form);
        case GEMM_CONV_RELU_128x128: return launch_cfg<T, 128, 128, 1, false>(p, stream, form);
        case GEMM_SUBPIX_STAGED: return launch_subpixel<T>(p, stream, form);
        default: break;
    }
    if constexpr (sizeof(T) == 2) {
        switch (form) {
            case GEMM_WGRP_64x64_DEEP: return launch_cfg<T, 64, 64, 0, true, 4, true>(p, stream, form);
            case GEMM_WGRP_128x64_DEEP: return launch_cfg<T, 128, 64, 0, true, 4, true>(p, stream, form);
            // (the plain enumerators: the body gemm_8p_two_phase names for the shape; _2PH / _4PH: knob gemm_8p_body)
            case GEMM_8P_256x256:
                return gemm_8p_two_phase(p, form) ? launch_8p<T, 0, 2, 4, false, 8, 4, true>(p, stream, form) : launch_8p<T, 0, 2, 4>(p, stream, form);
            case GEMM_8P_256x192:
                return gemm_8p_two_phase(p, form) ? launch_8p<T, 0, 4, 2, false, 4, 6, true>(p, stream, form)
                                                  : launch_8p<T, 0, 4, 2, false, 4, 6>(p, stream, form);
            case GEMM_8P_2PH_256x256: return launch_8p<T, 0, 2, 4, false, 8, 4, true>(p, stream, form);
            case GEMM_8P_2PH_256x192: return launch_8p<T, 0, 4, 2, false, 4, 6, true>(p, stream, form);
            case GEMM_8P_4PH_256x256: return launch_8p<T, 0, 2, 4>(p, stream, form);
            case GEMM_8P_4PH_256x192: return launch_8p<T, 0, 4, 2, false, 4, 6>(p, stream, form);
            case GEMM_8P_SK_256x256: return launch_8p<T, 0, 2, 4, true>(p, stream, form);
            case GEMM_8P_SK_256x192: return launch_8p<T, 0, 4, 2, true, 4, 6>(p, stream, form);
            case GEMM_8P_CONV: return launch_8p<T, 1, 2, 4>(p, stream, form);
            case GEMM_HALO_2x4: return launch_halo<T, 2, 4>(p, stream, form);
            case GEMM_HALO_4x2: return launch_halo<T, 4, 2>(p, stream, form);
            case GEMM_HALO_2x4_2P: return launch_halo<T, 2, 4, false, true>(p, stream, form);
            case GEMM_HALO_4x2_2P: return launch_halo<T, 4, 2, false, true>(p, stream, form);
            case GEMM_SKINNY: return launch_skinny<T, false>(p, stream, form);
            case GEMM_SKINNY_WGRP: return launch_skinny<T, true>(p, stream, form);
            case GEMM_SUBPIX_8P: return launch_8p_subpixel<T>(p, stream, form);
#ifdef L4P_PROBE_KERNELS
            case GEMM_HALO_4x2_UPS: return launch_halo<T, 4, 2, true>(p, stream, form);
            case GEMM_4W: return launch_4w<T, false>(p, stream, form);
#endif
            default: break;
        }
    }
    l4p_set_error("gemm: kernel form %d does not exist for this element type in this build", (int)form);
    return L4P_E_INVALID;
}

template <typename T>
int launch_gemm_typed(int mode, const GemmParams& p_in, hipStream_t stream) {
    // the tuning bits of two knobs, in front of the selection: it sees the effective descriptor
    const int epi_generic = knob(KNOB_EPI_GENERIC);
    const bool maskdot_valu = p_in.epi == L4P_EPI_MASKDOT && !knob(KNOB_MASKDOT_MFMA);  // (A/B and parity aid: the all-VALU form)
    GemmParams patched;
    const GemmParams* p = &p_in;
    if (epi_generic || maskdot_valu) {
        patched = p_in;
        if (epi_generic) patched.tuning |= 1;
        if (maskdot_valu) patched.tuning |= 4;
        p = &patched;
    }
    const char* err = nullptr;
    const GemmForm form = gemm_select(mode, (int)sizeof(T), *p, gemm_knobs(), &err);
    if (form == GEMM_FORM_INVALID) {
        l4p_set_error("%s", err);
        return L4P_E_INVALID;
    }
    return launch_form<T>(form, *p, stream);
}

// members [0, n) and the first workgroup of each (bm x bn output blocks per workgroup); returns the grid
static int fill_group(GemmGroupParams& g, const GemmParams* p, int n, int bm, int bn) {
    std::memset(&g, 0, sizeof(g));
    int first = 0;
    for (int i = 0; i < L4P_GEMM_GROUP_MAX; ++i) {
        g.first[i] = first;
        if (i < n) {
            g.p[i] = p[i];
            first += ((p[i].M + bm - 1) / bm) * ((p[i].N + bn - 1) / bn);
        } else {
            g.first[i] = 0x7FFFFFFF;  // never selected
        }
    }
    g.first[L4P_GEMM_GROUP_MAX] = first;
    return first;
}

// l4p_gemm_group on a 16-bit type (launch_gemm_group has checked the members)
template <typename T>
int launch_gemm_group_typed(const GemmParams* p, int n, hipStream_t stream) {
    static_assert(sizeof(T) == 2, "the grouped kernels exist for the 16-bit types");
    const char* err = nullptr;
    const GemmGroupForm form = gemm_group_select(p, n, gemm_knobs(), &err);
    if (form == GEMM_GROUP_INVALID) {
        l4p_set_error("%s", err);
        return L4P_E_INVALID;
    }
    if (form == GEMM_GROUP_ONE_BY_ONE) {
        for (int i = 0; i < n; ++i) {
            const int rc = launch_gemm_typed<T>(0, p[i], stream);
            if (rc) return rc;
        }
        return 0;
    }
    GemmGroupParams g;
    if (form == GEMM_GROUP_SKINNY) {
        const int grid = fill_group(g, p, n, 16, 32);
        ProfScope prof(PROF_GEMM_SMALL, stream, "group of %d: M%d N%d K%d ... %s", n, p[0].M, p[0].N, p[0].K, gemm_group_tag(form));
        hipLaunchKernelGGL(gemm_skinny_group_kernel<T>, dim3(grid), dim3(64), 0, stream, g);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int grid = fill_group(g, p, n, 128, 64);
    constexpr int STAGES = 4;
    const size_t lds = STAGES * (128 + 64) * 128;
    auto kern = gemm_group_kernel<T, 128, 64, 2, 2, true, STAGES>;
    static lds_attr_state attr_done;
    HIP_TRY(lds_attr_once(attr_done, kern, (int)lds));
    ProfScope prof(p[0].M < 1024 ? PROF_GEMM_SMALL : PROF_GEMM, stream, "group of %d: M%d N%d K%d ... %s", n, p[0].M, p[0].N, p[0].K, gemm_group_tag(form));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, g);
    HIP_TRY(hipGetLastError());
    return 0;
}
