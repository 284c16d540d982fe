#include "gemm.hpp"

// the element type's instantiation of the launcher (gemm_launch.hpp)
static int launch_gemm_of(int dtype, int mode, const GemmParams& p, hipStream_t stream) {
    return dtype == L4P_BF16 ? launch_gemm_typed<bf16_t>(mode, p, stream)
           : dtype == L4P_F16 ? launch_gemm_typed<f16_t>(mode, p, stream)
                              : launch_gemm_typed<float>(mode, p, stream);
}

// l4p_conv3d_subpixel (mode 2): the arguments the kernels rely on, then the conv descriptor they read (output grid == input grid, stride 1)
static int launch_subpixel_checked(int dtype, const GemmParams& d, hipStream_t stream) {
    const int es = esize_of(dtype);
    GemmParams p = d;
    const long long ksub = (long long)p.kt * p.kh * p.kw;
    if (p.kt < 1 || p.kh < 1 || p.kw < 1 || ksub < 2 || ksub > 64 || p.Ti < 1 || p.Hi < 1 || p.Wi < 1 || p.Cin < 1 || p.Cout < 1 || p.M <= 0) {
        l4p_set_error("conv3d_subpixel: needs strides kt, kh, kw >= 1 (at least one axis up-scaled, at most 64 sub-positions), a grid and channels");
        return L4P_E_INVALID;
    }
    const int cells = (p.kt == 1 ? 3 : 2) * (p.kh == 1 ? 3 : 2) * (p.kw == 1 ? 3 : 2);
    if (p.Cin % (128 / es) || p.Cout % 128 || p.N != ksub * p.Cout || p.M % (p.Ti * p.Hi * p.Wi) || p.ldw < (long long)cells * p.Cin || (p.ldw * es) % 16) {
        l4p_set_error("conv3d_subpixel: Cin %% %d, Cout %% 128, N == kt*kh*kw*Cout, M == B*Ti*Hi*Wi, ldw >= %d*Cin", 128 / es, cells);
        return L4P_E_INVALID;
    }
    if (p.Ti * p.kt < 2 || p.Hi * p.kh < 2 || p.Wi * p.kw < 2) {
        l4p_set_error("conv3d_subpixel: every up-scaled axis must be at least 2 long (three border classes per axis)");
        return L4P_E_INVALID;
    }
    if (!p.out_T || p.out_f32 || p.res1 || p.res2 || p.act != L4P_ACT_NONE || p.relu_in || p.splitk > 1 || p.a_gr > 0 || p.c_gr > 0 || p.w_gr > 0 ||
        p.kw_cols > 0 || p.ups_hi > 0 || (long long)p.M * ksub * p.Cout >= (1ll << 40)) {
        l4p_set_error("conv3d_subpixel: out_T (+ out_relu_T) only: no residual, activation, split-K, row maps or grouped weights");
        return L4P_E_INVALID;
    }
    p.To = p.Ti, p.Ho = p.Hi, p.Wo = p.Wi;
    p.st = p.sh = p.sw = 1;
    p.K = (int)p.ldw;
    p.epi = L4P_EPI_CONVT;
    return launch_gemm_of(dtype, 2, p, stream);
}

int launch_gemm(int dtype, int mode, const GemmParams& p, hipStream_t stream) {
    if (!dtype_ok(dtype)) { l4p_set_error("gemm: unknown dtype %d", dtype); return L4P_E_INVALID; }
    if (mode == 2) return launch_subpixel_checked(dtype, p, stream);
    const int es = esize_of(dtype);
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) { l4p_set_error("gemm: empty problem M=%d N=%d K=%d", p.M, p.N, p.K); return L4P_E_INVALID; }
    if (p.N % 8) { l4p_set_error("gemm: N=%d must be a multiple of 8", p.N); return L4P_E_INVALID; }
    if ((p.K * es) % 16 || (p.ldw * es) % 16) { l4p_set_error("gemm: K/ldw not 16-byte aligned"); return L4P_E_INVALID; }
    if (mode == 0 && (p.lda * es) % 16) { l4p_set_error("gemm: lda not 16-byte aligned"); return L4P_E_INVALID; }
    if (mode == 1 && (p.Cin % (128 / es) || p.K != 27 * p.Cin)) { l4p_set_error("conv3d: Cin=%d must be a multiple of %d and K=27*Cin", p.Cin, 128 / es); return L4P_E_INVALID; }
    if (p.ups_hi > 0 && (mode != 1 || !is16(dtype) || p.ups_wi <= 0 || p.To != p.Ti)) {
        l4p_set_error("conv3d: the fused up-sampling loader (ups_hi / ups_wi) exists for l4p_conv3d_k3 on the 16-bit engines, time axis not resized");
        return L4P_E_INVALID;
    }
    if (p.splitk > 1) {
        const int bk = 128 / es, nk = (p.K + bk - 1) / bk;
        if (p.epi != L4P_EPI_DENSE || !p.partial || p.splitk > nk || p.c_gr > 0) {
            l4p_set_error("gemm: split-K needs the dense epilogue, a partial buffer and splitk <= %d k-tiles", nk);
            return L4P_E_INVALID;
        }
    }
    return launch_gemm_of(dtype, mode, p, stream);
}

int launch_gemm_group(int dtype, const GemmParams* p, int n, hipStream_t stream) {
    if (!p || n < 1 || n > L4P_GEMM_GROUP_MAX) {
        l4p_set_error("gemm_group: 1 <= n <= %d descriptors", L4P_GEMM_GROUP_MAX);
        return L4P_E_INVALID;
    }
    if (is16(dtype)) {
        for (int i = 0; i < n; ++i) {  // the checks of launch_gemm that the fast path would skip
            if (p[i].M <= 0 || p[i].N <= 0 || p[i].K <= 0 || p[i].N % 8 || (p[i].K * 2) % 16 || (p[i].ldw * 2) % 16 || (p[i].lda * 2) % 16 ||
                p[i].splitk > 1)
                goto one_by_one;
        }
        return dtype == L4P_F16 ? launch_gemm_group_typed<f16_t>(p, n, stream) : launch_gemm_group_typed<bf16_t>(p, n, stream);
    }
one_by_one:
    for (int i = 0; i < n; ++i) {
        const int rc = launch_gemm(dtype, 0, p[i], stream);
        if (rc) return rc;
    }
    return 0;
}
