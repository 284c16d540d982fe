// The device pieces attn_kernel (attention.hip) and attn64_kernel (attention64.hip) share: the constant chunks of a tile, where the
// padding of the head dim carries the denominator and the deferred maximum, the tile walk and the store tail.  Operand layouts: the
// comment at the top of attention.hip.  Each kernel keeps its own fragment addresses (K-row bit swap, koff, va), issue_q and
// move-the-reference arithmetic, and attn_kernel the padding predicate of its query-split requests: written as functions here, the
// same expressions compile to other instruction text ("Attention: one pure form selection").
#pragma once
#include <type_traits>

#include "attn_select.hpp"
#include "common.hpp"
#include "static_for.hpp"

// ---- the constant 16-byte chunks a tile copy substitutes for padding ----
// row DH of a V^T tile reads ones: O^T[DH][q] = sum_k P[q][k], the softmax denominator with exactly the weights used for O
__device__ __attribute__((aligned(16))) static const unsigned short g_ones_bf16[8] = {0x3F80, 0x3F80, 0x3F80, 0x3F80,
                                                                                         0x3F80, 0x3F80, 0x3F80, 0x3F80};
__device__ __attribute__((aligned(16))) static const unsigned short g_ones_f16[8] = {0x3C00, 0x3C00, 0x3C00, 0x3C00,
                                                                                        0x3C00, 0x3C00, 0x3C00, 0x3C00};
__device__ __attribute__((aligned(16))) static const float g_ones_f32[4] = {1.f, 1.f, 1.f, 1.f};
// K-tile chunk holding head dims DH .. DH+7 (all padding) in the deferred-maximum form: dims DH and DH+1 read as 1.0, so
// the two 16-bit halves of -m that sit in the same dims of Q are added to every score by the QK^T MFMA itself
__device__ __attribute__((aligned(16))) static const unsigned short g_kone_bf16[8] = {0x3F80, 0x3F80, 0, 0, 0, 0, 0, 0};
__device__ __attribute__((aligned(16))) static const unsigned short g_kone_f16[8] = {0x3C00, 0x3C00, 0, 0, 0, 0, 0, 0};
template <typename T>
__device__ __forceinline__ const char* attn_ones_chunk() {
    return std::is_same<T, f16_t>::value ? (const char*)g_ones_f16 : sizeof(T) == 2 ? (const char*)g_ones_bf16 : (const char*)g_ones_f32;
}
template <typename T>
__device__ __forceinline__ const char* attn_kone_chunk() {
    return std::is_same<T, f16_t>::value ? (const char*)g_kone_f16 : (const char*)g_kone_bf16;
}
// chunk c of a K tile is (k-step c / (2 KVB), key (c % (2 KVB)) / 2, half (c & 1) ^ ((key >> 3) & 1)): is it head dims DH .. DH+7?
template <int KVB, int DH>
__device__ __forceinline__ bool attn_k_chunk_is_pad(int c) {
    const int key = (c % (2 * KVB)) >> 1;
    return (c / (2 * KVB)) * 16 + (((c & 1) ^ ((key >> 3) & 1)) << 3) == DH;
}
// where the padding lands in the registers: the denominator row DH of O^T (d tile DT_L, register R_L of lane half HI_L; a lane holds
// d = 32 dt + (r & 3) + 8 (r >> 2) + 4 hi) and the Q fragment with dims DH .. DH+7 (k-step KS_P of lane half HI_P)
template <int DH>
struct AttnPad {
    static_assert(DH % 8 == 0 && DH < ATTN_DP, "the first padding chunk starts at DH and carries -m / the denominator");
    static constexpr int I_L = DH % 32;
    static constexpr int DT_L = DH / 32, HI_L = (I_L >> 2) & 1, R_L = (I_L & 3) + 4 * (I_L >> 3);
    static constexpr int KS_P = DH / 16, HI_P = (DH / 8) & 1;
};

// XCD-aware work mapping: workgroup L runs on XCD L % 8 (observed dispatch order; speed only, not correctness).  All nqb query blocks
// of one (batch, head) are given to the SAME XCD so that head's K / V^T (786 KB) is fetched into one L2 instead of eight.
// tile v -> (batch * H + head, first query row of the tile: batch * S + token); units = B * H
template <int QROWS>
__device__ __forceinline__ void attn_tile_decode(int v, int nqb, int units, int H, int S, int& bh_, int& qrow0_) {
    int unit, qb;
    if ((units & 7) == 0) {
        const int xcd = v & 7, j = v >> 3;
        unit = xcd + 8 * (j / nqb);
        qb = j % nqb;
    } else {
        unit = v / nqb;
        qb = v % nqb;
    }
    bh_ = unit;
    qrow0_ = (unit / H) * S + qb * QROWS;
}

// The store tail of a 16-bit output row.  The row is split across the half-waves in 4-column pieces (lane: columns 8k + 4hi .. + 3 of
// every 8-column group k, packed in pk[k]).  One v_permlane32_swap per dword of a group PAIR (k, k+1) hands the upper half's group-k
// piece down and the lower half's group-(k+1) piece up: lanes 0-31 then hold columns 8k .. 8k+7, lanes 32-63 columns 8k+8 .. 8k+15 ->
// one 16-byte store per pair instead of two 8-byte ones (the store tail is bound by the number of store instructions, not by bytes).
template <int NG, typename T>
__device__ __forceinline__ void attn_store_row16(T* op, const u32x2 (&pk)[NG], int hi) {
#pragma unroll
    for (int k = 0; k + 1 < NG; k += 2) {
        const auto x = __builtin_amdgcn_permlane32_swap(pk[k][0], pk[k + 1][0], false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(pk[k][1], pk[k + 1][1], false, false);
        *(u32x4*)(op + 8 * k + 8 * hi) = (u32x4){x[0], y[0], x[1], y[1]};
    }
    if constexpr (NG & 1) *(u32x2*)(op + 8 * (NG - 1) + 4 * hi) = pk[NG - 1];
}
