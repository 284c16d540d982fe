// MFMA GEMM / implicit-GEMM conv3d for gfx950.
//
//   out[m][n] = epilogue( sum_k A[m][k] * W[n][k] )        (both operands k-contiguous)
//
// One kernel template serves: the encoder linears (reference modeling_finetune.py:169-190, :62-69),
// the patch-embed GEMM (:276-283), every Conv3d 1x1x1 / 3x3x3 and ConvTranspose3d k==stride of the
// DPT decoders (dpt_block.py:29-90,93-157,255-278,406-414) and the SAM-style tracker's projections
// (sam/transformer.py:223-245, mask_decoder.py:58-66).
//
// CDNA4 mapping:
//  * operands are swapped into the MFMA (weights = A operand, activations = B operand) so that a lane
//    ends up with 4*TN *consecutive output columns of one row*: bias / residual / store are 16-byte
//    vector accesses and every output row is written in 64..256-byte runs.
//  * LDS tiles have 128-byte rows, XOR-swizzled at 16-byte granularity (chunk ^= (row>>1)&7) so the
//    non-contiguous 16-lane groups of ds_read_b128 hit 16 distinct slots.
//  * tiles are staged by LDS-DMA (global_load_lds, 16 B per lane, swizzle applied to the per-lane SOURCE chunk);
//    the register-staged loader remains for the conv path with a fused input ReLU.  Next tile's loads are issued
//    before the current tile's MFMAs (double-buffered LDS, one barrier per k-tile).
//  * T = bf16 uses v_mfma_f32_16x16x32_bf16, T = float uses 8x v_mfma_f32_16x16x4_f32 on the same
//    fragment registers (exact-f32 parity mode).
#pragma once
#include "common.hpp"
#include "static_for.hpp"

#include <type_traits>

enum { EPI_DENSE = L4P_EPI_DENSE, EPI_QKV = L4P_EPI_QKV, EPI_CONVT = L4P_EPI_CONVT, EPI_MASKDOT = L4P_EPI_MASKDOT };
enum { ACT_NONE = L4P_ACT_NONE, ACT_GELU = L4P_ACT_GELU, ACT_RELU = L4P_ACT_RELU };

// The kernel parameter block IS the public descriptor (include/l4p_hip.h): plain pointers and ints.
typedef l4p_gemm_desc GemmParams;

// 16 zero bytes in global memory: the source of LDS-DMA chunks that must read as zero (conv padding, k tail)
__device__ __attribute__((aligned(16))) static const unsigned g_zero_chunk[4] = {0u, 0u, 0u, 0u};

// the addressing arithmetic every kernel form shares, and the epilogues (they read GemmParams and the enums above)
#include "gemm_tile.hpp"
#include "gemm_epilogue.hpp"

// GLDS = true: tiles are staged with global_load_lds (LDS-DMA, no VGPR round trip, no ds_write); the LDS image is
// lane-linear, so the XOR swizzle is applied to the per-lane SOURCE chunk and again on the fragment reads.
// GLDS = false: global -> register -> ds_write staging (needed for the fused input ReLU of the conv loader).
// STAGES = 3 (LDS-DMA only): two k-tiles stay in flight; the per-iteration wait is a COUNTED s_waitcnt vmcnt(loads of one
// tile) followed by a raw s_barrier, so the next tile's DMA is not drained at the barrier (a __syncthreads() would emit
// vmcnt(0)).  Order per iteration: wait(own loads of tile kt) -> barrier (everyone's tile kt landed, everyone finished
// reading tile kt-1) -> issue tile kt+2 into the buffer tile kt-1 used -> MFMAs on tile kt.
// (the kernel body is a device function of (descriptor, workgroup index): gemm_kernel runs it for one problem,
//  gemm_group_kernel for up to four problems in ONE launch, see below)
// GROUPW: row-grouped weights (l4p_gemm_desc.w_gr): the tile's row group selects the weight matrix and the bias row.  Its own
// instantiation - the descriptor is copied and patched per workgroup, which the plain kernels must not pay for.
// SUBPIX (MODE 1, LDS-DMA): the sub-pixel conv (see subpix_cells above): the k-loop walks the active cells of the tile's sub-position.
template <typename T, int BM, int BN, int WM, int WN, int MODE, bool GLDS, int STAGES = 2, bool GROUPW = false, bool SUBPIX = false>
__device__ __forceinline__ void gemm_body(const GemmParams& p_in, const int wg_index) {
    static_assert(STAGES == 2 || (STAGES >= 3 && STAGES <= 5 && GLDS), "deeper pipelines need LDS-DMA staging");
    static_assert(!GROUPW || MODE == 0, "row-grouped weights: dense GEMM");
    static_assert(!SUBPIX || (MODE == 1 && GLDS && STAGES == 2), "sub-pixel conv: the LDS-DMA conv form");
    GemmParams patched;
    const GemmParams* pp = &p_in;
    if constexpr (GROUPW) {
        const int ntn_ = (p_in.N + BN - 1) / BN;
        const int grp = ((wg_index / ntn_) * BM) / p_in.w_gr;  // (no split-K, no XCD remap in MODE 0: tile = wg_index, m-major)
        patched = p_in;
        patched.W = (const T*)p_in.W + (long long)grp * p_in.w_gs;
        if (p_in.bias) patched.bias = p_in.bias + (long long)grp * p_in.b_gs;
        if (p_in.o_gs) {
            if (p_in.out_T) patched.out_T = (T*)p_in.out_T + (long long)grp * p_in.o_gs;
            if (p_in.out_f32) patched.out_f32 = p_in.out_f32 + (long long)grp * p_in.o_gs;
        }
        pp = &patched;
    }
    const GemmParams& p = *pp;
    constexpr int NT = WM * WN * 64;
    constexpr int ES = sizeof(T);
    constexpr int BK = 128 / ES;   // 64 bf16 / 32 f32 per LDS row
    constexpr int EPC = 16 / ES;   // elements per 16-byte chunk
    constexpr int CPF = 8 * ES / 16;  // chunks per fragment (1 bf16, 2 f32)
    constexpr int KK = BK / 32;
    constexpr int A_IT = BM * 8 / NT, W_IT = BN * 8 / NT;
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    typedef typename Frag<T>::type frag_t;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                       // [STAGES][BM*128]
    char* Ws = smem + STAGES * BM * 128;   // [STAGES][BN*128]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ntn = (p.N + BN - 1) / BN;
    const int ntiles = ntn * ((p.M + BM - 1) / BM);
    const int ksplit = wg_index / ntiles;  // split-K slice of this workgroup
    int tile = wg_index - ksplit * ntiles;
    if (MODE == 1 && p.splitk <= 1) tile = xcd_tile(tile, ntiles);  // conv: XCD-contiguous tile ranges (workgroup b runs on XCD b % 8)
    int mt = tile / ntn;
    const int nt = tile % ntn;
    if (MODE == 1 && p.splitk <= 1) mt = conv_tile_walk(p, mt, BM, ES);
    const int m0 = mt * BM, n0 = nt * BN;

    const int crow = tid >> 3, cc = tid & 7;  // this thread's (row, LDS slot) inside a staging pass
    // chunk of the 128-byte source row this thread fetches: with LDS-DMA the swizzle moves to the source side
    const int cs = GLDS ? (cc ^ ((crow >> 1) & 7)) : cc;
    // The W tile is read with the permuted row map (rows 16g + 4j + r of a wave's range, see wrow[] below), so it gets
    // its own XOR phase: distinct over (g, r >> 1) where the A tile's phase is distinct over 8 consecutive row pairs.
    auto sww = [](int row) { return ((((row % (16 * TN)) / (4 * TN)) & 3) << 1) | ((row >> 1) & 1); };
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- per-thread source addressing -------------------------------------------------------
    const T* a_base[A_IT];
    unsigned a_mask[A_IT];
    const T* w_base[W_IT];
    int cs_w[W_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        int m = m0 + crow + i * (NT / 8);
        if (m >= p.M) m = p.M - 1;
        if (MODE == 0) {
            a_base[i] = (const T*)p.A + gemm_a_row(p, m) * p.lda + cs * EPC;
            a_mask[i] = 0;
        } else {
            int b, ti, hi, wi;
            conv_voxel(p, m, b, ti, hi, wi);
            a_mask[i] = conv_tap_mask(p, ti, hi, wi);
            const long long vox = conv_voxel_index(p, b, ti, hi, wi);
            a_base[i] = (const T*)p.A + vox * p.Cin + cs * EPC;
        }
    }
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        int n = n0 + crow + i * (NT / 8);
        // (plain weights are packed with rows padded to the tile, packing.py; a GROUP's matrix has exactly N rows and the next
        //  group's - or nothing - behind them: rows past N re-read row N - 1, their outputs are discarded by the epilogue)
        if constexpr (GROUPW) n = n < p.N ? n : p.N - 1;
        cs_w[i] = GLDS ? (cc ^ sww(crow + i * (NT / 8))) : cc;
        w_base[i] = (const T*)p.W + (long long)n * p.ldw + cs_w[i] * EPC;
    }

    const int kpc = (MODE == 1) ? (p.Cin / BK) : 1;  // k-tiles per conv tap
    SubpixCells cells{};
    if constexpr (SUBPIX) cells = subpix_cells(p, n0);
    const int nk = SUBPIX ? cells.n * kpc : (p.K + BK - 1) / BK;

    u32x4 ra[A_IT], rw[W_IT];

    auto load_tile = [&](int kt) {
        if (MODE == 0) {
            const int k = kt * BK + cs * EPC;
            const bool kin = k < p.K;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                u32x4 z = {0, 0, 0, 0};
                ra[i] = kin ? *(const u32x4*)(a_base[i] + kt * BK) : z;
            }
#pragma unroll
            for (int i = 0; i < W_IT; ++i) {
                u32x4 z = {0, 0, 0, 0};
                rw[i] = (kt * BK + cs_w[i] * EPC) < p.K ? *(const u32x4*)(w_base[i] + kt * BK) : z;
            }
        } else {
            const int tap = kt / kpc;
            const int ci0 = (kt - tap * kpc) * BK;
            const long long toff = conv_tap_offset(p, tap) + ci0;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                u32x4 z = {0, 0, 0, 0};
                const bool ok = (a_mask[i] >> tap) & 1u;
                u32x4 v = ok ? *(const u32x4*)(a_base[i] + toff) : z;
                if (p.relu_in) {
                    if (ES == 2) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            unsigned x = v[q];
                            unsigned neg = ((x >> 15) & 0x00010001u) * 0xFFFFu;
                            v[q] = x & ~neg;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = __float_as_uint(fmaxf(__uint_as_float(v[q]), 0.0f));
                    }
                }
                ra[i] = v;
            }
#pragma unroll
            for (int i = 0; i < W_IT; ++i) rw[i] = *(const u32x4*)(w_base[i] + kt * BK);
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int row = crow + i * (NT / 8);
            *(u32x4*)(As + buf * BM * 128 + row * 128 + ((cc ^ ((row >> 1) & 7)) << 4)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < W_IT; ++i) {
            const int row = crow + i * (NT / 8);
            *(u32x4*)(Ws + buf * BN * 128 + row * 128 + ((cc ^ sww(row)) << 4)) = rw[i];
        }
    };

    // LDS-DMA staging: one global_load_lds per 16-byte chunk; destination = wave-uniform base + lane*16
    // conv position of the LDS-DMA stream (see issue_tile); starts at this workgroup's first k-tile (split-K: not 0)
    // (SUBPIX: cp_tap counts the active cells, cp_bit is the current cell's tap)
    // (the split-K start and the tap offsets are splitk_begin / conv_tap_offset of gemm_tile.hpp written out: called here, they
    //  compile the LDS-DMA conv kernels to other instruction text)
    int cp_kt = 0, cp_tap = 0, cp_ci0 = 0, cp_bit = 0;
    long long cp_off = 0;
    if constexpr (SUBPIX) {
        cp_bit = subpix_tap(cells, 0);
        cp_off = (((long long)(cp_bit / 9 - 1) * p.Hi + ((cp_bit / 3) % 3 - 1)) * p.Wi + (cp_bit % 3 - 1)) * p.Cin;
    } else if (MODE == 1) {
        const int nsp = p.splitk > 1 ? p.splitk : 1;
        cp_kt = (int)((long long)nk * ksplit / nsp);
        cp_tap = cp_kt / kpc;
        cp_ci0 = (cp_kt - cp_tap * kpc) * BK;
        const int tp = cp_tap < 27 ? cp_tap : 26;
        cp_off = (((long long)(tp / 9 - 1) * p.Hi + ((tp / 3) % 3 - 1)) * p.Wi + (tp % 3 - 1)) * p.Cin;
    }
    auto issue_tile = [&](int kt, int buf) {
        const char* zero = (const char*)g_zero_chunk;
        if (MODE == 0) {
            const bool kin = (kt * BK + cs * EPC) < p.K;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                const char* src = kin ? (const char*)(a_base[i] + kt * BK) : zero;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(As + buf * BM * 128 + (wave_u * 64 + i * NT) * 16), 16, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < W_IT; ++i) {
                const char* src = (kt * BK + cs_w[i] * EPC) < p.K ? (const char*)(w_base[i] + kt * BK) : zero;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(Ws + buf * BN * 128 + (wave_u * 64 + i * NT) * 16), 16, 0, 0);
            }
        } else {
            // (tap, channel slice) of k-tile kt, carried as counters: tiles are issued in k order, one further per call
            while (cp_kt < kt) {
                ++cp_kt;
                cp_ci0 += BK;
                if (cp_ci0 == p.Cin) {
                    cp_ci0 = 0;
                    ++cp_tap;
                    const int tp = SUBPIX ? subpix_tap(cells, cp_tap) : (cp_tap < 27 ? cp_tap : 26);
                    if constexpr (SUBPIX) cp_bit = tp;
                    cp_off = (((long long)(tp / 9 - 1) * p.Hi + ((tp / 3) % 3 - 1)) * p.Wi + (tp % 3 - 1)) * p.Cin;
                }
            }
            const int tap = SUBPIX ? cp_bit : cp_tap;
            const long long toff = cp_off + cp_ci0;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                const bool ok = (a_mask[i] >> tap) & 1u;
                const char* src = ok ? (const char*)(a_base[i] + toff) : zero;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(As + buf * BM * 128 + (wave_u * 64 + i * NT) * 16), 16, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < W_IT; ++i)
                __builtin_amdgcn_global_load_lds((gptr_t)(const char*)(w_base[i] + kt * BK),
                                                 (lptr_t)(Ws + buf * BN * 128 + (wave_u * 64 + i * NT) * 16), 16, 0, 0);
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int li = lane & 15, kg = lane >> 4;
    // fragment rows inside the block tile
    int xrow[TM], wrow[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) xrow[i] = wm * (TM * 16) + i * 16 + li;
#pragma unroll
    for (int j = 0; j < TN; ++j) wrow[j] = wn * (TN * 16) + 4 * TN * (li >> 2) + 4 * j + (li & 3);

    // split-K: this workgroup contracts k-tiles [kt0, kt1) only and leaves a float partial (see below)
    // (splitk_begin, gemm_tile.hpp, written out: the call swaps two scalar instructions in every dense kernel)
    const int nsplit = p.splitk > 1 ? p.splitk : 1;
    int kt0 = (int)((long long)nk * ksplit / nsplit), kt1 = (int)((long long)nk * (ksplit + 1) / nsplit);
    if (MODE == 0 && p.kw_cols > 0) {  // block-structured weights (l4p_gemm_desc.kw_cols): only the k-tiles of this tile's column group
        const int grp = n0 / p.kw_cols;
        kt0 = (grp * p.kw_len) / BK;
        kt1 = ((grp + 1) * p.kw_len + BK - 1) / BK;
        kt1 = kt1 < nk ? kt1 : nk;
    }
    if (STAGES >= 3) {
#pragma unroll
        for (int s = 0; s < STAGES - 1; ++s)
            if (kt0 + s < kt1) issue_tile(kt0 + s, s);
    } else if (GLDS) {
        issue_tile(kt0, 0);
        __syncthreads();
    } else {
        load_tile(kt0);
        store_tile(0);
        __syncthreads();
    }

    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = STAGES >= 3 ? (kt - kt0) % STAGES : (kt - kt0) & 1;
        if (STAGES >= 3) {
            // tile kt has landed once only the tiles issued after it (at most STAGES - 2 of them) are still in flight
            const int ahead = kt1 - 1 - kt < STAGES - 2 ? kt1 - 1 - kt : STAGES - 2;
            if (ahead >= 3)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (A_IT + W_IT)) : "memory");
            else if (ahead == 2)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (A_IT + W_IT)) : "memory");
            else if (ahead == 1)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_IT + W_IT) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + STAGES - 1 < kt1) issue_tile(kt + STAGES - 1, (kt + STAGES - 1 - kt0) % STAGES);
        } else if (kt + 1 < kt1) {
#ifndef GEMM_DBG_NOLOAD  // (tools/probes/gemm_variants.hip: ablation timing)
            if (GLDS)
                issue_tile(kt + 1, cur ^ 1);
            else
                load_tile(kt + 1);
#endif
        }
        const char* Ab = As + cur * BM * 128;
        const char* Wb = Ws + cur * BN * 128;
#if !defined(GEMM_DBG_NOMMA) && !defined(GEMM_NO_HANDSCHED)
        if constexpr (ES == 2 && GLDS && STAGES == 2) {
            // Hand-scheduled k-tile (bf16, LDS-DMA staging).  hipcc answers every LDS wait with lgkmcnt(0) while an LDS-DMA is
            // in flight (four full drains of the read queue per k-tile in its own schedule).  The fragment reads are therefore
            // inline-asm ds_read_b128 with hand-counted lgkmcnt: LDS reads return in order, so MFMA m may issue as soon as the
            // only outstanding reads are those requested after its two operands.  Read order per k-step: A_0, W_0..W_{TN-1},
            // A_1..A_{TM-1}; MFMA order per k-step: i-major; PRE reads run ahead, one more is requested behind each MFMA.
            #ifndef GEMM_HS_PRE
#define GEMM_HS_PRE (TM + TN)
#endif
            constexpr int RPK = TM + TN, NR = KK * RPK, NM = KK * TM * TN, PRE = (GEMM_HS_PRE) < NR ? (GEMM_HS_PRE) : NR;
            const unsigned a_base = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)Ab + (wm * (TM * 16) + li) * 128;
            const unsigned w_base = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)Wb +
                                    (wn * (TN * 16) + 4 * TN * (li >> 2) + (li & 3)) * 128;
            const int swa = (li >> 1) & 7, swq = (((li >> 2) & 3) << 1) | ((li >> 1) & 1);
            unsigned a_ad[KK], w_ad[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                a_ad[kk] = a_base + (((kk * 4 + kg) ^ swa) << 4);
                w_ad[kk] = w_base + (((kk * 4 + kg) ^ swq) << 4);
            }
            u32x4 fr[NR];
            auto rd = [&fr, &a_ad, &w_ad](auto r_) {  // (explicit captures: asm operands do not trigger implicit capture)
                constexpr int r = decltype(r_)::value, kk = r / RPK, q = r % RPK;
                if constexpr (q == 0)
                    asm volatile("ds_read_b128 %0, %1" : "=v"(fr[r]) : "v"(a_ad[kk]) : "memory");
                else if constexpr (q <= TN)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fr[r]) : "v"(w_ad[kk]), "n"((q - 1) * 512) : "memory");
                else
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fr[r]) : "v"(a_ad[kk]), "n"((q - TN) * 2048) : "memory");
            };
            static_for<0, (PRE < NR ? PRE : NR)>(rd);
            static_for<0, NM>([&](auto m_) {
                constexpr int m = decltype(m_)::value, kk = m / (TM * TN), i = (m % (TM * TN)) / TN, j = m % TN;
                constexpr int ra = kk * RPK + (i == 0 ? 0 : TN + i), rw = kk * RPK + 1 + j;  // reads holding A_i / W_j
                constexpr int need = ra > rw ? ra : rw;
                constexpr int issued = (PRE + m < NR) ? PRE + m : NR;
                static_assert(need < issued, "operand requested before use");
                asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(issued - need - 1 > 15 ? 15 : issued - need - 1) : "memory");
                __builtin_amdgcn_sched_barrier(0);
                acc[i][j] = mma16(__builtin_bit_cast(frag_t, fr[rw]), __builtin_bit_cast(frag_t, fr[ra]), acc[i][j]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (PRE + m < NR) rd(std::integral_constant<int, PRE + m>{});
            });
        } else
#endif
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            frag_t xf[TM], wf[TN];
            const int c0 = kk * 2 * ES + kg * CPF;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = xrow[i];
                const int sw = (row >> 1) & 7;
                u32x4* d = (u32x4*)&xf[i];
#pragma unroll
                for (int q = 0; q < CPF; ++q) d[q] = *(const u32x4*)(Ab + row * 128 + (((c0 + q) ^ sw) << 4));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wrow[j];
                const int sw = sww(row);
                u32x4* d = (u32x4*)&wf[j];
#pragma unroll
                for (int q = 0; q < CPF; ++q) d[q] = *(const u32x4*)(Wb + row * 128 + (((c0 + q) ^ sw) << 4));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
#ifdef GEMM_DBG_NOMMA  // keep the fragment reads alive, skip the matrix pipe
                    asm volatile("" ::"v"(wf[j]), "v"(xf[i]));
#else
                    acc[i][j] = mma16(wf[j], xf[i], acc[i][j]);
#endif
                }
        }
        if (!GLDS && kt + 1 < kt1) store_tile(cur ^ 1);
        if (STAGES == 2) __syncthreads();
    }

    if constexpr (SUBPIX) {
        gemm_epilogue_subpixel<T, TM, TN>(p, acc, m0 + wm * (TM * 16), n0 + wn * (TN * 16), li, kg);
        return;
    }
    if (p.splitk > 1) {
        // raw float partial [ksplit][M][N]; bias / activation / residuals / conversion happen in splitk_finish_kernel
        const int nb2 = n0 + wn * (TN * 16) + 4 * TN * kg;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * (TM * 16) + i * 16 + li;
            if (m >= p.M) continue;
            float* pp = p.partial + ((long long)ksplit * p.M + m) * p.N + nb2;
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (nb2 + 4 * j < p.N) *(f32x4*)(pp + 4 * j) = acc[i][j];
        }
        return;
    }

    if (p.epi == EPI_MASKDOT) {
        gemm_epilogue_maskdot<T, TM, TN>(p, acc, m0 + wm * (TM * 16), n0 + wn * (TN * 16), li, kg);
        return;
    }
    if constexpr (ES == 2) {  // plain dense / QKV epilogues: the lean specialisations
        if (gemm_epilogue_dense_dispatch<T, TM, TN>(p, acc, m0 + wm * (TM * 16), n0 + wn * (TN * 16), li, kg)) return;
    }
    gemm_epilogue<T, TM, TN>(p, acc, m0 + wm * (TM * 16), n0 + wn * (TN * 16), li, kg);
}

template <typename T, int BM, int BN, int WM, int WN, int MODE, bool GLDS, int STAGES = 2, bool GROUPW = false, bool SUBPIX = false>
__global__ __launch_bounds__(WM* WN * 64) void gemm_kernel(const GemmParams p) {
    gemm_body<T, BM, BN, WM, WN, MODE, GLDS, STAGES, GROUPW, SUBPIX>(p, (int)blockIdx.x);
}

// Up to L4P_GEMM_GROUP_MAX independent dense GEMMs as ONE launch: workgroups [first[g], first[g + 1]) run problem g.  For the
// tracker's token-side projections (self-attention q / k / v, image -> token k / v, the three hyper-network MLP stages): each is
// a 20 us launch that fills a quarter of the chip, and they come in independent groups of two or three.
struct GemmGroupParams {
    GemmParams p[L4P_GEMM_GROUP_MAX];
    int first[L4P_GEMM_GROUP_MAX + 1];
};
template <typename T, int BM, int BN, int WM, int WN, bool GLDS, int STAGES>
__global__ __launch_bounds__(WM* WN * 64) void gemm_group_kernel(const GemmGroupParams g) {
    const int b = (int)blockIdx.x;
    int i = 0;
#pragma unroll
    for (int k = 1; k < L4P_GEMM_GROUP_MAX; ++k)
        if (b >= g.first[k]) i = k;
    // (a uniform switch keeps the descriptor accesses static: kernel arguments are read through scalar loads)
    switch (i) {
        case 0: gemm_body<T, BM, BN, WM, WN, 0, GLDS, STAGES>(g.p[0], b - g.first[0]); break;
        case 1: gemm_body<T, BM, BN, WM, WN, 0, GLDS, STAGES>(g.p[1], b - g.first[1]); break;
        case 2: gemm_body<T, BM, BN, WM, WN, 0, GLDS, STAGES>(g.p[2], b - g.first[2]); break;
        default: gemm_body<T, BM, BN, WM, WN, 0, GLDS, STAGES>(g.p[3], b - g.first[3]); break;
    }
}

// host launcher (gemm.hip)
int launch_gemm(int dtype, int mode, const GemmParams& p, hipStream_t stream);
int launch_gemm_group(int dtype, const GemmParams* p, int n, hipStream_t stream);
// ... and its per-element-type halves (gemm_launch.hpp; instantiated in gemm_bf16.hip / gemm_f16.hip / gemm_f32.hip, the grouped one 16-bit only)
template <typename T>
int launch_gemm_typed(int mode, const GemmParams& p, hipStream_t stream);
template <typename T>
int launch_gemm_group_typed(const GemmParams* p, int n, hipStream_t stream);
