// The addressing arithmetic the GEMM / implicit-conv kernels share (gemm.hpp, gemm8p.hpp, gemm4w.hpp, conv3_halo.hpp,
// gemm_skinny.hpp) and the epilogues (gemm_epilogue.hpp) read: workgroup -> tile orders, the row-group map of A, the conv's voxel
// decode, tap masks and tap offsets, the split-K k-range and the sub-pixel conv's cell walk.  Each kernel keeps its own XOR swizzles,
// and a few call sites keep their own copy of an expression below because the call compiles their kernel to other instruction text
// (marked where they stand; DESIGN.md, "GEMM kernels: epilogues in their own header, shared addressing helpers").
// Plain integer arithmetic on the public descriptor, so a host compiler takes it too (no HIP header on that path):
// tests/gemm_tile_main.cpp runs it on the CPU against brute force (tests/test_gemm_tile_cpu.py).
#pragma once
#if defined(__HIPCC__)
#include "common.hpp"
#define GEMM_TILE_FN __device__ __forceinline__
// LDS-DMA operands: global_load_lds / buffer_load ... lds take their source and destination in these address spaces
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
#else
#define GEMM_TILE_FN inline
#endif
#include "l4p_hip.h"

// XCD-contiguous tile ranges: workgroup bid runs on XCD bid % 8 and is that XCD's (bid / 8)-th; XCD x owns a contiguous range of the
// ntiles tiles (the first ntiles % 8 ranges are one longer), so the tiles an XCD runs at a time are neighbours and share its L2
GEMM_TILE_FN int xcd_tile(int bid, int ntiles) {
    const int xcd = bid & 7, idx = bid >> 3, q = ntiles >> 3, r = ntiles & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Banded linear order of ntm x ntn tiles (gemm8p.hpp, "Linear order of the tiles"): column bands of <= 8 tile columns, inside a band
// m-major with the band's columns fastest; one band (ntn <= 8) is plain row-major order
GEMM_TILE_FN void banded_tile(int tile, int ntn, int ntm, int& mt, int& nt) {
    const int nb = (ntn + 7) >> 3, bw = (ntn + nb - 1) / nb, full = (nb - 1) * ntm * bw;
    if (nb == 1) {
        mt = tile / ntn;
        nt = tile % ntn;
    } else if (tile < full) {
        const int band = tile / (ntm * bw), rem = tile - band * (ntm * bw);
        mt = rem / bw;
        nt = band * bw + rem % bw;
    } else {
        const int w = ntn - (nb - 1) * bw, rem = tile - full;  // last band: the remaining w columns
        mt = rem / w;
        nt = (nb - 1) * bw + rem % w;
    }
}

// logical row m of A -> physical row: the descriptor's optional one-level row-group map (l4p_gemm_desc.a_*)
GEMM_TILE_FN long long gemm_a_row(const l4p_gemm_desc& p, int m) {
    return p.a_gr > 0 ? (long long)(m / p.a_gr) * p.a_gs + p.a_go + (m % p.a_gr) : m;
}

// split-K: slice ksplit of nsplit contracts the k-tiles [splitk_begin(ksplit), splitk_begin(ksplit + 1)) of nk; the slices tile [0, nk)
GEMM_TILE_FN int splitk_begin(int nk, int ksplit, int nsplit) { return (int)((long long)nk * ksplit / nsplit); }

// ---- implicit-GEMM conv (3x3x3, pad 1, channels-last): row m of the GEMM is output voxel (b, to, ho, wo); tap = (dt+1)*9 + (dh+1)*3 + dw+1 ----
// output voxel m -> batch index and its centre input voxel (ti, hi, wi)
GEMM_TILE_FN void conv_voxel(const l4p_gemm_desc& p, int m, int& b, int& ti, int& hi, int& wi) {
    int wo = m % p.Wo;
    int r = m / p.Wo;
    int ho = r % p.Ho;
    r /= p.Ho;
    int to = r % p.To;
    b = r / p.To;
    ti = to * p.st, hi = ho * p.sh, wi = wo * p.sw;
}
// ... and that voxel's index in the input volume
GEMM_TILE_FN long long conv_voxel_index(const l4p_gemm_desc& p, int b, int ti, int hi, int wi) {
    return (((long long)b * p.Ti + ti) * p.Hi + hi) * p.Wi + wi;
}
// bit tap = that tap of the voxel lies inside the input volume (the others read as zero: the conv's padding)
GEMM_TILE_FN unsigned conv_tap_mask(const l4p_gemm_desc& p, int ti, int hi, int wi) {
    unsigned mask = 0;
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
        int dt = tap / 9 - 1, dh = (tap / 3) % 3 - 1, dw = tap % 3 - 1;
        bool ok = (unsigned)(ti + dt) < (unsigned)p.Ti && (unsigned)(hi + dh) < (unsigned)p.Hi &&
                  (unsigned)(wi + dw) < (unsigned)p.Wi;
        mask |= (ok ? 1u : 0u) << tap;
    }
    return mask;
}
// element offset of a tap's voxel relative to the centre voxel
GEMM_TILE_FN long long conv_tap_offset(const l4p_gemm_desc& p, int tap) {
    const int dt = tap / 9 - 1, dh = (tap / 3) % 3 - 1, dw = tap % 3 - 1;
    return (((long long)dt * p.Hi + dh) * p.Wi + dw) * p.Cin;
}

// Tile walk of the implicit-GEMM conv.  Every input voxel feeds 27 taps; with workgroups handed out in plain row order
// over eight XCDs the three t-planes a tile touches are 2 x (Ho*Wo*Cin) bytes apart and each XCD's 4 MB L2 re-fetched
// them from HBM (PMC: 7.9 GB read per launch of the 16x224x224x128 conv against 0.8 GB of input).  Here an XCD owns a
// contiguous range of tiles (the caller's XCD remap) and position n of the walk is the m-tile
//   (b, band, t, i):  i fastest inside a band of BT tiles (a few image rows), then t, then the next band
// so the rows of planes t-1 / t / t+1 that a band needs are still in L2 when the walk moves to t+1.
#ifdef GEMM_PROBE_VARIANTS
__device__ int g_conv_bt_override = 0;  // (tools/probes: band size experiments)
#endif
GEMM_TILE_FN int conv_tile_walk(const l4p_gemm_desc& p, int n, int BM, int es) {
    const int P = p.Ho * p.Wo;  // output voxels per (b, t) plane
    if (P % BM) return n;
    const int TP = P / BM;
    const long long tile_bytes = (long long)BM * p.sh * p.sw * p.Cin * es;
    int bt = (int)((2ll << 20) / 3 / (tile_bytes > 0 ? tile_bytes : 1));
#ifdef GEMM_PROBE_VARIANTS
    if (g_conv_bt_override > 0) bt = g_conv_bt_override;
#endif
    if (bt > TP) bt = TP;
    if (bt < 1) bt = 1;
    while (TP % bt) --bt;  // largest divisor of TP that keeps three planes of a band within ~2 MB
    const int i = n % bt;
    int r = n / bt;
    const int t = r % p.To;
    r /= p.To;
    const int band = r % (TP / bt), b = r / (TP / bt);
    return (b * p.To + t) * TP + band * bt + i;
}

// ---- sub-pixel conv (l4p_conv3d_subpixel, include/l4p_hip.h): ConvTranspose3d with kernel == stride == k folded into the 3x3x3 conv
//      behind it (packing.py fold_convT_rn).  Output column n = s * Cout + f, s = (s_t * kh + s_h) * kw + s_w the sub-position of the
//      up-scaled voxel inside its low-resolution cell.  Along an axis the three taps of position k i + s reach the cells
//      {i-1, i} (s = 0), {i, i+1} (s = k - 1), {i} (in between) or {i-1, i, i+1} (k = 1), so a column tile - which lies inside ONE
//      sub-position: Cout is a multiple of the tile width - contracts only those cells, in ascending (c_t, c_h, c_w) order, Cin
//      channels each: its weight rows hold exactly that sequence.  A cell is a tap of the 27-tap low-resolution neighbourhood, so the
//      loaders' validity masks and tap offsets serve unchanged. ----
struct SubpixCells {
    int t0, h0, w0;  // first cell of each axis as a tap coordinate (0 .. 2 = cell offset -1 .. +1)
    int nh, nw, n;   // cells along h and w, cells in all
};
GEMM_TILE_FN void subpix_axis(int k, int s, int& c0, int& nc) {
    if (k == 1)
        c0 = 0, nc = 3;
    else if (s == 0)
        c0 = 0, nc = 2;
    else if (s == k - 1)
        c0 = 1, nc = 2;
    else
        c0 = 1, nc = 1;
}
GEMM_TILE_FN SubpixCells subpix_cells(const l4p_gemm_desc& p, int n0) {  // (n0: wave uniform)
    const int s = n0 / p.Cout;
    SubpixCells c;
    int nt;
    subpix_axis(p.kt, s / (p.kw * p.kh), c.t0, nt);
    subpix_axis(p.kh, (s / p.kw) % p.kh, c.h0, c.nh);
    subpix_axis(p.kw, s % p.kw, c.w0, c.nw);
    c.n = nt * c.nh * c.nw;
    return c;
}
// tap (0 .. 26) of the j-th active cell; j past the end repeats the last one (loaders that run ahead mask those tiles out)
GEMM_TILE_FN int subpix_tap(const SubpixCells& c, int j) {
    j = j < c.n ? j : c.n - 1;
    const int r = j / c.nw;
    return (c.t0 + r / c.nh) * 9 + (c.h0 + r % c.nh) * 3 + c.w0 + j % c.nw;
}
