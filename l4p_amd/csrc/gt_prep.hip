// Ground-truth clip preparation on the GPU: the per-element work of the reference's L4PDataset base class
// (l4p/data/l4p_dataset_mini.py:126-395, 499-519) for a sample whose raw tensors are already in HBM.
//
// Replaces, per sample,
//   * mirror_and_pad / repeat_single_frame (:126-235): a frame table (source frame, swap flag) computed on the host; the swap
//     flag selects the opposite-direction flow source, so no padded tensor is ever written;
//   * resize (:237-290): F.interpolate(nearest) as two index tables, F.interpolate(trilinear, frame count unchanged) as per-frame
//     bilinear in ATen's order, the flow / track rescaling as ONE float32 multiply after the interpolation;
//   * crop (:292-395): the offsets are folded into the tables; the query bounds filter is an ordered compaction; the track
//     shift, the visibility clearing and the query shift run in the gather of the kept rows;
//   * fix_track_valid_for_causal_estimation (:499-519) and the ImageNet normalisation of rgb (:576-580).
//
// Three launches: every dense field of the sample in one (a by-value array of field descriptors), the query filter (one
// workgroup; its 4-byte count is the only thing the host reads back), the track tensors.  Byte-moving work bound by HBM.
#include <cstdint>

#include "common.hpp"
#include "l4p_hip.h"

// This file is compiled with -ffp-contract=off (Makefile): `x * f - j0` and `w0 * v0 + w1 * v1` round operation by operation, as
// the reference's separate torch operations do, so the nearest-gathered fields, the tracks and the queries equal the reference's
// bit for bit.

namespace {

struct DenseArgs {
    l4p_gt_field f[L4P_GT_MAX_FIELDS];
    int plane0[L4P_GT_MAX_FIELDS + 1];  // first (channel, frame) plane of every field; plane0[n_fields] = number of planes
    int n_fields;
    int T0, H, W;                // size of every source
    const int* frame_table;      // [Tn][2] (source frame, swap flag)
    const int* ynear;            // [Hn] / [Wn] nearest source row / column (crop folded in)
    const int* xnear;
    const int* yi0;              // [Hn] bilinear rows and weight (crop folded in); NULL when no field is bilinear
    const int* yi1;
    const float* ylam;
    const int* xi0;
    const int* xi1;
    const float* xlam;
    int Tn, Hn, Wn;
};

// grid.y = (field, channel, frame) plane, grid.x = tiles of 256 pixels of the plane.  The descriptor of a plane is uniform over
// the workgroup (scalar loads from the kernel arguments); the tail tile is guarded.  A frame or table entry outside the source
// writes NaN, never reads out of range.
__global__ __launch_bounds__(256) void gt_dense_clip_kernel(DenseArgs a) {
    const int plane = blockIdx.y;
    int fi = 0;
    while (fi + 1 < a.n_fields && plane >= a.plane0[fi + 1]) ++fi;
    const l4p_gt_field& d = a.f[fi];
    const int local = plane - a.plane0[fi];
    const int c = local / a.Tn, t = local - c * a.Tn;
    const int per_frame = a.Hn * a.Wn;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= per_frame) return;
    const int oy = p / a.Wn, ox = p - oy * a.Wn;
    const int fr = a.frame_table[2 * t], swap = a.frame_table[2 * t + 1];
    const float* src = (swap && d.src_swap) ? d.src_swap : d.src;
    float v = __builtin_nanf("");
    if ((unsigned)fr < (unsigned)a.T0) {
        const float* img = src + ((long long)c * a.T0 + fr) * a.H * a.W;
        if (d.mode == L4P_GT_NEAREST) {
            const int y = a.ynear[oy], x = a.xnear[ox];
            if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) v = img[(long long)y * a.W + x];
        } else {
            const int y0 = a.yi0[oy], y1 = a.yi1[oy], x0 = a.xi0[ox], x1 = a.xi1[ox];
            if ((unsigned)y0 < (unsigned)a.H && (unsigned)y1 < (unsigned)a.H && (unsigned)x0 < (unsigned)a.W &&
                (unsigned)x1 < (unsigned)a.W) {
                const float ly = a.ylam[oy], lx = a.xlam[ox];
                const float wy0 = 1.f - ly, wx0 = 1.f - lx;
                const float* r0 = img + (long long)y0 * a.W;
                const float* r1 = img + (long long)y1 * a.W;
                // w0 * v0 + w1 * v1 per axis as ATen writes it, un-contracted
                const float top = __fadd_rn(__fmul_rn(r0[x0], wx0), __fmul_rn(r0[x1], lx));
                const float bot = __fadd_rn(__fmul_rn(r1[x0], wx0), __fmul_rn(r1[x1], lx));
                v = __fadd_rn(__fmul_rn(top, wy0), __fmul_rn(bot, ly));
                // the time axis keeps its size: ATen "simply copies" such an axis with both indices on the same frame and weights
                // (1, 0) (UpSampleKernel.cpp compute_source_index_and_lambda) - every finite v stays as it is, inf becomes nan
                v = __fadd_rn(__fmul_rn(v, 1.f), __fmul_rn(v, 0.f));
            }
        }
        if (d.apply_scale) v = __fmul_rn(v, d.scale[c]);
        if (d.normalize) v = __fdiv_rn(__fsub_rn(v, d.mean[c]), d.stdv[c]);
    }
    d.out[((long long)c * a.Tn + t) * per_frame + p] = v;
}

struct Bounds {
    float t_lo, t_hi, x_lo, x_hi, y_lo, y_hi;  // the integer bounds t0, t0 + Tn, j0, j0 + Wn, i0, i0 + Hn as float32
    float qx, qy;                              // query scaling of the scale_queries extension (applied when scale_q)
    int scale_q;
};

__device__ __forceinline__ void load_query(const float* __restrict__ q, int n, const Bounds& b, float& qt, float& qx, float& qy) {
    qt = q[3 * n];
    qx = q[3 * n + 1];
    qy = q[3 * n + 2];
    if (b.scale_q) {
        qx = __fmul_rn(qx, b.qx);
        qy = __fmul_rn(qy, b.qy);
    }
}

// One workgroup (4 waves): query n is kept iff it lies strictly inside the crop on all three axes; kept n in ascending order
// (ballot + popcount inside a wave, the four wave totals through LDS, rounds of 256 queries in order).
__global__ __launch_bounds__(256) void gt_query_select_kernel(const float* __restrict__ q, int N, Bounds b, int* __restrict__ sel,
                                                              int* __restrict__ count) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + threadIdx.x;
        bool keep = false;
        if (n < N) {
            float qt, qx, qy;
            load_query(q, n, b, qt, qx, qy);
            keep = qt > b.t_lo && qt < b.t_hi && qx > b.x_lo && qx < b.x_hi && qy > b.y_lo && qy < b.y_hi;
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int k = 0; k < wave; ++k) off += wave_total[k];
        if (keep) sel[off + before] = n;
        base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

struct TrackArgs {
    const float* traj;           // [N][2][T0]
    const unsigned char* vis;    // [N][T0]
    const unsigned char* valid;  // [N][T0]
    const float* depth;          // [N][T0] or NULL
    const float* queries;        // [N][3]
    const float* labels;         // [N]
    const int* sel;              // [M] kept rows, NULL = identity
    const int* frame_table;      // [Tn][2]
    int N, T0, M, Tn;
    float fw, fh;                // resize factors as float32 (applied when scale_traj)
    int scale_traj;
    int cropped;                 // 0: the crop was a no-op (the reference returns before the shift and the clearing)
    float t0, j0, i0, Wn, Hn;    // crop offsets and size as float32
    int causal;                  // 0, or the single estimation direction 1 / -1
    Bounds b;                    // (only the query scaling is read here)
    float* traj_out;             // [M][2][Tn]
    unsigned char* vis_out;      // [M][Tn]
    unsigned char* valid_out;    // [M][Tn]
    float* depth_out;            // [M][Tn] or NULL
    float* queries_out;          // [M][3]
    float* labels_out;           // [M]
};

// One thread per (kept row, output frame); the thread of frame 0 also writes the row's query and label.
__global__ __launch_bounds__(256) void gt_tracks_clip_kernel(TrackArgs a) {
    const long long total = (long long)a.M * a.Tn;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const int m = (int)(i / a.Tn), t = (int)(i - (long long)m * a.Tn);
        const int n = a.sel ? a.sel[m] : m;
        const int fr = a.frame_table[2 * t];
        const bool ok = (unsigned)n < (unsigned)a.N && (unsigned)fr < (unsigned)a.T0;
        float x = __builtin_nanf(""), y = x, dep = x, qt = x, qx = x, qy = x, lab = x;
        unsigned char vis = 0, valid = 0;
        if (ok) {
            x = a.traj[((long long)n * 2 + 0) * a.T0 + fr];
            y = a.traj[((long long)n * 2 + 1) * a.T0 + fr];
            vis = a.vis[(long long)n * a.T0 + fr] ? 1 : 0;
            valid = a.valid[(long long)n * a.T0 + fr] ? 1 : 0;
            if (a.depth) dep = a.depth[(long long)n * a.T0 + fr];
            load_query(a.queries, n, a.b, qt, qx, qy);
            lab = a.labels[n];
        }
        if (a.scale_traj) {
            x = __fmul_rn(x, a.fw);
            y = __fmul_rn(y, a.fh);
        }
        if (a.cropped) {
            x = __fsub_rn(x, a.j0);
            y = __fsub_rn(y, a.i0);
            if (x >= a.Wn || x < 0.f || y >= a.Hn || y < 0.f) vis = 0;
            qt = __fsub_rn(qt, a.t0);
            qx = __fsub_rn(qx, a.j0);
            qy = __fsub_rn(qy, a.i0);
        }
        const float time = (float)t + 0.5f;
        if (a.causal > 0) valid = (valid && time >= qt) ? 1 : 0;
        if (a.causal < 0) valid = (valid && time <= qt) ? 1 : 0;
        a.traj_out[((long long)m * 2 + 0) * a.Tn + t] = x;
        a.traj_out[((long long)m * 2 + 1) * a.Tn + t] = y;
        a.vis_out[i] = vis;
        a.valid_out[i] = valid;
        if (a.depth_out) a.depth_out[i] = dep;
        if (t == 0) {
            a.queries_out[3 * m] = qt;
            a.queries_out[3 * m + 1] = qx;
            a.queries_out[3 * m + 2] = qy;
            a.labels_out[m] = lab;
        }
    }
}

Bounds make_bounds(int t0, int Tn, int i0, int Hn, int j0, int Wn, int scale_q, float fw, float fh) {
    Bounds b{};
    b.t_lo = (float)t0;
    b.t_hi = (float)(t0 + Tn);
    b.x_lo = (float)j0;
    b.x_hi = (float)(j0 + Wn);
    b.y_lo = (float)i0;
    b.y_hi = (float)(i0 + Hn);
    b.qx = fw;
    b.qy = fh;
    b.scale_q = scale_q ? 1 : 0;
    return b;
}

}  // namespace

extern "C" {

int l4p_gt_dense_clip(l4p_stream s, const l4p_gt_field* fields, int n_fields, int T0, int H, int W, const int* frame_table,
                      const int* ynear, const int* xnear, const int* yi0, const int* yi1, const float* ylam, const int* xi0,
                      const int* xi1, const float* xlam, int Tn, int Hn, int Wn) {
    if (!fields || n_fields <= 0 || n_fields > L4P_GT_MAX_FIELDS || T0 <= 0 || H <= 0 || W <= 0 || Tn <= 0 || Hn <= 0 || Wn <= 0 ||
        !frame_table || !ynear || !xnear) {
        l4p_set_error("gt_dense_clip: bad arguments (%d fields, source %dx%dx%d, output %dx%dx%d)", n_fields, T0, H, W, Tn, Hn, Wn);
        return L4P_E_INVALID;
    }
    DenseArgs a{};
    long long planes = 0;
    for (int i = 0; i < n_fields; ++i) {
        const l4p_gt_field& f = fields[i];
        if (!f.src || !f.out || f.channels < 1 || f.channels > 3 || (f.mode != L4P_GT_NEAREST && f.mode != L4P_GT_BILINEAR)) {
            l4p_set_error("gt_dense_clip: field %d: bad descriptor (channels %d, mode %d)", i, f.channels, f.mode);
            return L4P_E_INVALID;
        }
        if (f.mode == L4P_GT_BILINEAR && (!yi0 || !yi1 || !ylam || !xi0 || !xi1 || !xlam)) {
            l4p_set_error("gt_dense_clip: field %d is bilinear and the bilinear tables are missing", i);
            return L4P_E_INVALID;
        }
        a.f[i] = f;
        a.plane0[i] = (int)planes;
        planes += (long long)f.channels * Tn;
    }
    if (planes > 65535 || (long long)Hn * Wn > (1ll << 30)) {
        l4p_set_error("gt_dense_clip: %lld planes of %dx%d pixels exceed one launch", planes, Hn, Wn);
        return L4P_E_INVALID;
    }
    a.plane0[n_fields] = (int)planes;
    a.n_fields = n_fields;
    a.T0 = T0;
    a.H = H;
    a.W = W;
    a.frame_table = frame_table;
    a.ynear = ynear;
    a.xnear = xnear;
    a.yi0 = yi0;
    a.yi1 = yi1;
    a.ylam = ylam;
    a.xi0 = xi0;
    a.xi1 = xi1;
    a.xlam = xlam;
    a.Tn = Tn;
    a.Hn = Hn;
    a.Wn = Wn;
    hipStream_t stream = (hipStream_t)s;
    ProfScope prof(PROF_PREP, stream, "gt_dense_clip F%d T%d %dx%d->%dx%d", n_fields, Tn, H, W, Hn, Wn);
    const dim3 grid((unsigned)(((long long)Hn * Wn + 255) / 256), (unsigned)planes);
    hipLaunchKernelGGL(gt_dense_clip_kernel, grid, dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_gt_query_select(l4p_stream s, const float* queries, int N, int t0, int Tn, int i0, int Hn, int j0, int Wn,
                        int scale_queries, float fw, float fh, int* sel, int* count) {
    if (!queries || !sel || !count || N <= 0 || Tn <= 0 || Hn <= 0 || Wn <= 0 || t0 < 0 || i0 < 0 || j0 < 0) {
        l4p_set_error("gt_query_select: bad arguments (N %d, crop %d+%d, %d+%d, %d+%d)", N, t0, Tn, i0, Hn, j0, Wn);
        return L4P_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)s;
    ProfScope prof(PROF_PREP, stream, "gt_query_select N%d", N);
    hipLaunchKernelGGL(gt_query_select_kernel, dim3(1), dim3(256), 0, stream, queries, N,
                       make_bounds(t0, Tn, i0, Hn, j0, Wn, scale_queries, fw, fh), sel, count);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_gt_tracks_clip(l4p_stream s, const float* traj, const unsigned char* vis, const unsigned char* valid, const float* depth,
                       const float* queries, const float* labels, int N, int T0, const int* sel, int M, const int* frame_table,
                       int Tn, int scale_traj, int scale_queries, float fw, float fh, int cropped, int t0, int i0, int j0, int Hn,
                       int Wn, int causal, float* traj_out, unsigned char* vis_out, unsigned char* valid_out, float* depth_out,
                       float* queries_out, float* labels_out) {
    if (M == 0) return 0;  // nothing kept: the caller's tensors are empty
    if (!traj || !vis || !valid || !queries || !labels || !frame_table || !traj_out || !vis_out || !valid_out || !queries_out ||
        !labels_out || N <= 0 || T0 <= 0 || M < 0 || M > N || Tn <= 0 || Hn <= 0 || Wn <= 0 || (depth == nullptr) != (depth_out == nullptr) ||
        (causal != 0 && causal != 1 && causal != -1)) {
        l4p_set_error("gt_tracks_clip: bad arguments (N %d, M %d, T %d->%d, causal %d)", N, M, T0, Tn, causal);
        return L4P_E_INVALID;
    }
    TrackArgs a{};
    a.traj = traj;
    a.vis = vis;
    a.valid = valid;
    a.depth = depth;
    a.queries = queries;
    a.labels = labels;
    a.sel = sel;
    a.frame_table = frame_table;
    a.N = N;
    a.T0 = T0;
    a.M = M;
    a.Tn = Tn;
    a.fw = fw;
    a.fh = fh;
    a.scale_traj = scale_traj ? 1 : 0;
    a.cropped = cropped ? 1 : 0;
    a.t0 = (float)t0;
    a.j0 = (float)j0;
    a.i0 = (float)i0;
    a.Wn = (float)Wn;
    a.Hn = (float)Hn;
    a.causal = causal;
    a.b = make_bounds(t0, Tn, i0, Hn, j0, Wn, scale_queries, fw, fh);
    a.traj_out = traj_out;
    a.vis_out = vis_out;
    a.valid_out = valid_out;
    a.depth_out = depth_out;
    a.queries_out = queries_out;
    a.labels_out = labels_out;
    hipStream_t stream = (hipStream_t)s;
    ProfScope prof(PROF_PREP, stream, "gt_tracks_clip M%d T%d", M, Tn);
    const long long blocks = ((long long)M * Tn + 255) / 256;
    hipLaunchKernelGGL(gt_tracks_clip_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
