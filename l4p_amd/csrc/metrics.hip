// Evaluation metrics on the GPU: what a metrics_module(batch, out, metadata) of the reference's L4PLitModule.step (l4p/l4p.py:74-78)
// has to compute for the five tasks.  The reference ships no metrics code; the definitions are the benchmarks' own (depth: abs_rel /
// rmse / delta; flow: end-point error; motion mask: IoU / F1; tracks: TAP-Vid; cameras: ATE / RPE) and are stated at the entry
// points in include/l4p_hip.h, operation by operation in f32 (this file is compiled with -ffp-contract=off), so that
// tests/metrics_restate.py restates them in numpy bit for bit.  Everything stays on the device and on the caller's stream.
//
// Dense kernels (depth, flow, mask): one grid-stride pass over the n elements of a clip (blockIdx.y), 16-byte loads between a scalar
// head and tail where every array of the clip starts at the same offset inside a 16-byte line (else the whole clip goes the scalar
// way), f64 sums and integer counts in registers, a wave butterfly, then one 8-slot row per workgroup into a scratch slab; a second
// launch adds the rows of a clip in a FIXED order (thread j takes rows j, j + 256, ..., then a fixed tree) and forms the metrics in
// f64.  No float atomics: two runs give the same bits (the pattern of affine_sums_kernel / affine_solve_kernel in geom.hip).
//
// l4p_metric_depth_full runs the depth entry's passes (its first 13 columns are that entry's bits) with a fourth alignment, least
// squares in inverse depth, and one more dense pass for the log-space sums; the logs are f64 (log of the device library on doubles),
// so that the result does not hang on the last bit of one library's logf.  l4p_metric_tracks3d: see the 3D tracks block below.
#include "common.hpp"
#include "umeyama_moments.hpp"

#define MET_SLOTS 8         // 8-byte slots of one partial row: the f64 sums first, then the counts
#define MET_MAX_BLOCKS 1024 // workgroups per clip
#define MET_OUT 16          // doubles per clip of the dense entries (L4P_METRIC_DENSE_OUT)
#define MET_TRK_OUT 32      // L4P_METRIC_TRACKS_OUT
#define MET_TRK_COUNTS 18
#define MET_CAM_OUT 8       // L4P_METRIC_CAMERAS_OUT
#define MET_TRK_TRACKS 16   // tracks per workgroup
#define MET_FULL_OUT 24     // L4P_METRIC_DEPTH_FULL_OUT

enum { MET_DEPTH_QUOT = 0, MET_DEPTH_LSQ, MET_DEPTH_ERR, MET_FLOW, MET_MASK, MET_DEPTH_LSQ_INV, MET_DEPTH_ERR_INV, MET_DEPTH_LOG };

struct MetParams {
    const float* a;    // estimate / logit
    const float* g;    // ground truth
    const float* v;    // valid or NULL
    long long n;       // elements per clip (and per channel)
    float dmin, dmax;  // depth
    const float* sol;  // depth error: (s, t) per clip, NULL = (1, 0)
    float* quot;       // depth quotients [B][n]
    int inv;           // depth log errors: the alignment is in inverse depth
};

struct MetAcc {
    double f[4];
    unsigned c[4];
};

__device__ __forceinline__ bool met_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double met_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

template <int MODE> struct MetElem;
// x[0] = est, x[1] = gt, x[2] = valid
__device__ __forceinline__ bool met_depth_ok(const float* x, const MetParams& p) {
    return x[2] > 0.5f && met_finite(x[1]) && x[1] > p.dmin && x[1] < p.dmax && met_finite(x[0]) && x[0] > 0.f;
}
template <> struct MetElem<MET_DEPTH_QUOT> {
    static constexpr int NS = 3, NF = 0, NC = 1;
    __device__ static void streams(const MetParams& p, int b, const float** s) {
        s[0] = p.a + b * p.n, s[1] = p.g + b * p.n, s[2] = p.v ? p.v + b * p.n : nullptr;
    }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float, float, MetAcc& acc) {
        const bool ok = met_depth_ok(x, p);
        acc.c[0] += ok;
        return ok ? x[1] / x[0] : __uint_as_float(0x7F800000u);
    }
};
template <> struct MetElem<MET_DEPTH_LSQ> {
    static constexpr int NS = 3, NF = 4, NC = 1;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float, float, MetAcc& acc) {
        if (met_depth_ok(x, p)) {
            const double e = x[0], g = x[1];
            acc.f[0] += e;
            acc.f[1] += e * e;
            acc.f[2] += g;
            acc.f[3] += e * g;
            acc.c[0] += 1;
        }
        return 0.f;
    }
};
template <> struct MetElem<MET_DEPTH_ERR> {
    static constexpr int NS = 3, NF = 2, NC = 4;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float s, float t, MetAcc& acc) {
        if (met_depth_ok(x, p) && s == s && t == t) {  // (a NaN alignment scores nothing)
            const float g = x[1];
            const float m = s * x[0];
            const float a = fminf(fmaxf(m + t, p.dmin), p.dmax);
            const float d = a - g;
            acc.f[0] += (double)(fabsf(d) / g);
            acc.f[1] += (double)(d * d);
            const float r = fmaxf(a / g, g / a);
            acc.c[0] += 1;
            acc.c[1] += r < 1.25f;
            acc.c[2] += r < 1.5625f;
            acc.c[3] += r < 1.953125f;
        }
        return 0.f;
    }
};
// l4p_metric_depth_full: the alignment in inverse depth, and the second error pass of every alignment (the log-space sums)
__device__ __forceinline__ float met_depth_aligned(const float* x, const MetParams& p, float s, float t, bool inv) {
    if (!inv) {
        const float m = s * x[0];
        return fminf(fmaxf(m + t, p.dmin), p.dmax);
    }
    const float xi = 1.f / x[0];
    const float m = s * xi;
    const float pc = fminf(fmaxf(m + t, 1.f / p.dmax), 1.f / p.dmin);
    return fminf(fmaxf(1.f / pc, p.dmin), p.dmax);
}
template <> struct MetElem<MET_DEPTH_LSQ_INV> {
    static constexpr int NS = 3, NF = 4, NC = 1;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float, float, MetAcc& acc) {
        if (met_depth_ok(x, p)) {
            const float xi = 1.f / x[0], yi = 1.f / x[1];
            const double e = xi, g = yi;
            acc.f[0] += e;
            acc.f[1] += e * e;
            acc.f[2] += g;
            acc.f[3] += e * g;
            acc.c[0] += 1;
        }
        return 0.f;
    }
};
template <> struct MetElem<MET_DEPTH_ERR_INV> {  // MET_DEPTH_ERR on the inverse-depth aligned value
    static constexpr int NS = 3, NF = 2, NC = 4;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float s, float t, MetAcc& acc) {
        if (met_depth_ok(x, p) && s == s && t == t) {
            const float g = x[1];
            const float a = met_depth_aligned(x, p, s, t, true);
            const float d = a - g;
            acc.f[0] += (double)(fabsf(d) / g);
            acc.f[1] += (double)(d * d);
            const float r = fmaxf(a / g, g / a);
            acc.c[0] += 1;
            acc.c[1] += r < 1.25f;
            acc.c[2] += r < 1.5625f;
            acc.c[3] += r < 1.953125f;
        }
        return 0.f;
    }
};
template <> struct MetElem<MET_DEPTH_LOG> {  // sums of (d * d) / gt, l, l * l, |l| with l = log(a) - log(gt) in f64
    static constexpr int NS = 3, NF = 4, NC = 1;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams& p, float s, float t, MetAcc& acc) {
        if (met_depth_ok(x, p) && s == s && t == t) {
            const float g = x[1];
            const float a = met_depth_aligned(x, p, s, t, p.inv != 0);
            const float d = a - g;
            const float dd = d * d;
            const double l = log((double)a) - log((double)g);
            acc.f[0] += (double)(dd / g);
            acc.f[1] += l;
            acc.f[2] += l * l;
            acc.f[3] += fabs(l);
            acc.c[0] += 1;
        }
        return 0.f;
    }
};
// x[0], x[1] = est u, v; x[2], x[3] = gt u, v; x[4], x[5] = valid u, v
template <> struct MetElem<MET_FLOW> {
    static constexpr int NS = 6, NF = 1, NC = 4;
    __device__ static void streams(const MetParams& p, int b, const float** s) {
        s[0] = p.a + 2 * b * p.n, s[1] = s[0] + p.n, s[2] = p.g + 2 * b * p.n, s[3] = s[2] + p.n;
        s[4] = p.v ? p.v + 2 * b * p.n : nullptr, s[5] = p.v ? s[4] + p.n : nullptr;
    }
    __device__ static __forceinline__ float run(const float* x, const MetParams&, float, float, MetAcc& acc) {
        if (x[4] > 0.5f && x[5] > 0.5f && met_finite(x[2]) && met_finite(x[3])) {
            const float du = x[0] - x[2], dv = x[1] - x[3];
            const float uu = du * du, vv = dv * dv;
            const float epe = sqrtf(uu + vv);
            acc.f[0] += (double)epe;
            acc.c[0] += 1;
            acc.c[1] += epe < 1.f;
            acc.c[2] += epe < 3.f;
            acc.c[3] += epe < 5.f;
        }
        return 0.f;
    }
};
// x[0] = logit, x[1] = gt, x[2] = valid; counts TP, FP, FN, TN
template <> struct MetElem<MET_MASK> {
    static constexpr int NS = 3, NF = 0, NC = 4;
    __device__ static void streams(const MetParams& p, int b, const float** s) { MetElem<MET_DEPTH_QUOT>::streams(p, b, s); }
    __device__ static __forceinline__ float run(const float* x, const MetParams&, float, float, MetAcc& acc) {
        if (x[2] > 0.5f) {
            const bool pp = x[0] > 0.f, gp = x[1] > 0.5f;
            acc.c[0] += pp && gp;
            acc.c[1] += pp && !gp;
            acc.c[2] += !pp && gp;
            acc.c[3] += !pp && !gp;
        }
        return 0.f;
    }
};

// scratch: [B][gridDim.x][MET_SLOTS] 8-byte slots
template <int MODE>
__global__ __launch_bounds__(256) void met_dense_kernel(MetParams p, unsigned long long* __restrict__ scratch) {
    typedef MetElem<MODE> E;
    constexpr int NS = E::NS, NF = E::NF, NC = E::NC;
    const int b = blockIdx.y;
    const long long n = p.n;
    const float* s[NS];
    E::streams(p, b, s);
    float* q = MODE == MET_DEPTH_QUOT ? p.quot + b * n : nullptr;
    float sc = 1.f, sh = 0.f;
    if ((MODE == MET_DEPTH_ERR || MODE == MET_DEPTH_ERR_INV || MODE == MET_DEPTH_LOG) && p.sol) sc = p.sol[2 * b], sh = p.sol[2 * b + 1];
    // 16-byte path only when every array of this clip sits at the same offset inside a 16-byte line
    const unsigned mis = (unsigned)((uintptr_t)s[0] & 15u);
    bool vec = (mis & 3u) == 0;
#pragma unroll
    for (int k = 1; k < NS; ++k) vec = vec && (!s[k] || (unsigned)((uintptr_t)s[k] & 15u) == mis);
    if (q) vec = vec && (unsigned)((uintptr_t)q & 15u) == mis;
    long long head = n;
    if (vec) {
        head = ((16u - mis) & 15u) >> 2;
        head = head < n ? head : n;
    }
    const long long nvec = (n - head) >> 2, tail = head + 4 * nvec;
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    MetAcc acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc.f[k] = 0.0, acc.c[k] = 0u;
    auto scalar = [&](long long i) {
        float x[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] = s[k] ? s[k][i] : 1.f;
        const float r = E::run(x, p, sc, sh, acc);
        if (MODE == MET_DEPTH_QUOT) q[i] = r;
    };
    for (long long i = tid; i < head; i += stride) scalar(i);
    for (long long w = tid; w < nvec; w += stride) {
        const long long i = head + 4 * w;
        f32x4 xv[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) xv[k] = s[k] ? *reinterpret_cast<const f32x4*>(s[k] + i) : (f32x4){1.f, 1.f, 1.f, 1.f};
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = xv[k][j];
            r[j] = E::run(x, p, sc, sh, acc);
        }
        if (MODE == MET_DEPTH_QUOT) *reinterpret_cast<f32x4*>(q + i) = r;
    }
    for (long long i = tail + tid; i < n; i += stride) scalar(i);

    __shared__ double redf[4][4];
    __shared__ unsigned redc[4][4];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc.f[k] += __shfl_xor(acc.f[k], o);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc.c[k] += (unsigned)__shfl_xor((int)acc.c[k], o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < NF; ++k) redf[wave][k] = acc.f[k];
        for (int k = 0; k < NC; ++k) redc[wave][k] = acc.c[k];
    }
    __syncthreads();
    unsigned long long* row = scratch + ((long long)b * gridDim.x + blockIdx.x) * MET_SLOTS;
    const int k = threadIdx.x;
    if (k < NF) row[k] = (unsigned long long)__double_as_longlong(((redf[0][k] + redf[1][k]) + redf[2][k]) + redf[3][k]);
    if (k >= NF && k < NF + NC) {
        const int j = k - NF;
        row[k] = (unsigned long long)redc[0][j] + redc[1][j] + redc[2][j] + redc[3][j];
    }
}

// One workgroup per clip adds its nblocks rows in a fixed order, then thread 0 forms the results.
// cnt [B] (QUOT), sol [B][2] (LSQ: written; ERR: read, NULL = (1, 0)), out [B][ostride] (ERR, FLOW, MASK: MET_OUT columns from 0;
// LOG: columns 13 .. MET_FULL_OUT of the row whose first 13 the ERR pass has written)
template <int MODE>
__global__ __launch_bounds__(256) void met_finish_kernel(const unsigned long long* __restrict__ scratch, int nblocks,
                                                         unsigned long long* __restrict__ cnt, float* __restrict__ sol,
                                                         double* __restrict__ out, int ostride) {
    typedef MetElem<MODE> E;
    constexpr int NF = E::NF, NC = E::NC;
    __shared__ double redf[256][4];
    __shared__ unsigned long long redc[256][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    double f[4] = {0, 0, 0, 0};
    unsigned long long c[4] = {0, 0, 0, 0};
    for (int r = tid; r < nblocks; r += 256) {
        const unsigned long long* row = scratch + ((long long)b * nblocks + r) * MET_SLOTS;
        for (int k = 0; k < NF; ++k) f[k] += __longlong_as_double((long long)row[k]);
        for (int k = 0; k < NC; ++k) c[k] += row[NF + k];
    }
    for (int k = 0; k < 4; ++k) redf[tid][k] = f[k], redc[tid][k] = c[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < 4; ++k) redf[tid][k] += redf[tid + o][k], redc[tid][k] += redc[tid + o][k];
        __syncthreads();
    }
    if (tid != 0) return;
    for (int k = 0; k < 4; ++k) f[k] = redf[0][k], c[k] = redc[0][k];
    const double nan = met_nan();
    if (MODE == MET_DEPTH_QUOT) {
        cnt[b] = c[0];
    } else if (MODE == MET_DEPTH_LSQ || MODE == MET_DEPTH_LSQ_INV) {
        const double N = (double)c[0], se = f[0], see = f[1], sg = f[2], seg = f[3];
        const double det = N * see - se * se;
        double s = nan, t = nan;
        if (c[0] >= 2 && det > 0.0) {
            s = (N * seg - se * sg) / det;
            t = (see * sg - se * seg) / det;
        }
        sol[2 * b] = (float)s;
        sol[2 * b + 1] = (float)t;
    } else if (MODE == MET_DEPTH_LOG) {
        double* o = out + (long long)b * ostride;
        const double N = (double)c[0];
        for (int k = 0; k < 4; ++k) o[13 + k] = f[k];
        const double ml = f[1] / N, mll = f[2] / N;
        o[17] = c[0] ? f[0] / N : nan;
        o[18] = c[0] ? sqrt(mll) : nan;
        o[19] = c[0] ? (f[3] / N) / 2.302585092994046 : nan;
        o[20] = c[0] ? 100.0 * sqrt(fmax(mll - ml * ml, 0.0)) : nan;
        for (int k = 21; k < MET_FULL_OUT; ++k) o[k] = nan;
    } else {
        double* o = out + (long long)b * ostride;
        for (int k = 0; k < MET_OUT; ++k) o[k] = 0.0;
        if (MODE == MET_DEPTH_ERR || MODE == MET_DEPTH_ERR_INV) {
            const double N = (double)c[0];
            o[0] = N, o[1] = f[0], o[2] = f[1], o[3] = (double)c[1], o[4] = (double)c[2], o[5] = (double)c[3];
            o[6] = c[0] ? f[0] / N : nan;
            o[7] = c[0] ? sqrt(f[1] / N) : nan;
            for (int k = 0; k < 3; ++k) o[8 + k] = c[0] ? (double)c[1 + k] / N : nan;
            o[11] = sol ? (double)sol[2 * b] : 1.0;
            o[12] = sol ? (double)sol[2 * b + 1] : 0.0;
        } else if (MODE == MET_FLOW) {
            const double N = (double)c[0];
            o[0] = N, o[1] = f[0], o[2] = (double)c[1], o[3] = (double)c[2], o[4] = (double)c[3];
            o[5] = c[0] ? f[0] / N : nan;
            for (int k = 0; k < 3; ++k) o[6 + k] = c[0] ? (double)c[1 + k] / N : nan;
        } else {
            const double tp = (double)c[0], fp = (double)c[1], fn = (double)c[2], tn = (double)c[3];
            o[0] = tp, o[1] = fp, o[2] = fn, o[3] = tn;
            o[4] = c[0] + c[1] + c[2] ? tp / (tp + fp + fn) : nan;
            o[5] = c[0] + c[1] ? tp / (tp + fp) : nan;
            o[6] = c[0] + c[2] ? tp / (tp + fn) : nan;
            o[7] = c[0] + c[1] + c[2] ? 2.0 * tp / (2.0 * tp + fp + fn) : nan;
            o[8] = c[0] + c[1] + c[2] + c[3] ? (tp + tn) / (tp + fp + fn + tn) : nan;
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Tracks (TAP-Vid): one workgroup per (block of MET_TRK_TRACKS tracks, clip); integer atomics into the clip's counters
// (integer sums do not depend on the order).  counts [B][18]: scored, occlusion-correct, gt-visible, then per threshold
// 1, 2, 4, 8, 16: within & gt-visible [3..8), TP [8..13), FP [13..18).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void met_tracks_kernel(const float* __restrict__ traj_e, const float* __restrict__ traj_g,
                                                         const float* __restrict__ vis_logit, const unsigned char* __restrict__ vis_gt,
                                                         const unsigned char* __restrict__ valid, const float* __restrict__ queries,
                                                         int N, int T, float sx, float sy, unsigned long long* __restrict__ counts) {
    __shared__ unsigned lds[MET_TRK_COUNTS];
    const int b = blockIdx.y, i0 = blockIdx.x * MET_TRK_TRACKS;
    if (threadIdx.x < MET_TRK_COUNTS) lds[threadIdx.x] = 0u;
    __syncthreads();
    const int ntr = N - i0 < MET_TRK_TRACKS ? N - i0 : MET_TRK_TRACKS;
    const long long total = (long long)ntr * T;
    unsigned c[MET_TRK_COUNTS];
#pragma unroll
    for (int k = 0; k < MET_TRK_COUNTS; ++k) c[k] = 0u;
    for (long long e = threadIdx.x; e < total; e += 256) {
        const int i = i0 + (int)(e / T), t = (int)(e % T);
        const long long tr = (long long)b * N + i;
        const float qt = floorf(queries[tr * 3]);
        const bool ok = (valid ? valid[tr * T + t] != 0 : true) && (float)t != qt;
        if (!ok) continue;
        const float xe = traj_e[(tr * 2 + 0) * T + t], ye = traj_e[(tr * 2 + 1) * T + t];
        const float xg = traj_g[(tr * 2 + 0) * T + t], yg = traj_g[(tr * 2 + 1) * T + t];
        const float dx = (xe - xg) * sx, dy = (ye - yg) * sy;
        const float xx = dx * dx, yy = dy * dy;
        const float d2 = xx + yy;
        const bool pv = vis_logit[tr * T + t] > 0.f, gv = vis_gt[tr * T + t] != 0;
        c[0] += 1;
        c[1] += pv == gv;
        c[2] += gv;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float thr = (float)(1 << k);
            const bool within = d2 < thr * thr;
            c[3 + k] += within && gv;
            c[8 + k] += within && pv && gv;
            c[13 + k] += pv && !(gv && within);
        }
    }
#pragma unroll
    for (int k = 0; k < MET_TRK_COUNTS; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += (unsigned)__shfl_xor((int)c[k], o);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < MET_TRK_COUNTS; ++k)
            if (c[k]) atomicAdd(&lds[k], c[k]);
    __syncthreads();
    if (threadIdx.x < MET_TRK_COUNTS && lds[threadIdx.x])
        atomicAdd(&counts[(long long)b * MET_TRK_COUNTS + threadIdx.x], (unsigned long long)lds[threadIdx.x]);
}
__global__ void met_tracks_finish_kernel(const unsigned long long* __restrict__ counts, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long* c = counts + (long long)b * MET_TRK_COUNTS;
    double* o = out + (long long)b * MET_TRK_OUT;
    const double nan = met_nan();
    for (int k = 0; k < MET_TRK_COUNTS; ++k) o[k] = (double)c[k];
    o[18] = c[0] ? (double)c[1] / (double)c[0] : nan;
    double sp = 0.0, sj = 0.0;
    for (int k = 0; k < 5; ++k) {
        const double pts = c[2] ? (double)c[3 + k] / (double)c[2] : nan;
        const unsigned long long den = c[2] + c[13 + k];
        const double jac = den ? (double)c[8 + k] / (double)den : nan;
        o[19 + k] = pts;
        o[24 + k] = jac;
        sp += pts;
        sj += jac;
    }
    o[29] = sp / 5.0;
    o[30] = sj / 5.0;
    o[31] = 0.0;
}

// -------------------------------------------------------------------------------------------------
// 3D tracks: camera-space points from (x, y, z) and the gt intrinsics, one scale per clip or per track, depth-adaptive
// thresholds.  Up to three launches before the finish: the ratios |G| / |E| of the eligible frames (+inf elsewhere) with their
// counts per clip and per track; the scale (the radix select of l4p_select_median_dev for the clip, met_t3d_track_median_kernel
// per track, met_t3d_query_scale_kernel at the query frame); the scoring pass in met_tracks_kernel's pattern.
// -------------------------------------------------------------------------------------------------
struct MetT3d {
    const float *traj_e, *traj_g, *z_e, *z_g, *vis_logit;
    const unsigned char *vis_gt, *valid;
    const float *queries, *K;
    int N, T;
    float sx, sy;
};
struct MetT3dFrame {
    bool scored, eligible, gv;
    float ex, ey, ez, gx, gy, gz, f;
};
__device__ __forceinline__ float met_norm3(float x, float y, float z) {
    const float xx = x * x, yy = y * y, zz = z * z;
    return sqrtf((xx + yy) + zz);
}
// frame t of track tr = b * N + i
__device__ __forceinline__ MetT3dFrame met_t3d_frame(const MetT3d& p, int b, long long tr, int t) {
    MetT3dFrame r;
    const float qt = floorf(p.queries[tr * 3]);
    const float zg = p.z_g[tr * p.T + t], ze = p.z_e[tr * p.T + t];
    r.scored = (p.valid ? p.valid[tr * p.T + t] != 0 : true) && (float)t != qt && met_finite(zg) && zg > 0.f;
    r.gv = p.vis_gt[tr * p.T + t] != 0;
    r.eligible = r.scored && r.gv && met_finite(ze) && ze > 0.f;
    const float* K = p.K + (long long)b * 16 * p.T + t;
    const float fx = K[0], fy = K[5 * (long long)p.T], cx = K[2 * (long long)p.T], cy = K[6 * (long long)p.T];
    const float xe = p.traj_e[(tr * 2 + 0) * p.T + t], ye = p.traj_e[(tr * 2 + 1) * p.T + t];
    const float xg = p.traj_g[(tr * 2 + 0) * p.T + t], yg = p.traj_g[(tr * 2 + 1) * p.T + t];
    r.ex = ((xe - cx) * ze) / fx, r.ey = ((ye - cy) * ze) / fy, r.ez = ze;
    r.gx = ((xg - cx) * zg) / fx, r.gy = ((yg - cy) * zg) / fy, r.gz = zg;
    r.f = sqrtf((fx * p.sx) * (fy * p.sy));
    return r;
}
// ratio [B][N][T]: r of the eligible frames, +inf elsewhere; cnt_clip [B] (cleared by the caller), cnt_track [B][N] or NULL
__global__ __launch_bounds__(256) void met_t3d_ratio_kernel(MetT3d p, float* __restrict__ ratio, unsigned long long* __restrict__ cnt_clip,
                                                            unsigned* __restrict__ cnt_track) {
    __shared__ unsigned lds[MET_TRK_TRACKS];
    const int b = blockIdx.y, i0 = blockIdx.x * MET_TRK_TRACKS, T = p.T;
    if (threadIdx.x < MET_TRK_TRACKS) lds[threadIdx.x] = 0u;
    __syncthreads();
    const int ntr = p.N - i0 < MET_TRK_TRACKS ? p.N - i0 : MET_TRK_TRACKS;
    const long long total = (long long)ntr * T;
    for (long long e = threadIdx.x; e < total; e += 256) {
        const int k = (int)(e / T), t = (int)(e % T);
        const long long tr = (long long)b * p.N + i0 + k;
        const MetT3dFrame fr = met_t3d_frame(p, b, tr, t);
        float r = __uint_as_float(0x7F800000u);
        if (fr.eligible) {
            r = met_norm3(fr.gx, fr.gy, fr.gz) / met_norm3(fr.ex, fr.ey, fr.ez);
            atomicAdd(&lds[k], 1u);
        }
        ratio[tr * T + t] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < ntr) {
        const unsigned c = lds[threadIdx.x];
        if (cnt_track) cnt_track[(long long)b * p.N + i0 + threadIdx.x] = c;
        if (c) atomicAdd(&cnt_clip[b], (unsigned long long)c);
    }
}
__device__ __forceinline__ unsigned met_key(float x) {  // order-preserving image of the bit pattern
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// One wave per track: the order statistic (c - 1) / 2 of the track's T ratios (the c eligible ones sort below the +inf of the
// others) by rank counting, ties broken by the frame index, frames walked in chunks of 64.  scale [B][N]; nfin [B]: tracks with a
// finite scale (integer atomics).
__global__ __launch_bounds__(256) void met_t3d_track_median_kernel(const float* __restrict__ ratio, const unsigned* __restrict__ cnt_track,
                                                                   int N, int T, float* __restrict__ scale,
                                                                   unsigned long long* __restrict__ nfin) {
    const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const long long tr = (long long)b * N + i;
    const float* r = ratio + tr * T;
    const unsigned c = cnt_track[tr];
    if (c == 0u) {
        if (lane == 0) scale[tr] = __uint_as_float(0x7FC00000u);
        return;
    }
    const int want = (int)((c - 1u) / 2u);
    for (int m = lane; m < T; m += 64) {
        const float v = r[m];
        const unsigned km = met_key(v);
        int rank = 0;
        for (int q = 0; q < T; ++q) {
            const unsigned kq = met_key(r[q]);
            rank += (kq < km) || (kq == km && q < m);
        }
        if (rank == want) {  // exactly one frame of the track
            scale[tr] = v;
            if (met_finite(v)) atomicAdd(&nfin[b], 1ull);
        }
    }
}
// s_i = zg / ze at the query frame
__global__ void met_t3d_query_scale_kernel(MetT3d p, int B, float* __restrict__ scale, unsigned long long* __restrict__ nfin) {
    const long long tr = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (tr >= (long long)B * p.N) return;
    const float qt = floorf(p.queries[tr * 3]);
    float s = __uint_as_float(0x7FC00000u);
    if (qt >= 0.f && qt < (float)p.T) {
        const int t = (int)qt;
        const float zg = p.z_g[tr * p.T + t], ze = p.z_e[tr * p.T + t];
        if ((p.valid ? p.valid[tr * p.T + t] != 0 : true) && met_finite(zg) && zg > 0.f && met_finite(ze) && ze > 0.f) s = zg / ze;
    }
    scale[tr] = s;
    if (met_finite(s)) atomicAdd(&nfin[tr / p.N], 1ull);
}
// scale: NULL (1), [B] (per_track = 0) or [B][N]; counts as met_tracks_kernel
__global__ __launch_bounds__(256) void met_t3d_score_kernel(MetT3d p, const float* __restrict__ scale, int per_track,
                                                            unsigned long long* __restrict__ counts) {
    __shared__ unsigned lds[MET_TRK_COUNTS];
    const int b = blockIdx.y, i0 = blockIdx.x * MET_TRK_TRACKS, T = p.T;
    if (threadIdx.x < MET_TRK_COUNTS) lds[threadIdx.x] = 0u;
    __syncthreads();
    const int ntr = p.N - i0 < MET_TRK_TRACKS ? p.N - i0 : MET_TRK_TRACKS;
    const long long total = (long long)ntr * T;
    unsigned c[MET_TRK_COUNTS];
#pragma unroll
    for (int k = 0; k < MET_TRK_COUNTS; ++k) c[k] = 0u;
    for (long long e = threadIdx.x; e < total; e += 256) {
        const int t = (int)(e % T);
        const long long tr = (long long)b * p.N + i0 + (int)(e / T);
        const MetT3dFrame fr = met_t3d_frame(p, b, tr, t);
        if (!fr.scored) continue;
        const float s = !scale ? 1.f : per_track ? scale[tr] : scale[b];
        const float dx = s * fr.ex - fr.gx, dy = s * fr.ey - fr.gy, dz = s * fr.ez - fr.gz;
        const float d = met_norm3(dx, dy, dz);
        const float u = fr.gz / fr.f;
        const bool pv = p.vis_logit[tr * T + t] > 0.f, gv = fr.gv;
        c[0] += 1;
        c[1] += pv == gv;
        c[2] += gv;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float thr = (float)(1 << k);
            const bool within = d < thr * u;
            c[3 + k] += within && gv;
            c[8 + k] += within && pv && gv;
            c[13 + k] += pv && !(gv && within);
        }
    }
#pragma unroll
    for (int k = 0; k < MET_TRK_COUNTS; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += (unsigned)__shfl_xor((int)c[k], o);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < MET_TRK_COUNTS; ++k)
            if (c[k]) atomicAdd(&lds[k], c[k]);
    __syncthreads();
    if (threadIdx.x < MET_TRK_COUNTS && lds[threadIdx.x])
        atomicAdd(&counts[(long long)b * MET_TRK_COUNTS + threadIdx.x], (unsigned long long)lds[threadIdx.x]);
}
// out[31] after met_tracks_finish_kernel: the clip's scale (scale [B], NULL = 1) or the number of tracks with a finite one
__global__ void met_t3d_scale_out_kernel(const float* __restrict__ scale, const unsigned long long* __restrict__ nfin, int B,
                                         double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[(long long)b * MET_TRK_OUT + 31] = nfin ? (double)nfin[b] : scale ? (double)scale[b] : 1.0;
}

// -------------------------------------------------------------------------------------------------
// Cameras: ATE / RPE with the RMSE statistic, one workgroup per clip, f64 throughout.
// -------------------------------------------------------------------------------------------------
struct MetRt {  // x -> r x + t
    double r[3][3], t[3];
};
__device__ __forceinline__ MetRt met_load_rt(const float* __restrict__ base, int T, int t) {  // base: [16][T] row-major 4x4
    MetRt m;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m.r[i][j] = (double)base[(long long)(i * 4 + j) * T + t];
        m.t[i] = (double)base[(long long)(i * 4 + 3) * T + t];
    }
    return m;
}
__device__ MetRt met_inv_rt(const MetRt& m) {
    const double(*a)[3] = m.r;
    double c[3][3];  // cofactors
    c[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    c[0][1] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    c[0][2] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    c[1][0] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
    c[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
    c[1][2] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    c[2][0] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    c[2][1] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    c[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
    MetRt o;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o.r[i][j] = c[j][i] / det;
    for (int i = 0; i < 3; ++i) o.t[i] = -(o.r[i][0] * m.t[0] + o.r[i][1] * m.t[1] + o.r[i][2] * m.t[2]);
    return o;
}
__device__ MetRt met_mul_rt(const MetRt& a, const MetRt& b) {
    MetRt o;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o.r[i][j] = a.r[i][0] * b.r[0][j] + a.r[i][1] * b.r[1][j] + a.r[i][2] * b.r[2][j];
        o.t[i] = a.r[i][0] * b.t[0] + a.r[i][1] * b.t[1] + a.r[i][2] * b.t[2] + a.t[i];
    }
    return o;
}
// sums of K doubles over the 256 threads in a fixed order; every thread reads the result from res[]
template <int K> __device__ void met_block_sum(double* v, double (*red)[16], double* res) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if ((int)threadIdx.x < K) res[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
}
__global__ __launch_bounds__(256) void met_cameras_kernel(const float* __restrict__ pose_est, const float* __restrict__ extr_gt, int T,
                                                          double* __restrict__ out) {
    __shared__ double red[4][16];
    __shared__ double res[16];
    __shared__ double model[13];
    const int b = blockIdx.x;
    const float* pe = pose_est + (long long)b * 16 * T;
    const float* ex = extr_gt + (long long)b * 16 * T;
    double v[16];
    // centres: means
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) {
        const MetRt P = met_load_rt(pe, T, t), G = met_inv_rt(met_load_rt(ex, T, t));
        for (int k = 0; k < 3; ++k) v[k] += P.t[k], v[3 + k] += G.t[k];
    }
    met_block_sum<6>(v, red, res);
    double ms[3], md[3];
    for (int k = 0; k < 3; ++k) ms[k] = res[k] / T, md[k] = res[3 + k] / T;
    // covariance E[(gt - md)(est - ms)^T] and the variance of the estimate
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) {
        const MetRt P = met_load_rt(pe, T, t), G = met_inv_rt(met_load_rt(ex, T, t));
        double ds[3], dd[3];
        for (int k = 0; k < 3; ++k) {
            ds[k] = P.t[k] - ms[k];
            dd[k] = G.t[k] - md[k];
            v[9] += ds[k] * ds[k];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v[i * 3 + j] += dd[i] * ds[j];
    }
    met_block_sum<10>(v, red, res);
    if (threadIdx.x == 0) {
        double cov[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) cov[i][j] = res[i * 3 + j] / T;
        umeyama_from_moments<double>(ms, md, cov, res[9] / T, model);
    }
    __syncthreads();
    // errors
    const double sc = model[12];
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) {
        MetRt P = met_load_rt(pe, T, t);
        const MetRt G = met_inv_rt(met_load_rt(ex, T, t));
        for (int i = 0; i < 3; ++i) {
            const double r = model[i * 3 + 0] * P.t[0] + model[i * 3 + 1] * P.t[1] + model[i * 3 + 2] * P.t[2] + model[9 + i] - G.t[i];
            v[0] += r * r;
        }
        if (t + 1 < T) {
            MetRt P1 = met_load_rt(pe, T, t + 1);
            const MetRt G1 = met_inv_rt(met_load_rt(ex, T, t + 1));
            for (int k = 0; k < 3; ++k) P.t[k] *= sc, P1.t[k] *= sc;
            const MetRt relP = met_mul_rt(met_inv_rt(P), P1), relG = met_mul_rt(met_inv_rt(G), G1);
            const MetRt E = met_mul_rt(met_inv_rt(relG), relP);
            v[1] += E.t[0] * E.t[0] + E.t[1] * E.t[1] + E.t[2] * E.t[2];
            const double ax = E.r[2][1] - E.r[1][2], ay = E.r[0][2] - E.r[2][0], az = E.r[1][0] - E.r[0][1];
            const double sn = 0.5 * sqrt(ax * ax + ay * ay + az * az), cs = 0.5 * (E.r[0][0] + E.r[1][1] + E.r[2][2] - 1.0);
            const double deg = atan2(sn, cs) * (180.0 / 3.14159265358979323846);
            v[2] += deg * deg;
        }
    }
    met_block_sum<3>(v, red, res);
    if (threadIdx.x != 0) return;
    double* o = out + (long long)b * MET_CAM_OUT;
    o[0] = sqrt(res[0] / T);
    o[1] = sqrt(res[1] / (T - 1));
    o[2] = sqrt(res[2] / (T - 1));
    o[3] = sc;
    o[4] = res[0], o[5] = res[1], o[6] = res[2];
    o[7] = (double)T;
}

// ------------------------------------------------------------------------------------------------- host side
static inline int met_blocks(long long n) {
    const long long g = (n + 4095) / 4096;
    return (int)(g < 1 ? 1 : g > MET_MAX_BLOCKS ? MET_MAX_BLOCKS : g);
}
static inline size_t met_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct MetWs {
    unsigned long long* scratch;
    unsigned long long* cnt;
    float* sol;
    unsigned* qsel;
    float* quot;
    size_t bytes;
};
static MetWs met_ws_layout(void* base, int B, long long n, int mode) {
    MetWs w;
    size_t off = 0;
    char* p = (char*)base;
    w.scratch = (unsigned long long*)(p + off), off += met_align((size_t)B * MET_MAX_BLOCKS * MET_SLOTS * 8);
    w.cnt = (unsigned long long*)(p + off), off += met_align((size_t)B * 8);
    w.sol = (float*)(p + off), off += met_align((size_t)B * 2 * 4);
    w.qsel = (unsigned*)(p + off), w.quot = nullptr;
    if (mode == L4P_DEPTH_ALIGN_MEDIAN) {
        off += met_align((size_t)B * L4P_QUANTILE_WS_UINTS * 4);
        w.quot = (float*)(p + off), off += met_align((size_t)B * (size_t)n * 4);
    }
    w.bytes = off;
    return w;
}
template <int MODE>
static void met_launch_dense(hipStream_t s, const MetParams& p, int B, const MetWs& w, float* sol, double* out, int ostride = MET_OUT) {
    const int g = met_blocks(p.n);
    hipLaunchKernelGGL(met_dense_kernel<MODE>, dim3(g, B), dim3(256), 0, s, p, w.scratch);
    hipLaunchKernelGGL(met_finish_kernel<MODE>, dim3(B), dim3(256), 0, s, w.scratch, g, w.cnt, sol, out, ostride);
}

extern "C" {

size_t l4p_metric_ws_bytes(int B, long long n, int mode) {
    if (B < 1 || n < 1 || n > 0x7FFFFFFFll || (long long)B * n > 0x7FFFFFFFll || mode < 0 || mode > L4P_DEPTH_ALIGN_LSTSQ) return 0;
    return met_ws_layout(nullptr, B, n, mode).bytes;
}

static int met_dense_args_ok(const char* who, const void* a, const void* g, int B, long long n, const void* ws, size_t ws_bytes,
                             size_t need, const void* out) {
    if (B < 1 || n < 1 || n > 0x7FFFFFFFll || (long long)B * n > 0x7FFFFFFFll || !a || !g || !ws || !out || ws_bytes < need) {
        l4p_set_error("%s: need B >= 1, n >= 1, B * n < 2^31, the estimate, the ground truth, out and a workspace of %zu bytes "
                      "(B=%d n=%lld ws_bytes=%zu)", who, need, B, n, ws_bytes);
        return 0;
    }
    return 1;
}

// l4p_metric_depth (full = false: modes up to LSTSQ, out [B][MET_OUT]) and l4p_metric_depth_full (modes up to LSTSQ_INV, out
// [B][MET_FULL_OUT]: the same passes write its first 13 columns, a second error pass the log-space ones)
static int met_depth(const char* who, bool full, l4p_stream s_, const float* est, const float* gt, const float* valid, int B,
                     long long n, int mode, float dmin, float dmax, void* ws, size_t ws_bytes, double* out) {
    hipStream_t s = (hipStream_t)s_;
    if (mode < 0 || mode > (full ? L4P_DEPTH_ALIGN_LSTSQ_INV : L4P_DEPTH_ALIGN_LSTSQ) || !(dmin > 0.f) || !(dmax > dmin)) {
        l4p_set_error("%s: unknown alignment mode %d or not 0 < dmin < dmax (dmin=%g dmax=%g)", who, mode, (double)dmin, (double)dmax);
        return L4P_E_INVALID;
    }
    const size_t need = full ? l4p_metric_depth_full_ws_bytes(B, n, mode) : l4p_metric_ws_bytes(B, n, mode);
    if (!met_dense_args_ok(who, est, gt, B, n, ws, ws_bytes, need, out)) return L4P_E_INVALID;
    const MetWs w = met_ws_layout(ws, B, n, mode);
    const bool inv = mode == L4P_DEPTH_ALIGN_LSTSQ_INV;
    const int ostride = full ? MET_FULL_OUT : MET_OUT;
    MetParams p = {est, gt, valid, n, dmin, dmax, nullptr, w.quot, inv};
    {
        ProfScope prof(PROF_ELEMENTWISE, s, "%s", who);
        if (mode == L4P_DEPTH_ALIGN_MEDIAN) {
            HIP_TRY(hipMemsetAsync(w.sol, 0, (size_t)B * 2 * sizeof(float), s));
            met_launch_dense<MET_DEPTH_QUOT>(s, p, B, w, w.sol, out);
        } else if (mode == L4P_DEPTH_ALIGN_LSTSQ) {
            met_launch_dense<MET_DEPTH_LSQ>(s, p, B, w, w.sol, out);
        } else if (inv) {
            met_launch_dense<MET_DEPTH_LSQ_INV>(s, p, B, w, w.sol, out);
        }
        HIP_TRY(hipGetLastError());
    }
    if (mode == L4P_DEPTH_ALIGN_MEDIAN) {
        const int rc = l4p_select_median_dev(s_, w.quot, n, B, w.cnt, 1, w.qsel, w.sol, 2);
        if (rc) return rc;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "%s", who);
    float* sol = mode == L4P_DEPTH_ALIGN_NONE ? nullptr : w.sol;
    p.sol = sol;
    if (inv)
        met_launch_dense<MET_DEPTH_ERR_INV>(s, p, B, w, sol, out, ostride);
    else
        met_launch_dense<MET_DEPTH_ERR>(s, p, B, w, sol, out, ostride);
    if (full) met_launch_dense<MET_DEPTH_LOG>(s, p, B, w, sol, out, ostride);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_metric_depth(l4p_stream s_, const float* est, const float* gt, const float* valid, int B, long long n, int mode, float dmin,
                     float dmax, void* ws, size_t ws_bytes, double* out) {
    return met_depth("l4p_metric_depth", false, s_, est, gt, valid, B, n, mode, dmin, dmax, ws, ws_bytes, out);
}

size_t l4p_metric_depth_full_ws_bytes(int B, long long n, int align) {
    if (B < 1 || n < 1 || n > 0x7FFFFFFFll || (long long)B * n > 0x7FFFFFFFll || align < 0 || align > L4P_DEPTH_ALIGN_LSTSQ_INV) return 0;
    return met_ws_layout(nullptr, B, n, align).bytes;
}

int l4p_metric_depth_full(l4p_stream s_, const float* est, const float* gt, const float* valid, int B, long long n, int align,
                          float dmin, float dmax, void* ws, size_t ws_bytes, double* out) {
    return met_depth("l4p_metric_depth_full", true, s_, est, gt, valid, B, n, align, dmin, dmax, ws, ws_bytes, out);
}

int l4p_metric_flow(l4p_stream s_, const float* est, const float* gt, const float* valid, int B, long long n, void* ws,
                    size_t ws_bytes, double* out) {
    hipStream_t s = (hipStream_t)s_;
    if (B >= 1 && n >= 1 && 2 * (long long)B * n > 0x7FFFFFFFll) {
        l4p_set_error("l4p_metric_flow: need 2 * B * n < 2^31 (B=%d n=%lld)", B, n);
        return L4P_E_INVALID;
    }
    if (!met_dense_args_ok("l4p_metric_flow", est, gt, B, n, ws, ws_bytes, l4p_metric_ws_bytes(B, n, L4P_DEPTH_ALIGN_NONE), out))
        return L4P_E_INVALID;
    const MetWs w = met_ws_layout(ws, B, n, L4P_DEPTH_ALIGN_NONE);
    const MetParams p = {est, gt, valid, n, 0.f, 0.f, nullptr, nullptr};
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_flow");
    met_launch_dense<MET_FLOW>(s, p, B, w, nullptr, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_metric_mask(l4p_stream s_, const float* logit, const float* gt, const float* valid, int B, long long n, void* ws,
                    size_t ws_bytes, double* out) {
    hipStream_t s = (hipStream_t)s_;
    if (!met_dense_args_ok("l4p_metric_mask", logit, gt, B, n, ws, ws_bytes, l4p_metric_ws_bytes(B, n, L4P_DEPTH_ALIGN_NONE), out))
        return L4P_E_INVALID;
    const MetWs w = met_ws_layout(ws, B, n, L4P_DEPTH_ALIGN_NONE);
    const MetParams p = {logit, gt, valid, n, 0.f, 0.f, nullptr, nullptr};
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_mask");
    met_launch_dense<MET_MASK>(s, p, B, w, nullptr, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_metric_tracks(l4p_stream s_, const float* traj_est, const float* traj_gt, const float* vis_logit, const unsigned char* vis_gt,
                      const unsigned char* valid, const float* queries, int B, int N, int T, int H, int W,
                      unsigned long long* counts, double* out) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || N < 1 || T < 1 || H < 1 || W < 1 || 2 * (long long)B * N * T > 0x7FFFFFFFll || !traj_est || !traj_gt || !vis_logit ||
        !vis_gt || !queries || !counts || !out) {
        l4p_set_error("l4p_metric_tracks: need B, N, T, H, W >= 1, 2 * B * N * T < 2^31 and every pointer but valid "
                      "(B=%d N=%d T=%d H=%d W=%d)", B, N, T, H, W);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_tracks");
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)B * MET_TRK_COUNTS * sizeof(unsigned long long), s));
    const float sx = 256.f / (float)W, sy = 256.f / (float)H;
    hipLaunchKernelGGL(met_tracks_kernel, dim3((N + MET_TRK_TRACKS - 1) / MET_TRK_TRACKS, B), dim3(256), 0, s, traj_est, traj_gt,
                       vis_logit, vis_gt, valid, queries, N, T, sx, sy, counts);
    hipLaunchKernelGGL(met_tracks_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, counts, B, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

struct MetT3dWs {
    unsigned long long *cnt_clip, *nfin;  // [B] each, adjacent: one memset
    float* scale;                         // [B] (NONE, MEDIAN) or [B][N]
    unsigned* qsel;                       // MEDIAN
    unsigned* cnt_track;                  // TRACK_MEDIAN: [B][N]
    float* ratio;                         // MEDIAN, TRACK_MEDIAN: [B][N][T]
    size_t bytes;
};
static MetT3dWs met_t3d_ws_layout(void* base, int B, int N, int T, int scale) {
    MetT3dWs w = {};
    size_t off = 0;
    char* p = (char*)base;
    const bool per_track = scale == L4P_TRACK3D_SCALE_TRACK_MEDIAN || scale == L4P_TRACK3D_SCALE_QUERY;
    w.cnt_clip = (unsigned long long*)(p + off), w.nfin = w.cnt_clip + B, off += met_align((size_t)B * 2 * 8);
    w.scale = (float*)(p + off), off += met_align((size_t)B * (per_track ? N : 1) * 4);
    if (scale == L4P_TRACK3D_SCALE_MEDIAN) w.qsel = (unsigned*)(p + off), off += met_align((size_t)B * L4P_QUANTILE_WS_UINTS * 4);
    if (scale == L4P_TRACK3D_SCALE_TRACK_MEDIAN) w.cnt_track = (unsigned*)(p + off), off += met_align((size_t)B * N * 4);
    if (scale == L4P_TRACK3D_SCALE_MEDIAN || scale == L4P_TRACK3D_SCALE_TRACK_MEDIAN)
        w.ratio = (float*)(p + off), off += met_align((size_t)B * N * T * 4);
    w.bytes = off;
    return w;
}
static bool met_t3d_shape_ok(int B, int N, int T, int scale) {
    return B >= 1 && N >= 1 && T >= 1 && (long long)B * N * T <= 0x7FFFFFFFll && scale >= 0 && scale <= L4P_TRACK3D_SCALE_QUERY;
}

size_t l4p_metric_tracks3d_ws_bytes(int B, int N, int T, int scale) {
    return met_t3d_shape_ok(B, N, T, scale) ? met_t3d_ws_layout(nullptr, B, N, T, scale).bytes : 0;
}

int l4p_metric_tracks3d(l4p_stream s_, const float* traj_est, const float* traj_gt, const float* depth_est, const float* depth_gt,
                        const float* vis_logit, const unsigned char* vis_gt, const unsigned char* valid, const float* queries,
                        const float* intrinsics, int B, int N, int T, int H, int W, int scale, void* ws, size_t ws_bytes,
                        unsigned long long* counts, double* out) {
    hipStream_t s = (hipStream_t)s_;
    const size_t need = l4p_metric_tracks3d_ws_bytes(B, N, T, scale);
    if (!need || H < 1 || W < 1 || !traj_est || !traj_gt || !depth_est || !depth_gt || !vis_logit || !vis_gt || !queries || !intrinsics ||
        !ws || ws_bytes < need || !counts || !out) {
        l4p_set_error("l4p_metric_tracks3d: need B, N, T, H, W >= 1, B * N * T < 2^31, a scale mode 0..3, every pointer but valid and a "
                      "workspace of %zu bytes (B=%d N=%d T=%d H=%d W=%d scale=%d ws_bytes=%zu)", need, B, N, T, H, W, scale, ws_bytes);
        return L4P_E_INVALID;
    }
    const MetT3dWs w = met_t3d_ws_layout(ws, B, N, T, scale);
    const MetT3d p = {traj_est, traj_gt, depth_est, depth_gt, vis_logit, vis_gt, valid, queries, intrinsics, N, T,
                      256.f / (float)W, 256.f / (float)H};
    const dim3 grid((N + MET_TRK_TRACKS - 1) / MET_TRK_TRACKS, B);
    const bool per_track = scale == L4P_TRACK3D_SCALE_TRACK_MEDIAN || scale == L4P_TRACK3D_SCALE_QUERY;
    {
        ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_tracks3d");
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)B * MET_TRK_COUNTS * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(w.cnt_clip, 0, (size_t)B * 2 * sizeof(unsigned long long), s));
        if (w.ratio) hipLaunchKernelGGL(met_t3d_ratio_kernel, grid, dim3(256), 0, s, p, w.ratio, w.cnt_clip, w.cnt_track);
        if (scale == L4P_TRACK3D_SCALE_TRACK_MEDIAN)
            hipLaunchKernelGGL(met_t3d_track_median_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, w.ratio, w.cnt_track, N, T, w.scale,
                               w.nfin);
        if (scale == L4P_TRACK3D_SCALE_QUERY)
            hipLaunchKernelGGL(met_t3d_query_scale_kernel, dim3((unsigned)(((long long)B * N + 255) / 256)), dim3(256), 0, s, p, B,
                               w.scale, w.nfin);
        HIP_TRY(hipGetLastError());
    }
    if (scale == L4P_TRACK3D_SCALE_MEDIAN) {
        const int rc = l4p_select_median_dev(s_, w.ratio, (long long)N * T, B, w.cnt_clip, 1, w.qsel, w.scale, 1);
        if (rc) return rc;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_tracks3d");
    const float* sc = scale == L4P_TRACK3D_SCALE_NONE ? nullptr : w.scale;
    hipLaunchKernelGGL(met_t3d_score_kernel, grid, dim3(256), 0, s, p, sc, per_track ? 1 : 0, counts);
    hipLaunchKernelGGL(met_tracks_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, counts, B, out);
    hipLaunchKernelGGL(met_t3d_scale_out_kernel, dim3((B + 63) / 64), dim3(64), 0, s, sc, per_track ? w.nfin : nullptr, B, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_metric_cameras(l4p_stream s_, const float* pose_est, const float* extr_gt, int B, int T, double* out) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || T < 3 || 16 * (long long)B * T > 0x7FFFFFFFll || !pose_est || !extr_gt || !out) {
        l4p_set_error("l4p_metric_cameras: need B >= 1, T >= 3 frames, 16 * B * T < 2^31, pose_est, extr_gt and out (B=%d T=%d)", B, T);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_metric_cameras");
    hipLaunchKernelGGL(met_cameras_kernel, dim3(B), dim3(256), 0, s, pose_est, extr_gt, T, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
