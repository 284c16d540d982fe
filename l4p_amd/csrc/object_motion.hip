// Object motion: the rigid motion of every moving object from frame t - 1 to frame t, the poses composed from it, and the object's
// pixels carried into its first frame's pose (DESIGN.md "Object motion and models").  Pairs are the labelling's own temporal edges
// (csrc/objects.hip): a pixel of object k and the pixel of the frame before that its backward flow points to, when that one lies on
// object k too.  Every sum over pixels is a 64-bit integer sum of fixed-point coordinates (steps of v / 256, the tables' rule),
// reduced over runs of equal (object, frame) inside a wave before it touches memory: no float is accumulated by atomics and every
// output is the same bit for bit on every run.  The rule - include/l4p_hip.h states it operation by operation - is f32 per pixel
// and f64 per (object, frame), compiled with -ffp-contract=off (Makefile); the tests hold the integer outputs bit for bit, and
// the models within f32 rounding, to a numpy restatement (tests/object_motion_restate.py).
#include "common.hpp"
#include "prof.hpp"
#include "umeyama_moments.hpp"

#define OM_MAX_PIXELS (1ll << 30)
#define OM_MAX_HW (1ll << 20)    // pairs per (object, frame): 2^20 products below 2^42 sum below 2^62, three a pair below 2^64
#define OM_MAX_ROWS (1ll << 27)  // K T
#define OM_FAR (1 << 21)         // a pair with a |d| of this many steps or more is dropped
// columns of the centre accumulator (pass 1) and of the moments (fit passes); the first 18 moments are the `moments` output
enum { OM_C_N = 0, OM_C_A = 1, OM_C_B = 4, OM_C_PIX = 7, OM_C_COLS = 8 };
enum { OM_M_N = 0, OM_M_DA = 1, OM_M_DB = 4, OM_M_C = 7, OM_M_AA = 16, OM_M_BB = 17, OM_M_FAR = 18, OM_M_COLS = 19, OM_M_OUT = 18 };

struct OmWs {
    unsigned long long* cacc;  // [rows][OM_C_COLS]
    unsigned long long* mom;   // [rows][OM_M_COLS]
    int* cen;                  // [rows][6]: c_a, c_b
    double* inv;               // [rows][12]: the inverse of the pose, R^T row-major then -R^T t
    size_t bytes;
};

static OmWs om_layout(void* ws, long long rows) {
    OmWs w;
    auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
    char* p = (char*)ws;
    size_t o = 0;
    w.cacc = (unsigned long long*)(p + o), o += up((size_t)rows * OM_C_COLS * 8);
    w.mom = (unsigned long long*)(p + o), o += up((size_t)rows * OM_M_COLS * 8);
    w.cen = (int*)(p + o), o += up((size_t)rows * 6 * 4);
    w.inv = (double*)(p + o), o += up((size_t)rows * 12 * 8);
    w.bytes = o;
    return w;
}

static bool om_sizes_ok(int T, int H, int W, int K) {
    return T >= 1 && H >= 1 && W >= 1 && (long long)H * W <= OM_MAX_HW && (long long)T * H * W <= OM_MAX_PIXELS && K >= 0 &&
           (long long)K * T <= OM_MAX_ROWS;
}

__device__ __forceinline__ bool om_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// The fixed-point triple of a point by the rule of l4p_objects_tables; false for a point that rule leaves out.
__device__ __forceinline__ bool om_fixed(const float* p, const float* __restrict__ grid, int* s) {
    const float v = grid[3];
    bool ok = v > 0.f && om_finite(v) && om_finite(p[0]) && om_finite(p[1]) && om_finite(p[2]);
    if (!ok) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = (p[a] - grid[a]) / v;
        const float f = floorf(q * 256.0f);
        ok = ok && f >= -268435456.f && f < 268435456.f;  // a NaN f fails
        s[a] = ok ? (int)f : 0;
    }
    return ok;
}

struct OmPair {
    int a[3], b[3];      // fixed point, frame t - 1 and frame t
    float pa[3], pb[3];  // the raw points
};

// The pair of pixel m = (t, y, x) of object k, t >= 1: the temporal edge of l4p_objects_label with the same-object test.
__device__ __forceinline__ bool om_pair(const int* __restrict__ object_id, const float* __restrict__ points, const float* __restrict__ flow,
                                        const float* __restrict__ grid, long long M, int H, int W, long long m, int k, int t, int x, int y,
                                        OmPair& p) {
    int xq = x, yq = y;
    if (flow) {
        const float u = flow[m], v = flow[M + m];
        if (!(om_finite(u) && om_finite(v))) return false;
        const float gx = floorf(((float)x + u) + 0.5f), gy = floorf(((float)y + v) + 0.5f);
        if (!(gx >= 0.f && gx < (float)W && gy >= 0.f && gy < (float)H)) return false;
        xq = (int)gx, yq = (int)gy;
    }
    const long long n = ((long long)(t - 1) * H + yq) * W + xq;  // inside [0, M): t >= 1 and (xq, yq) inside the frame
    if (object_id[n] != k) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.pa[a] = points[n * 3 + a], p.pb[a] = points[m * 3 + a];
    return om_fixed(p.pa, grid, p.a) && om_fixed(p.pb, grid, p.b);
}

// Pixel m of the launch: its row k T + t, or -1 off every object.
__device__ __forceinline__ int om_row(const int* __restrict__ object_id, long long M, int T, int H, int W, int K, long long m, int& k, int& t,
                                      int& x, int& y) {
    if (m >= M) return -1;
    k = object_id[m];
    if (k < 0 || k >= K) return -1;
    x = (int)(m % W), y = (int)((m / W) % H), t = (int)(m / ((long long)W * H));
    return k * T + t;
}

// The sums of the lanes of a wave that share a row, left in the first lane of each run of consecutive such lanes (a segmented suffix
// reduction by shuffles, the form of ob_acc_kernel); returns whether this lane is such a first lane.  Called by all 64 lanes.
template <int N>
__device__ __forceinline__ bool om_run_sums(int row, long long (&v)[N]) {
    const int lane = threadIdx.x & 63;
    const bool live = row >= 0;
    const int before = __shfl_up(row, 1, 64);
    const bool brk = lane == 0 || before != row;
    const unsigned run = (unsigned)__popcll(__ballot(brk) & (~0ull >> (63 - lane)));
    for (int d = 1; d < 64; d <<= 1) {
        const bool same = __shfl_down(run, d, 64) == run && lane + d < 64 && live;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const long long o = __shfl_down(v[i], d, 64);
            if (same) v[i] += o;
        }
    }
    return live && brk;
}

template <int N>
__device__ __forceinline__ void om_add_row(unsigned long long* __restrict__ dst, const long long (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (v[i] != 0) atomicAdd(dst + i, (unsigned long long)v[i]);  // two's complement: the signed sum
}

// -------------------------------------------------------------------------------------------------
// Pass 1, one thread per pixel: per (object, frame) the pixels, the pairs and the sums of a and of b.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void om_centre_kernel(const int* __restrict__ object_id, const float* __restrict__ points,
                                                        const float* __restrict__ flow, const float* __restrict__ grid, int T, int H, int W,
                                                        int K, unsigned long long* __restrict__ cacc) {
    const long long M = (long long)T * H * W;
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    int k = 0, t = 0, x = 0, y = 0;
    const int row = om_row(object_id, M, T, H, W, K, m, k, t, x, y);
    if (__ballot(row >= 0) == 0) return;  // a wave off every object (most are): the whole wave leaves together
    long long v[OM_C_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    OmPair p;
    if (row >= 0) {
        v[OM_C_PIX] = 1;
        if (t >= 1 && om_pair(object_id, points, flow, grid, M, H, W, m, k, t, x, y, p)) {
            v[OM_C_N] = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) v[OM_C_A + a] = p.a[a], v[OM_C_B + a] = p.b[a];
        }
    }
    if (om_run_sums(row, v)) om_add_row(cacc + (long long)row * OM_C_COLS, v);
}

__device__ __forceinline__ long long om_floor_div(long long s, long long n) {  // n > 0
    const long long q = s / n;
    return (s % n != 0 && s < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(256) void om_cen_kernel(const unsigned long long* __restrict__ cacc, long long rows, int* __restrict__ cen) {
    const long long r = blockIdx.x * 256ll + threadIdx.x;
    if (r >= rows) return;
    const long long n = (long long)cacc[r * OM_C_COLS + OM_C_N];
    for (int a = 0; a < 6; ++a) cen[r * 6 + a] = n > 0 ? (int)om_floor_div((long long)cacc[r * OM_C_COLS + OM_C_A + a], n) : 0;
}

// -------------------------------------------------------------------------------------------------
// Fit and refit passes, one thread per pixel: the 18 moments about the centres of pass 1 (and the far pairs).  REFIT counts only
// the pairs whose residual under the previous round's f32 model passes the test.
// -------------------------------------------------------------------------------------------------
template <bool REFIT>
__global__ __launch_bounds__(256) void om_fit_kernel(const int* __restrict__ object_id, const float* __restrict__ points,
                                                     const float* __restrict__ flow, const float* __restrict__ grid, int T, int H, int W,
                                                     int K, const int* __restrict__ cen, const float* __restrict__ model, float inlier_voxels,
                                                     unsigned long long* __restrict__ mom) {
    const long long M = (long long)T * H * W;
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    int k = 0, t = 0, x = 0, y = 0;
    int row = om_row(object_id, M, T, H, W, K, m, k, t, x, y);
    if (row >= 0 && t < 1) row = -1;  // frame 0 has no pairs
    if (__ballot(row >= 0) == 0) return;
    long long v[OM_M_COLS];
#pragma unroll
    for (int i = 0; i < OM_M_COLS; ++i) v[i] = 0;
    OmPair p;
    if (row >= 0 && om_pair(object_id, points, flow, grid, M, H, W, m, k, t, x, y, p)) {
        int da[3], db[3];
        bool far = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            da[a] = p.a[a] - cen[(long long)row * 6 + a], db[a] = p.b[a] - cen[(long long)row * 6 + 3 + a];  // |a|, |c| <= 2^28
            far = far || da[a] >= OM_FAR || da[a] <= -OM_FAR || db[a] >= OM_FAR || db[a] <= -OM_FAR;
        }
        bool in = !far;
        if (REFIT && in) {
            const float* mo = model + (long long)row * 12;
            const float tau = inlier_voxels * grid[3];
            float d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float pred = ((mo[a * 3] * p.pa[0] + mo[a * 3 + 1] * p.pa[1]) + mo[a * 3 + 2] * p.pa[2]) + mo[9 + a];
                d[a] = pred - p.pb[a];
            }
            in = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= tau * tau;  // a NaN residual fails
        }
        if (far) v[OM_M_FAR] = 1;
        if (in) {
            v[OM_M_N] = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[OM_M_DA + a] = da[a], v[OM_M_DB + a] = db[a];
                v[OM_M_AA] += (long long)da[a] * da[a], v[OM_M_BB] += (long long)db[a] * db[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) v[OM_M_C + a * 3 + b] = (long long)db[a] * da[b];
            }
        }
    }
    if (om_run_sums(row, v)) om_add_row(mom + (long long)row * OM_M_COLS, v);
}

struct OmTables {
    float* motion;
    int *n_pairs, *n_inliers, *n_far;
    float* rms;
    unsigned char* valid;
    long long* moments;
};

// -------------------------------------------------------------------------------------------------
// Solve, one thread per (object, frame), f64: means and centred sums from the moments, R from the closed form, t = B - R A, the RMS
// residual from the moments.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void om_solve_kernel(const unsigned long long* __restrict__ cacc, const unsigned long long* __restrict__ mom,
                                                      const int* __restrict__ cen, const float* __restrict__ grid, long long rows,
                                                      int min_pairs, OmTables o) {
    const long long r = blockIdx.x * 64ll + threadIdx.x;
    if (r >= rows) return;
    long long s[OM_M_COLS];
    for (int i = 0; i < OM_M_COLS; ++i) s[i] = (long long)mom[r * OM_M_COLS + i];
    if (o.moments)
        for (int i = 0; i < OM_M_OUT; ++i) o.moments[r * OM_M_OUT + i] = s[i];
    const long long ni = s[OM_M_N];
    const bool valid = ni >= min_pairs;
    o.n_pairs[r] = (int)cacc[r * OM_C_COLS + OM_C_N];
    o.n_inliers[r] = (int)ni, o.n_far[r] = (int)s[OM_M_FAR], o.valid[r] = valid ? 1 : 0;
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0}, rms = 0;
    if (ni >= 1) {
        const double n = (double)ni, q = (double)grid[3] / 256.0;
        double sa[3], sb[3], C[3][3], A[3], B[3];
        for (int a = 0; a < 3; ++a) sa[a] = (double)s[OM_M_DA + a], sb[a] = (double)s[OM_M_DB + a];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) C[a][b] = (double)s[OM_M_C + a * 3 + b] - (sb[a] * sa[b]) / n;
        // (the two sums of squares hold three products a pair: up to 3 * 2^62, past a signed 64-bit sum but not an unsigned one)
        const double Saa = (double)(unsigned long long)s[OM_M_AA] - ((sa[0] * sa[0] + sa[1] * sa[1]) + sa[2] * sa[2]) / n;
        const double Sbb = (double)(unsigned long long)s[OM_M_BB] - ((sb[0] * sb[0] + sb[1] * sb[1]) + sb[2] * sb[2]) / n;
        if (valid) {
            double cov[3][3], sigma_sum;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) cov[a][b] = C[a][b] / n;
            umeyama_rotation(cov, R, &sigma_sum);
        }
        for (int a = 0; a < 3; ++a) {
            A[a] = (double)grid[a] + (((double)cen[r * 6 + a] + sa[a] / n) + 0.5) * q;
            B[a] = (double)grid[a] + (((double)cen[r * 6 + 3 + a] + sb[a] / n) + 0.5) * q;
        }
        double tr = 0;
        for (int a = 0; a < 3; ++a) {
            t[a] = B[a] - ((R[a][0] * A[0] + R[a][1] * A[1]) + R[a][2] * A[2]);
            for (int b = 0; b < 3; ++b) tr += R[a][b] * C[a][b];
        }
        rms = q * sqrt(fmax(0.0, ((Sbb + Saa) - 2.0 * tr) / n));
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) o.motion[r * 12 + a * 3 + b] = (float)R[a][b];
        o.motion[r * 12 + 9 + a] = (float)t[a];
    }
    o.rms[r] = (float)rms;
}

// -------------------------------------------------------------------------------------------------
// Composition, one thread per object, f64 over the emitted (f32) motions: G[first] = I, G[t] = M[t] G[t - 1]; the pose rounded to
// f32, and the inverse R^T, -R^T t in f64 for the canonical points.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void om_compose_kernel(const unsigned long long* __restrict__ cacc, const float* __restrict__ motion,
                                                        const unsigned char* __restrict__ valid, int K, int T, float* __restrict__ pose,
                                                        unsigned char* __restrict__ pose_valid, double* __restrict__ inv) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    int first = T;  // the first frame with a pixel of the object
    for (int t = T - 1; t >= 0; --t)
        if (cacc[((long long)k * T + t) * OM_C_COLS + OM_C_PIX] != 0) first = t;
    double G[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    bool ok = true;
    for (int t = 0; t < T; ++t) {
        const long long r = (long long)k * T + t;
        if (t > first) {
            double Mo[12], N[12];
            for (int i = 0; i < 12; ++i) Mo[i] = (double)motion[r * 12 + i];
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) N[a * 3 + b] = (Mo[a * 3] * G[b] + Mo[a * 3 + 1] * G[3 + b]) + Mo[a * 3 + 2] * G[6 + b];
                N[9 + a] = ((Mo[a * 3] * G[9] + Mo[a * 3 + 1] * G[10]) + Mo[a * 3 + 2] * G[11]) + Mo[9 + a];
            }
            for (int i = 0; i < 12; ++i) G[i] = N[i];
            ok = ok && valid[r] != 0;
        }
        for (int i = 0; i < 12; ++i) pose[r * 12 + i] = (float)G[i];
        pose_valid[r] = ok ? 1 : 0;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) inv[r * 12 + a * 3 + b] = G[b * 3 + a];
            inv[r * 12 + 9 + a] = -((G[a] * G[9] + G[3 + a] * G[10]) + G[6 + a] * G[11]);
        }
    }
}

__global__ __launch_bounds__(256) void om_canonical_kernel(const int* __restrict__ object_id, const float* __restrict__ points,
                                                           const double* __restrict__ inv, long long M, long long HW, int T, int K,
                                                           float* __restrict__ canonical) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M) return;
    const int k = object_id[m];
    float c[3] = {__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000)};
    if (k >= 0 && k < K) {
        const double* g = inv + ((long long)k * T + m / HW) * 12;
        const double p[3] = {(double)points[m * 3], (double)points[m * 3 + 1], (double)points[m * 3 + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = (float)(((g[a * 3] * p[0] + g[a * 3 + 1] * p[1]) + g[a * 3 + 2] * p[2]) + g[9 + a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) canonical[m * 3 + a] = c[a];
}

__global__ __launch_bounds__(256) void om_place_kernel(const float* __restrict__ xyz, const int* __restrict__ object, const float* __restrict__ pose,
                                                       long long V, int K, int T, int t, float* __restrict__ out) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= V) return;
    const int k = object[i];
    float c[3] = {__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000)};
    if (k >= 0 && k < K) {
        const float* g = pose + ((long long)k * T + t) * 12;
        const float p[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = ((g[a * 3] * p[0] + g[a * 3 + 1] * p[1]) + g[a * 3 + 2] * p[2]) + g[9 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out[i * 3 + a] = c[a];
}

static unsigned om_blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

extern "C" {

size_t l4p_objects_motion_ws_bytes(int K, int T) {
    if (K < 1 || T < 1 || (long long)K * T > OM_MAX_ROWS) return 0;
    return om_layout(nullptr, (long long)K * T).bytes;
}

int l4p_objects_motion(l4p_stream s_, const int* object_id, const float* points, const float* flow, const float* grid, int T, int H, int W,
                       int K, int n_refits, float inlier_voxels, int min_pairs, void* ws, float* motion, int* n_pairs, int* n_inliers,
                       int* n_far, float* rms, unsigned char* valid, long long* moments, float* pose, unsigned char* pose_valid) {
    hipStream_t s = (hipStream_t)s_;
    const bool rows_ok = K == 0 || (ws && motion && n_pairs && n_inliers && n_far && rms && valid && pose && pose_valid);
    const bool knobs = n_refits >= 0 && inlier_voxels > 0.f && inlier_voxels <= 3.402823466e+38f && min_pairs >= 3;
    if (!om_sizes_ok(T, H, W, K) || !knobs || !object_id || !points || !grid || !rows_ok) {
        l4p_set_error("l4p_objects_motion: need T, H, W >= 1, H W <= 2^20, T H W <= 2^30, 0 <= K, K T <= 2^27, n_refits >= 0, "
                      "inlier_voxels finite and > 0, min_pairs >= 3, object_id, points, grid and, with K > 0, ws and every output but "
                      "moments (T=%d H=%d W=%d K=%d n_refits=%d inlier_voxels=%g min_pairs=%d)", T, H, W, K, n_refits,
                      (double)inlier_voxels, min_pairs);
        return L4P_E_INVALID;
    }
    if (K == 0) return 0;
    const long long M = (long long)T * H * W, rows = (long long)K * T;
    const OmWs w = om_layout(ws, rows);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_motion");
    OmTables o = {motion, n_pairs, n_inliers, n_far, rms, valid, moments};
    HIP_TRY(hipMemsetAsync(w.cacc, 0, (size_t)rows * OM_C_COLS * 8, s));
    hipLaunchKernelGGL(om_centre_kernel, dim3(om_blocks(M)), dim3(256), 0, s, object_id, points, flow, grid, T, H, W, K, w.cacc);
    hipLaunchKernelGGL(om_cen_kernel, dim3(om_blocks(rows)), dim3(256), 0, s, w.cacc, rows, w.cen);
    for (int round = 0; round <= n_refits; ++round) {
        HIP_TRY(hipMemsetAsync(w.mom, 0, (size_t)rows * OM_M_COLS * 8, s));
        if (round == 0)
            hipLaunchKernelGGL(om_fit_kernel<false>, dim3(om_blocks(M)), dim3(256), 0, s, object_id, points, flow, grid, T, H, W, K, w.cen,
                               (const float*)nullptr, inlier_voxels, w.mom);
        else
            hipLaunchKernelGGL(om_fit_kernel<true>, dim3(om_blocks(M)), dim3(256), 0, s, object_id, points, flow, grid, T, H, W, K, w.cen,
                               (const float*)motion, inlier_voxels, w.mom);
        hipLaunchKernelGGL(om_solve_kernel, dim3(om_blocks(rows, 64)), dim3(64), 0, s, w.cacc, w.mom, w.cen, grid, rows, min_pairs, o);
    }
    hipLaunchKernelGGL(om_compose_kernel, dim3(om_blocks(K, 64)), dim3(64), 0, s, w.cacc, motion, valid, K, T, pose, pose_valid, w.inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_objects_canonical(l4p_stream s_, const int* object_id, const float* points, const void* ws, int T, int H, int W, int K,
                          float* canonical) {
    hipStream_t s = (hipStream_t)s_;
    if (!om_sizes_ok(T, H, W, K) || !object_id || !points || !canonical || (K > 0 && !ws)) {
        l4p_set_error("l4p_objects_canonical: need the sizes of l4p_objects_motion, object_id, points, canonical and, with K > 0, the ws "
                      "that l4p_objects_motion left (T=%d H=%d W=%d K=%d)", T, H, W, K);
        return L4P_E_INVALID;
    }
    const long long HW = (long long)H * W, M = HW * T;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_canonical");
    const double* inv = K > 0 ? om_layout((void*)ws, (long long)K * T).inv : nullptr;
    hipLaunchKernelGGL(om_canonical_kernel, dim3(om_blocks(M)), dim3(256), 0, s, object_id, points, inv, M, HW, T, K, canonical);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_objects_place(l4p_stream s_, const float* xyz, const int* object, const float* pose, long long V, int K, int T, int t,
                      float* out) {
    hipStream_t s = (hipStream_t)s_;
    const bool rows_ok = V == 0 || (xyz && object && out && (K == 0 || pose));
    if (V < 0 || V > OM_MAX_PIXELS || K < 0 || T < 1 || (long long)K * T > OM_MAX_ROWS || t < 0 || t >= T || !rows_ok) {
        l4p_set_error("l4p_objects_place: need 0 <= V <= 2^30, 0 <= K, K T <= 2^27, 0 <= t < T and, with V > 0, xyz, object, out and (K > "
                      "0) pose (V=%lld K=%d T=%d t=%d)", V, K, T, t);
        return L4P_E_INVALID;
    }
    if (V == 0) return 0;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_place");
    hipLaunchKernelGGL(om_place_kernel, dim3(om_blocks(V)), dim3(256), 0, s, xyz, object, pose, V, K, T, t, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
