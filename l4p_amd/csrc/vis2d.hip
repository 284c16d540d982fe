// The demo's 2D result video (reference generate_video_visualizations, l4p/utils/vis.py:34-104, with colormap_image vis.py:227-282,
// the colour-wheel flow vis.py:288-428 and visualize_2d_tracks / plot_2d_tracks vis.py:434-523): RGB, turbo depth, colour-wheel
// flow, thresholded motion mask and track trails over the grey video, side by side in one [T][H][P W][3] tensor.  The reference
// does the dense panels in per-frame numpy loops and the tracks in ~T x 16 x N cv2 calls; here it is four kernels:
//   vis_stats_kernel    one pass over depth and flow: min / max of the positive depths, max of u^2 + v^2          (HBM-bound)
//   vis_panels_kernel   one pass over rgb, depth, flow, mask: every dense panel and the track panel's background  (HBM-bound)
//   vis_track_prep      (after the shared argsort) the display list: integer points, visibility, colours           (latency)
//   vis_raster_kernel   trails and end points composited per 16 x 16 tile with the reference's ordering            (LDS / VALU)
// Compiled with -ffp-contract=off (Makefile): f32 expressions round operation by operation as ATen's and numpy's do, f64 where
// the reference computes in Python floats or numpy float64 (the flow panel after its clip, NumPy 2 promotion rules).
#include "common.hpp"
#include "prof.hpp"
#include "stable_argsort.hpp"

// -------------------------------------------------------------------------------------------------
// Statistics (vis.py:60-63, 413-417), one launch.  stats[0] = max over positive depths of ~bits(d) (so that a zero-filled
// buffer is the identity and stats[0] == 0 says "no positive depth"), stats[1] = max of bits(d), stats[2] = max of
// bits(u * u + v * v): non-negative floats order as their bit patterns.  Per wave, per workgroup, then one vector atomic each.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void vis_stats_kernel(const float* __restrict__ depth, const float* __restrict__ flow, long long n,
                                                        unsigned* __restrict__ stats) {
    __shared__ unsigned red[3][4];
    unsigned a = 0, b = 0, c = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (depth) {
            const float d = depth[i];
            if (d > 0.f) {
                const unsigned k = __float_as_uint(d);
                a = ~k > a ? ~k : a;
                b = k > b ? k : b;
            }
        }
        if (flow) {
            const float u = flow[i], v = flow[n + i];
            const unsigned k = __float_as_uint(u * u + v * v);  // (a NaN's pattern is above every finite one: it wins, as in torch.max)
            c = k > c ? k : c;
        }
    }
    a = wave_umax(a);
    b = wave_umax(b);
    c = wave_umax(c);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wid] = a;
        red[1][wid] = b;
        red[2][wid] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned m = red[threadIdx.x][0];
        for (int w = 1; w < 4; ++w) m = red[threadIdx.x][w] > m ? red[threadIdx.x][w] : m;
        if (m) atomicMax(stats + threadIdx.x, m);
    }
}

// The scalars the reference forms in Python doubles from the statistics (every consumer thread forms them itself):
// depth_range = (max(min, 0.05), min(max, 20)) (vis.py:58-63), rad_max = min(25, sqrt(max(u^2 + v^2))) (vis.py:413-418).
struct VisScalars {
    double vmin, vmax, rad_max;
    float vminf, vmaxf, denf;  // torch holds a Python scalar operand of an f32 tensor op in f32 (vis.py:64, 272)
    double clip, rad_eps;      // rad_max / np.sqrt(2), rad_max + 1e-5 (vis.py:422, 399-401)
    bool has_depth;
};
__device__ __forceinline__ VisScalars vis_scalars(const unsigned* __restrict__ stats) {
    VisScalars s;
    const unsigned s0 = stats[0], s1 = stats[1], s2 = stats[2];
    s.has_depth = s0 != 0u;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double dmin = (double)__uint_as_float(~s0), dmax = (double)__uint_as_float(s1);
    s.vmin = s.has_depth ? (0.05 > dmin ? 0.05 : dmin) : nan;
    s.vmax = s.has_depth ? (20.0 < dmax ? 20.0 : dmax) : nan;
    s.vminf = (float)s.vmin;
    s.vmaxf = (float)s.vmax;
    s.denf = (float)((s.vmax - s.vmin) * 1.05);
    const double r = (double)sqrtf(__uint_as_float(s2));
    s.rad_max = r < 25.0 ? r : 25.0;  // min(25.0, r): 25.0 unless r is smaller (a NaN r keeps 25.0, as Python's min does)
    s.clip = s.rad_max / sqrt(2.0);
    s.rad_eps = s.rad_max + 1e-5;
    return s;
}

// the project's own byte rule of the uint8 video: min(255, max(0, x * 255 + 0.5)) truncated (f32, NaN -> 0)
__device__ __forceinline__ unsigned char vis_u8(float x) {
    const float v = fminf(255.f, fmaxf(0.f, x * 255.f + 0.5f));
    return (unsigned char)v;
}

template <int V, typename OutT> struct VisStore;
template <> struct VisStore<1, float> {
    static __device__ __forceinline__ void put(float* o, const float* v) {
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
    }
};
template <> struct VisStore<4, float> {  // 4 pixels = 48 bytes, 16-byte aligned when W % 4 == 0
    static __device__ __forceinline__ void put(float* o, const float* v) {
        f32x4* q = reinterpret_cast<f32x4*>(o);
        q[0] = (f32x4){v[0], v[1], v[2], v[3]};
        q[1] = (f32x4){v[4], v[5], v[6], v[7]};
        q[2] = (f32x4){v[8], v[9], v[10], v[11]};
    }
};
template <> struct VisStore<1, unsigned char> {
    static __device__ __forceinline__ void put(unsigned char* o, const float* v) {
        o[0] = vis_u8(v[0]);
        o[1] = vis_u8(v[1]);
        o[2] = vis_u8(v[2]);
    }
};
template <> struct VisStore<4, unsigned char> {  // 12 bytes, 4-byte aligned when W % 4 == 0
    static __device__ __forceinline__ void put(unsigned char* o, const float* v) {
        unsigned* q = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (unsigned)vis_u8(v[4 * k]) | ((unsigned)vis_u8(v[4 * k + 1]) << 8) | ((unsigned)vis_u8(v[4 * k + 2]) << 16) |
                   ((unsigned)vis_u8(v[4 * k + 3]) << 24);
    }
};

template <int V> __device__ __forceinline__ void vis_load(const float* p, float* v);
template <> __device__ __forceinline__ void vis_load<1>(const float* p, float* v) { v[0] = p[0]; }
template <> __device__ __forceinline__ void vis_load<4>(const float* p, float* v) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0];
    v[1] = q[1];
    v[2] = q[2];
    v[3] = q[3];
}

struct VisPanelArgs {
    const float *rgb, *mean, *stdv, *depth, *flow, *mask;  // [3][T][H][W], [3], [3], [T][H][W], [2][T][H][W], [T][H][W]
    const unsigned* stats;
    const float* turbo;    // [256][3], already flipped (colormap_image flip=True)
    const double* wheel;   // [55][3] = make_colorwheel() / 255.0
    int T, H, W, P;        // P panels per row
    int p_depth, p_flow, p_mask, p_track;  // panel slot of each task, -1 = absent; rgb is slot 0
    void* out;             // [T][H][P W][3] float or uchar
    float* grey;           // uchar output only: [T][H][W] f32 background of the track panel for the raster kernel
    double* scalars;       // [3]: depth_range (2), flow_rad_max
};

// -------------------------------------------------------------------------------------------------
// The fused panel kernel: V pixels of one row per thread (V = 4 when W % 4 == 0: 16-byte loads and stores), grid-stride.
// -------------------------------------------------------------------------------------------------
template <int V, typename OutT> __global__ __launch_bounds__(256) void vis_panels_kernel(VisPanelArgs a) {
    __shared__ float turbo[256 * 3];
    __shared__ double wheel[55 * 3];
    if (a.p_depth >= 0)
        for (int k = threadIdx.x; k < 768; k += 256) turbo[k] = a.turbo[k];
    if (a.p_flow >= 0)
        for (int k = threadIdx.x; k < 165; k += 256) wheel[k] = a.wheel[k];
    __syncthreads();
    const VisScalars sc = vis_scalars(a.stats);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.scalars[0] = sc.vmin;
        a.scalars[1] = sc.vmax;
        a.scalars[2] = sc.rad_max;
    }
    const float m0 = a.mean[0], m1 = a.mean[1], m2 = a.mean[2], s0 = a.stdv[0], s1 = a.stdv[1], s2 = a.stdv[2];
    const int Wv = a.W / V;
    const long long thw = (long long)a.T * a.H * a.W, items = thw / V, row = (long long)a.P * a.W * 3;
    OutT* out = reinterpret_cast<OutT*>(a.out);
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
        const long long q = it * V;                       // (t * H + y) * W + x
        const long long line = it / Wv;                   // t * H + y
        const int x = (int)(it - line * Wv) * V;
        OutT* o = out + line * row + (long long)x * 3;
        float r[V], g[V], b[V], v[V * 3];
        vis_load<V>(a.rgb + q, r);
        vis_load<V>(a.rgb + thw + q, g);
        vis_load<V>(a.rgb + 2 * thw + q, b);
#pragma unroll
        for (int k = 0; k < V; ++k) {  // vis.py:48
            r[k] = r[k] * s0 + m0;
            g[k] = g[k] * s1 + m1;
            b[k] = b[k] * s2 + m2;
            v[3 * k] = r[k];
            v[3 * k + 1] = g[k];
            v[3 * k + 2] = b[k];
        }
        VisStore<V, OutT>::put(o, v);
        if (a.p_depth >= 0) {  // vis.py:64-65, 272-275
            float d[V];
            vis_load<V>(a.depth + q, d);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float dc = fminf(fmaxf(d[k], sc.vminf), sc.vmaxf);
                float xn = (dc - sc.vminf) / sc.denf * 255.f;
                xn = fminf(fmaxf(xn, 0.f), 255.f);  // (NaN, e.g. a zero range, -> entry 0)
                const int idx = (int)xn;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * k + c] = sc.has_depth ? turbo[idx * 3 + c] : 0.f;
            }
            VisStore<V, OutT>::put(o + (long long)a.p_depth * a.W * 3, v);
        }
        if (a.p_flow >= 0) {  // vis.py:393-402, 356-373, 426
            float fu[V], fv[V];
            vis_load<V>(a.flow + q, fu);
            vis_load<V>(a.flow + thw + q, fv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                double u = (double)fu[k], w = (double)fv[k];
                u = u < -sc.clip ? -sc.clip : (u > sc.clip ? sc.clip : u);
                w = w < -sc.clip ? -sc.clip : (w > sc.clip ? sc.clip : w);
                u = u / sc.rad_eps;
                w = w / sc.rad_eps;
                const double rad = sqrt(u * u + w * w);
                const double ang = atan2(-w, -u) / 3.141592653589793;
                const double fk = (ang + 1.0) / 2.0 * 54.0;
                const double fl = floor(fk);
                int k0 = (int)fl;
                int k1 = k0 + 1;
                if (k1 == 55) k1 = 0;
                const double f = fk - fl;
                k0 = k0 < 0 ? k0 + 55 : k0;  // numpy's negative index: -1 is the last entry
                k1 = k1 < 0 ? k1 + 55 : k1;
                k0 = k0 < 0 ? 0 : (k0 > 54 ? 54 : k0);  // (non-finite flow: the reference raises; stay inside the table)
                k1 = k1 < 0 ? 0 : (k1 > 54 ? 54 : k1);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double col = (1.0 - f) * wheel[k0 * 3 + c] + f * wheel[k1 * 3 + c];
                    col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
                    const double lv = floor(255.0 * col);
                    v[3 * k + c] = (float)(unsigned char)(int)(lv < 0.0 ? 0.0 : (lv > 255.0 ? 255.0 : lv)) / 255.f;
                }
            }
            VisStore<V, OutT>::put(o + (long long)a.p_flow * a.W * 3, v);
        }
        if (a.p_mask >= 0) {  // vis.py:81-86
            float m[V];
            vis_load<V>(a.mask + q, m);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float bit = 1.f / (1.f + expf(-m[k])) > 0.85f ? 1.f : 0.f;
                v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = bit;
            }
            VisStore<V, OutT>::put(o + (long long)a.p_mask * a.W * 3, v);
        }
        if (a.p_track >= 0) {  // vis.py:465: torch.mean over the three channels, (r + g + b) / 3
            float gr[V];
#pragma unroll
            for (int k = 0; k < V; ++k) gr[k] = ((r[k] + g[k]) + b[k]) / 3.f;
            if (a.grey) {  // uchar video: the raster kernel composites in f32 from this plane and writes the bytes
                if constexpr (V == 4) *reinterpret_cast<f32x4*>(a.grey + q) = (f32x4){gr[0], gr[1], gr[2], gr[3]};
                else a.grey[q] = gr[0];
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = gr[k];
                VisStore<V, OutT>::put(o + (long long)a.p_track * a.W * 3, v);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Display list of the track panel (vis.py:454-466, 479-483, 500-502), one thread per (frame t, rank i): track order[i];
// xy [T][N][2] = the estimated position rounded half to even (int(round(np.float32))), clamped to +-2^30; vis [T][N] =
// sigmoid(logit) > thr and both coordinates finite (the reference raises on a non-finite one; here the primitive is skipped);
// colors [N][3] = hsv(Normalize(0, N - 1)(i)) as recon4d's trails form the index, the float64 table entry rounded to f32.
// traj [N][2][T], logit [N][T], hsv [256][3] double.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vis_track_prep_kernel(const float* __restrict__ traj, const float* __restrict__ logit,
                                                             const int* __restrict__ order, const double* __restrict__ hsv, int N,
                                                             int T, float thr, int* __restrict__ xy,
                                                             unsigned char* __restrict__ vis, float* __restrict__ colors) {
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= (long long)T * N) return;
    const int t = (int)(idx / N), i = (int)(idx % N);
    const long long n = order[i];
    const float x = traj[(n * 2 + 0) * T + t], y = traj[(n * 2 + 1) * T + t];
    const bool finite = fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f;
    const float lim = 1073741824.f;
    xy[idx * 2 + 0] = finite ? (int)fminf(fmaxf(rintf(x), -lim), lim) : 0;
    xy[idx * 2 + 1] = finite ? (int)fminf(fmaxf(rintf(y), -lim), lim) : 0;
    vis[idx] = (finite && 1.f / (1.f + expf(-logit[n * T + t])) > thr) ? 1 : 0;
    if (t == 0) {
        double f = N > 1 ? (double)i / (double)(N - 1) : 0.0;
        f *= 256.0;
        const int ci = f >= 256.0 ? 255 : (int)f;
        for (int c = 0; c < 3; ++c) colors[i * 3 + c] = (float)hsv[ci * 3 + c];
    }
}

// -------------------------------------------------------------------------------------------------
// Track raster (plot_2d_tracks, vis.py:489-521, with the project's own coverage rules in place of cv2's anti-aliasing): one
// workgroup per 16 x 16 tile and frame, one thread per pixel, the pixel in registers from its one read to its one write.
// Frame t, t0 = max(0, t - trail), L = t - t0 + 1: for s = 0 .. L - 2: G = F; every track in ascending rank whose points t0 + s
// and t0 + s + 1 are both visible paints its segment: c = clamp(1 - d, 0, 1) with d the distance from the pixel centre to the
// segment, F = (1 - c) F + c colour where c > 0; then F = wa F + wb G, wa = f32(alpha), wb = f32(1 - alpha), alpha = (s + 1) /
// (L - 1) in double.  Then every visible track in ascending rank overwrites the pixels with dx^2 + dy^2 <= 5 around its point
// of frame t.  Per step the tracks are walked in chunks of 256: each thread tests one track's primitive (bounding box grown by
// one against the tile), the survivors are compacted in rank order into LDS (ballot, prefix count, per-wave offsets) and
// every pixel walks that list.  A pixel outside a segment's grown bounding box is at distance >= 2: skipping it changes nothing.
// src: the grey background, pixel (t, y, x) at src[t * s_frame + y * s_row + x * s_px]; out pixel at out[t * o_frame + y * o_row +
// x * 3 + c] (src may alias out: each pixel is read and written by its own thread only).
// -------------------------------------------------------------------------------------------------
template <typename OutT> __device__ __forceinline__ OutT vis_out(float v);
template <> __device__ __forceinline__ float vis_out<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned char vis_out<unsigned char>(float v) { return vis_u8(v); }

template <typename OutT>
__global__ __launch_bounds__(256) void vis_raster_kernel(const int* __restrict__ xy, const unsigned char* __restrict__ vis,
                                                         const float* __restrict__ colors, int N, int T, int H, int W, int trail,
                                                         const float* src, long long s_px, long long s_row, long long s_frame,
                                                         OutT* out, long long o_row, long long o_frame) {
    __shared__ int seg[256][5];  // x1, y1, x2, y2, rank
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16, t = blockIdx.z;
    const int px = x0 + (tid & 15), py = y0 + (tid >> 4);
    const bool inside = px < W && py < H;
    float F0 = 0.f, F1, F2;
    if (inside) F0 = src[(long long)t * s_frame + (long long)py * s_row + (long long)px * s_px];
    F1 = F2 = F0;
    const int t0 = t - trail > 0 ? t - trail : 0, L = t - t0 + 1;
    for (int s = 0; s <= L - 2; ++s) {
        const float G0 = F0, G1 = F1, G2 = F2;
        const long long ra = (long long)(t0 + s) * N, rb = ra + N;
        for (int i0 = 0; i0 < N; i0 += 256) {
            const int i = i0 + tid;
            bool keep = false;
            int ax = 0, ay = 0, bx = 0, by = 0;
            if (i < N && vis[ra + i] && vis[rb + i]) {
                ax = xy[(ra + i) * 2];
                ay = xy[(ra + i) * 2 + 1];
                bx = xy[(rb + i) * 2];
                by = xy[(rb + i) * 2 + 1];
                const int lox = (ax < bx ? ax : bx) - 1, hix = (ax < bx ? bx : ax) + 1;
                const int loy = (ay < by ? ay : by) - 1, hiy = (ay < by ? by : ay) + 1;
                keep = hix >= x0 && lox <= x0 + 15 && hiy >= y0 && loy <= y0 + 15;
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wtot[wid] = __popcll(m);
            __syncthreads();
            int before = 0;
            for (int w = 0; w < wid; ++w) before += wtot[w];
            const int cnt = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            if (keep) {
                int* e = seg[before + __popcll(m & ((1ull << lane) - 1ull))];
                e[0] = ax;
                e[1] = ay;
                e[2] = bx;
                e[3] = by;
                e[4] = i;
            }
            __syncthreads();
            if (inside)
                for (int k = 0; k < cnt; ++k) {
                    const int x1 = seg[k][0], y1 = seg[k][1], x2 = seg[k][2], y2 = seg[k][3];
                    if (px < (x1 < x2 ? x1 : x2) - 1 || px > (x1 < x2 ? x2 : x1) + 1 || py < (y1 < y2 ? y1 : y2) - 1 ||
                        py > (y1 < y2 ? y2 : y1) + 1)
                        continue;
                    const float dx = (float)(x2 - x1), dy = (float)(y2 - y1), qx = (float)(px - x1), qy = (float)(py - y1);
                    const float len2 = dx * dx + dy * dy;
                    float u = 0.f;
                    if (len2 != 0.f) u = fminf(fmaxf((qx * dx + qy * dy) / len2, 0.f), 1.f);
                    const float ex = qx - u * dx, ey = qy - u * dy;
                    const float c = fminf(fmaxf(1.f - sqrtf(ex * ex + ey * ey), 0.f), 1.f);
                    if (c > 0.f) {
                        const float* col = colors + seg[k][4] * 3;
                        const float ic = 1.f - c;
                        F0 = ic * F0 + c * col[0];
                        F1 = ic * F1 + c * col[1];
                        F2 = ic * F2 + c * col[2];
                    }
                }
            __syncthreads();
        }
        const double alpha = (double)(s + 1) / (double)(L - 1);
        const float wa = (float)alpha, wb = (float)(1.0 - alpha);
        F0 = wa * F0 + wb * G0;
        F1 = wa * F1 + wb * G1;
        F2 = wa * F2 + wb * G2;
    }
    const long long rt = (long long)t * N;
    for (int i0 = 0; i0 < N; i0 += 256) {  // end points (vis.py:513-516)
        const int i = i0 + tid;
        bool keep = false;
        int ax = 0, ay = 0;
        if (i < N && vis[rt + i]) {
            ax = xy[(rt + i) * 2];
            ay = xy[(rt + i) * 2 + 1];
            keep = ax + 2 >= x0 && ax - 2 <= x0 + 15 && ay + 2 >= y0 && ay - 2 <= y0 + 15;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wtot[wid] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wid; ++w) before += wtot[w];
        const int cnt = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        if (keep) {
            int* e = seg[before + __popcll(m & ((1ull << lane) - 1ull))];
            e[0] = ax;
            e[1] = ay;
            e[4] = i;
        }
        __syncthreads();
        if (inside)
            for (int k = 0; k < cnt; ++k) {
                const int dx = px - seg[k][0], dy = py - seg[k][1];
                if (dx < -2 || dx > 2 || dy < -2 || dy > 2) continue;
                if (dx * dx + dy * dy <= 5) {
                    const float* col = colors + seg[k][4] * 3;
                    F0 = col[0];
                    F1 = col[1];
                    F2 = col[2];
                }
            }
        __syncthreads();
    }
    if (inside) {
        OutT* o = out + (long long)t * o_frame + (long long)py * o_row + (long long)px * 3;
        o[0] = vis_out<OutT>(F0);
        o[1] = vis_out<OutT>(F1);
        o[2] = vis_out<OutT>(F2);
    }
}

extern "C" {

int l4p_vis_stats(l4p_stream s_, const float* depth, const float* flow, long long n, unsigned* stats) {
    hipStream_t s = (hipStream_t)s_;
    if (n < 1 || !stats) {
        l4p_set_error("l4p_vis_stats: need n >= 1 and stats (n=%lld)", n);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_vis_stats");
    HIP_TRY(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned), s));
    if (!depth && !flow) return 0;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(vis_stats_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, depth, flow, n, stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_vis_panels(l4p_stream s_, const float* rgb, const float* mean, const float* stdv, const float* depth, const float* flow,
                   const float* mask, const unsigned* stats, const float* turbo, const double* wheel, int T, int H, int W, int P,
                   int p_depth, int p_flow, int p_mask, int p_track, void* out, int out_u8, float* grey, double* scalars) {
    hipStream_t s = (hipStream_t)s_;
    const int slots[4] = {p_depth, p_flow, p_mask, p_track};
    const void* need[4] = {depth, flow, mask, rgb};
    bool ok = T >= 1 && H >= 1 && W >= 1 && P >= 1 && P <= 5 && rgb && mean && stdv && stats && out && scalars &&
              (long long)T * H * W * P * 3 <= 0x7FFFFFFFFFFFll && (p_depth < 0 || turbo) && (p_flow < 0 || wheel) &&
              (!out_u8 || p_track < 0 || grey);
    unsigned used = 1u;  // slot 0 is the rgb panel
    for (int k = 0; k < 4 && ok; ++k) {
        if (slots[k] < 0) continue;
        ok = slots[k] >= 1 && slots[k] < P && !(used & (1u << slots[k])) && need[k];
        used |= 1u << slots[k];
    }
    if (ok) ok = used == (1u << P) - 1u;  // every panel of the row is written
    if (!ok) {
        l4p_set_error("l4p_vis_panels: bad arguments (T=%d H=%d W=%d P=%d slots depth=%d flow=%d mask=%d track=%d): P <= 5 panels, "
                      "each task's slot distinct in [1, P) with its input, tables for depth / flow, grey for a uchar track panel",
                      T, H, W, P, p_depth, p_flow, p_mask, p_track);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_vis_panels");
    VisPanelArgs a = {rgb, mean, stdv, depth, flow, mask, stats, turbo, wheel, T, H, W, P, p_depth, p_flow, p_mask, p_track,
                      out, out_u8 ? grey : nullptr, scalars};
    const int V = W % 4 == 0 ? 4 : 1;
    const long long items = (long long)T * H * W / V, blocks = (items + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(256);
    if (V == 4 && out_u8) hipLaunchKernelGGL((vis_panels_kernel<4, unsigned char>), grid, block, 0, s, a);
    else if (V == 4) hipLaunchKernelGGL((vis_panels_kernel<4, float>), grid, block, 0, s, a);
    else if (out_u8) hipLaunchKernelGGL((vis_panels_kernel<1, unsigned char>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((vis_panels_kernel<1, float>), grid, block, 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_vis_track_prep(l4p_stream s_, const float* key_traj, const float* traj, const float* vis_logit, const double* hsv, int N,
                       int T, float vis_thr, int* order, int* xy, unsigned char* vis, float* colors) {
    hipStream_t s = (hipStream_t)s_;
    if (N < 1 || T < 1 || (long long)N * T > 0x3FFFFFFFll || !key_traj || !traj || !vis_logit || !hsv || !order || !xy || !vis ||
        !colors) {
        l4p_set_error("l4p_vis_track_prep: need N, T >= 1, N T < 2^30 and every pointer (N=%d T=%d)", N, T);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_vis_track_prep");
    hipLaunchKernelGGL(recon_argsort_kernel, dim3((N + 3) / 4), dim3(256), 0, s, key_traj, N, T, order);
    const long long n = (long long)N * T;
    hipLaunchKernelGGL(vis_track_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, traj, vis_logit, order, hsv, N, T,
                       vis_thr, xy, vis, colors);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_vis_track_raster(l4p_stream s_, const int* xy, const unsigned char* vis, const float* colors, int N, int T, int H, int W,
                         int trail, const float* src, long long s_px, long long s_row, long long s_frame, void* out,
                         long long o_row, long long o_frame, int out_u8) {
    hipStream_t s = (hipStream_t)s_;
    if (N < 0 || T < 1 || T > 65535 || H < 1 || W < 1 || (H + 15) / 16 > 65535 || trail < 0 || !src || !out ||
        (N > 0 && (!xy || !vis || !colors)) || s_px < 1 || s_row < (long long)W * s_px || s_frame < (long long)H * s_row ||
        o_row < (long long)W * 3 || o_frame < (long long)H * o_row) {
        l4p_set_error("l4p_vis_track_raster: bad arguments (N=%d T=%d H=%d W=%d trail=%d strides %lld %lld %lld / %lld %lld)", N, T, H,
                      W, trail, s_px, s_row, s_frame, o_row, o_frame);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_vis_track_raster");
    const dim3 grid((W + 15) / 16, (H + 15) / 16, T), block(256);
    if (out_u8)
        hipLaunchKernelGGL((vis_raster_kernel<unsigned char>), grid, block, 0, s, xy, vis, colors, N, T, H, W, trail, src, s_px, s_row,
                           s_frame, (unsigned char*)out, o_row, o_frame);
    else
        hipLaunchKernelGGL((vis_raster_kernel<float>), grid, block, 0, s, xy, vis, colors, N, T, H, W, trail, src, s_px, s_row, s_frame,
                           (float*)out, o_row, o_frame);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
