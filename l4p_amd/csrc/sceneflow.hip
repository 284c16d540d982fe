// Dense scene flow and camera-compensated flow from depth, backward optical flow and camera poses (DESIGN.md "Scene flow").
// For frame t >= 1 and pixel p = (i, j): X_t = P_t [D_t(p) K_t^-1 (i, j, 1); 1]; the flow sends p to q = p + F_t(p) in frame t - 1,
// whose depth is sampled bilinearly there, X' = P_{t-1} [d' K_{t-1}^-1 (q, 1); 1]; scene flow S = X' - X_t (world frame, backward
// in time); rigid flow R = proj_{t-1}(P_{t-1}^-1 X_t) - p, the flow a static point would show; compensated flow C = F - R.
// One memory-bound pass: 12 B read, one four-tap gather of the previous depth plane and 29 B written per pixel.  All per-pixel
// arithmetic is f32 and the file is compiled with -ffp-contract=off (Makefile): every operation rounds on its own, which is what
// lets the tests hold `valid` and the summary exactly.  The matrix inverses are formed in double once per block and rounded once.
// Matrix layout: b44t, element (i, j) of frame t at [(i * 4 + j) * T + t].
#include "common.hpp"
#include "prof.hpp"

// general 3x3 inverse by cofactors, double; a, o row-major [9]
__device__ void sf_inv3_d(const double* a, double* o) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double id = 1.0 / (a[0] * c00 + a[1] * c01 + a[2] * c02);
    o[0] = c00 * id, o[1] = (a[2] * a[7] - a[1] * a[8]) * id, o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    o[3] = c01 * id, o[4] = (a[0] * a[8] - a[2] * a[6]) * id, o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    o[6] = c02 * id, o[7] = (a[1] * a[6] - a[0] * a[7]) * id, o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// upper-left 3x3 of the b44t matrix m (frame stride T) inverted in double, rounded to f32: o row-major [9]
__device__ void sf_kinv(const float* __restrict__ m, int T, float* o) {
    double a[9], r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i * 3 + j] = (double)m[(long long)(i * 4 + j) * T];
    sf_inv3_d(a, r);
    for (int k = 0; k < 9; ++k) o[k] = (float)r[k];
}

// affine inverse [A | b]^-1 = [A^-1 | -A^-1 b] of the b44t matrix m in double, rounded to f32: o row-major 3x4 [12]
__device__ void sf_pinv(const float* __restrict__ m, int T, float* o) {
    double a[9], r[9], b[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) a[i * 3 + j] = (double)m[(long long)(i * 4 + j) * T];
        b[i] = (double)m[(long long)(i * 4 + 3) * T];
    }
    sf_inv3_d(a, r);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = (float)r[i * 3 + j];
        o[i * 4 + 3] = (float)(-(r[i * 3] * b[0] + r[i * 3 + 1] * b[1] + r[i * 3 + 2] * b[2]));
    }
}

// the first n row-major entries of the b44t matrix m (n = 12: rows 0..2 as a 3x4)
__device__ void sf_rows(const float* __restrict__ m, int T, int n, float* o) {
    for (int k = 0; k < n; ++k) o[k] = m[(long long)k * T];
}

// a 3x4 row-major affine map applied to (x, y, z, 1), left to right
__device__ __forceinline__ void sf_affine(const float* m, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = m[0] * x + m[1] * y + m[2] * z + m[3];
    oy = m[4] * x + m[5] * y + m[6] * z + m[7];
    oz = m[8] * x + m[9] * y + m[10] * z + m[11];
}

// a 3x3 row-major matrix applied to (x, y, 1), then scaled by d: the camera-frame point of a pixel
__device__ __forceinline__ void sf_ray(const float* m, float x, float y, float d, float& ox, float& oy, float& oz) {
    ox = (m[0] * x + m[1] * y + m[2]) * d;
    oy = (m[3] * x + m[4] * y + m[5]) * d;
    oz = (m[6] * x + m[7] * y + m[8]) * d;
}

__device__ __forceinline__ bool sf_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// the six matrices of a frame pair (t, t - 1): K_t^-1, K_{t-1}^-1 (3x3), rows 0..1 of K_{t-1}, rows 0..2 of P_t, P_{t-1}, P_{t-1}^-1
struct SfPair {
    float kinv_t[9], kinv_p[9], k_p[8], p_t[12], p_p[12], pinv_p[12];
};

// one pixel (i, j) of frame t: depth d, flow (fx, fy), dprev = depth plane t - 1.  o = scene xyz, rigid xy, comp xy; returns valid.
__device__ __forceinline__ bool sf_pixel(const SfPair& m, const float* __restrict__ dprev, int H, int W, int i, int j, float d, float fx,
                                         float fy, float* o) {
    const float fi = (float)i, fj = (float)j;
    float cx, cy, cz, X, Y, Z;
    sf_ray(m.kinv_t, fi, fj, d, cx, cy, cz);
    sf_affine(m.p_t, cx, cy, cz, X, Y, Z);
    const float qx = fi + fx, qy = fj + fy;
    const bool inside = qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1);  // NaN fails
    float sx = 0.f, sy = 0.f, sz = 0.f, dp = 0.f;
    if (inside) {  // only then are the taps inside the plane
        const float flx = floorf(qx), fly = floorf(qy);
        const int x0 = (int)flx, y0 = (int)fly;
        const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
        const float ax = qx - flx, ay = qy - fly;
        const float v00 = dprev[y0 * W + x0], v01 = dprev[y0 * W + x1], v10 = dprev[y1 * W + x0], v11 = dprev[y1 * W + x1];
        const float w00 = (1.f - ay) * (1.f - ax), w01 = (1.f - ay) * ax, w10 = ay * (1.f - ax), w11 = ay * ax;
        dp = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
        float ex, ey, ez, X1, Y1, Z1;
        sf_ray(m.kinv_p, qx, qy, dp, ex, ey, ez);
        sf_affine(m.p_p, ex, ey, ez, X1, Y1, Z1);
        sx = X1 - X, sy = Y1 - Y, sz = Z1 - Z;
    }
    float ux, uy, uz;  // the point, assumed static, in camera t - 1
    sf_affine(m.pinv_p, X, Y, Z, ux, uy, uz);
    const bool front = uz > 1e-6f;
    float rx = 0.f, ry = 0.f;
    if (front) {
        rx = (m.k_p[0] * ux + m.k_p[1] * uy + m.k_p[2] * uz) / uz - fi;
        ry = (m.k_p[4] * ux + m.k_p[5] * uy + m.k_p[6] * uz) / uz - fj;
    }
    const float gx = fx - rx, gy = fy - ry;
    const bool ok = inside && d > 0.f && dp > 0.f && front && sf_finite(sx) && sf_finite(sy) && sf_finite(sz) && sf_finite(rx) &&
                    sf_finite(ry) && sf_finite(gx) && sf_finite(gy);
    o[0] = ok ? sx : 0.f, o[1] = ok ? sy : 0.f, o[2] = ok ? sz : 0.f;
    o[3] = ok ? rx : 0.f, o[4] = ok ? ry : 0.f, o[5] = ok ? gx : 0.f, o[6] = ok ? gy : 0.f;
    return ok;
}

// -------------------------------------------------------------------------------------------------
// Fields.  Block = (frame (b, t), slice of its pixels); one pixel per thread, block-stride over the slice (the pixel's row and
// column advance by the stride's row and column parts: one integer division per thread, none per pixel).  The six matrices of the
// frame pair are formed by lane 0 of one wave each (the three inverses in double) and handed over through LDS.  depth
// [B][T][HW], flow [B][2][T][HW], K, P [B][16][T]; scene [B][3][T][HW], rigid / comp [B][2][T][HW], valid [B][T][HW] uchar: every
// store is channel-planar and coalesced; the only gather is the four taps of depth plane t - 1, read only when q lies inside the
// image.  Frame 0 is zeroed and reads nothing.
// (Measured and not kept: four pixels per thread with 16-byte accesses, and the matrices in scalar registers: the same time.)
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_flow_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                         const float* __restrict__ P, const float* __restrict__ K, int T, int H, int W,
                                                         int bpf, float* __restrict__ scene, float* __restrict__ rigid,
                                                         float* __restrict__ comp, unsigned char* __restrict__ valid) {
    __shared__ SfPair lds;
    const int bt = blockIdx.x / bpf, slice = blockIdx.x - bt * bpf;
    const int b = bt / T, t = bt - b * T;
    const int HW = H * W;
    const long long thw = (long long)T * HW;
    const long long plane = ((long long)b * T + t) * HW;   // depth / valid plane of (b, t)
    const long long c0 = ((long long)b * 2 * T + t) * HW;  // channel 0 of a [B][2][T][HW] tensor
    const long long s0 = ((long long)b * 3 * T + t) * HW;  // channel 0 of a [B][3][T][HW] tensor
    const int first = slice * 256 + (int)threadIdx.x, step = bpf * 256;
    if (t == 0) {  // no predecessor: nothing of frame -1 is read
        for (int pix = first; pix < HW; pix += step) {
            scene[s0 + pix] = 0.f, scene[s0 + thw + pix] = 0.f, scene[s0 + 2 * thw + pix] = 0.f;
            rigid[c0 + pix] = 0.f, rigid[c0 + thw + pix] = 0.f;
            comp[c0 + pix] = 0.f, comp[c0 + thw + pix] = 0.f;
            valid[plane + pix] = 0;
        }
        return;
    }
    if ((threadIdx.x & 63) == 0) {
        const float* kt = K + (long long)b * 16 * T + t;
        const float* pt = P + (long long)b * 16 * T + t;
        const int w = threadIdx.x >> 6;
        if (w == 0) {
            sf_kinv(kt, T, lds.kinv_t);
        } else if (w == 1) {
            sf_kinv(kt - 1, T, lds.kinv_p);
        } else if (w == 2) {
            sf_pinv(pt - 1, T, lds.pinv_p);
        } else {
            sf_rows(pt, T, 12, lds.p_t);
            sf_rows(pt - 1, T, 12, lds.p_p);
            sf_rows(kt - 1, T, 8, lds.k_p);
        }
    }
    __syncthreads();
    const SfPair m = lds;
    const float* dprev = depth + plane - HW;
    const int dj = step / W, di = step - dj * W;
    int j = first / W, i = first - j * W;
    for (int pix = first; pix < HW; pix += step) {
        float o[7];
        const bool ok = sf_pixel(m, dprev, H, W, i, j, depth[plane + pix], flow[c0 + pix], flow[c0 + thw + pix], o);
        scene[s0 + pix] = o[0], scene[s0 + thw + pix] = o[1], scene[s0 + 2 * thw + pix] = o[2];
        rigid[c0 + pix] = o[3], rigid[c0 + thw + pix] = o[4];
        comp[c0 + pix] = o[5], comp[c0 + thw + pix] = o[6];
        valid[plane + pix] = ok ? 1 : 0;
        i += di, j += dj;
        if (i >= W) i -= W, ++j;
    }
}

// -------------------------------------------------------------------------------------------------
// Summary, pass 1: block (chunk c of L4P_SCENE_FLOW_CHUNK pixels, frame bt) -> ws[(bt * nchunk + c) * 8 + k].  Each thread adds its
// pixels in index order, lanes are folded by a fixed shuffle tree, the four waves in wave order: no atomics, the same bits every run.
// Magnitudes are f32 (sqrtf of the unfused sum of squares of the stored values), accumulated in double.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_flow_partial_kernel(const float* __restrict__ scene, const float* __restrict__ comp,
                                                                 const unsigned char* __restrict__ valid,
                                                                 const float* __restrict__ mask, int T, int HW, int nchunk, float tau,
                                                                 double* __restrict__ ws) {
    __shared__ double part[4][8];
    const int bt = blockIdx.y, c = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const long long thw = (long long)T * HW;
    const long long plane = (long long)bt * HW, c0 = ((long long)b * 2 * T + t) * HW, s0 = ((long long)b * 3 * T + t) * HW;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int end = (c + 1) * L4P_SCENE_FLOW_CHUNK < HW ? (c + 1) * L4P_SCENE_FLOW_CHUNK : HW;
    for (int pix = c * L4P_SCENE_FLOW_CHUNK + threadIdx.x; pix < end; pix += 256) {
        if (!valid[plane + pix]) continue;
        const float gx = comp[c0 + pix], gy = comp[c0 + thw + pix];
        const float sx = scene[s0 + pix], sy = scene[s0 + thw + pix], sz = scene[s0 + 2 * thw + pix];
        const float mc = sqrtf(gx * gx + gy * gy), ms = sqrtf(sx * sx + sy * sy + sz * sz);
        const float m = mask ? mask[plane + pix] : 0.f;
        a[0] += 1.0;
        if (m <= 0.f) {
            a[1] += 1.0;
            a[3] += (double)mc;
            a[5] += (double)ms;
        }
        if (m > 0.f) {
            a[2] += 1.0;
            a[4] += (double)mc;
            a[6] += (double)ms;
        }
        if (mc > tau) a[7] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8)
        ws[((long long)bt * nchunk + c) * 8 + threadIdx.x] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// pass 2: rows[bt][k] = the chunks' partials added in chunk order
__global__ void scene_flow_rows_kernel(const double* __restrict__ ws, int BT, int nchunk, double* __restrict__ rows) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= BT * 8) return;
    const int bt = idx >> 3, k = idx & 7;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += ws[((long long)bt * nchunk + c) * 8 + k];
    rows[idx] = acc;
}

// -------------------------------------------------------------------------------------------------
// Motion colours: a valid pixel takes lut[floor(255 min(1, |S| / s_max))] (f32 throughout, |S| as in the summary), an invalid one
// mid-grey.  colors [B][T * HW][3] uchar, frame-major as the 4D reconstruction's.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_flow_colors_kernel(const float* __restrict__ scene, const unsigned char* __restrict__ valid,
                                                                const unsigned char* __restrict__ lut, long long n, long long thw,
                                                                const float* __restrict__ s_max, unsigned char* __restrict__ colors) {
    const float smax = s_max[0];
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / thw, q = idx - b * thw;
        unsigned char c0 = 128, c1 = 128, c2 = 128;
        if (valid[idx]) {
            const float* s = scene + b * 3 * thw + q;
            const float sx = s[0], sy = s[thw], sz = s[2 * thw];
            const float r = sqrtf(sx * sx + sy * sy + sz * sz) / smax;
            int k = (int)floorf(255.f * (r < 1.f ? r : 1.f));  // a NaN ratio (0 / 0) takes entry 255
            k = k < 0 ? 0 : (k > 255 ? 255 : k);
            c0 = lut[k * 3], c1 = lut[k * 3 + 1], c2 = lut[k * 3 + 2];
        }
        unsigned char* o = colors + idx * 3;
        o[0] = c0, o[1] = c1, o[2] = c2;
    }
}

extern "C" {

int l4p_scene_flow(l4p_stream s_, const float* depth, const float* flow, const float* P, const float* K, const float* mask, int B,
                   int T, int H, int W, float* scene, float* rigid, float* comp, unsigned char* valid) {
    hipStream_t s = (hipStream_t)s_;
    (void)mask;  // the fields do not depend on the motion mask; it enters in l4p_scene_flow_summary
    const long long hw = (long long)H * W;
    if (B < 1 || T < 1 || H < 1 || W < 1 || hw > (1ll << 30) || !depth || !flow || !P || !K || !scene || !rigid || !comp || !valid) {
        l4p_set_error("l4p_scene_flow: need B, T, H, W >= 1, H W <= 2^30 and depth, flow, P, K, scene, rigid, comp, valid "
                      "(B=%d T=%d H=%d W=%d)", B, T, H, W);
        return L4P_E_INVALID;
    }
    // at most ~2048 blocks: each frame is shared by bpf blocks that stride over its `per` block-sized pieces in `rounds` rounds;
    // bpf is then the fewest blocks that need no more rounds, so that every block does the same work
    const long long frames = (long long)B * T, per = (hw + 255) / 256;
    long long bpf = 2048 / frames < 1 ? 1 : 2048 / frames;
    if (bpf > per) bpf = per;
    const long long rounds = (per + bpf - 1) / bpf;
    bpf = (per + rounds - 1) / rounds;
    if (frames * bpf > 0x7FFFFFFFll) {
        l4p_set_error("l4p_scene_flow: B T = %lld frames exceed the grid", frames);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_scene_flow");
    hipLaunchKernelGGL(scene_flow_kernel, dim3((unsigned)(frames * bpf)), dim3(256), 0, s, depth, flow, P, K, T, H, W, (int)bpf, scene,
                       rigid, comp, valid);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_scene_flow_summary(l4p_stream s_, const float* scene, const float* comp, const unsigned char* valid, const float* mask, int B,
                           int T, int H, int W, float tau_px, double* ws, double* rows) {
    hipStream_t s = (hipStream_t)s_;
    const long long hw = (long long)H * W, frames = (long long)B * T;
    if (B < 1 || T < 1 || H < 1 || W < 1 || hw > (1ll << 30) || frames > 65535 || !scene || !comp || !valid ||
        !ws || !rows) {
        l4p_set_error("l4p_scene_flow_summary: need B, T, H, W >= 1, H W <= 2^30, B T < 65536 and scene, comp, valid, ws, rows "
                      "(B=%d T=%d H=%d W=%d)", B, T, H, W);
        return L4P_E_INVALID;
    }
    const int nchunk = (int)((hw + L4P_SCENE_FLOW_CHUNK - 1) / L4P_SCENE_FLOW_CHUNK);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_scene_flow_summary");
    hipLaunchKernelGGL(scene_flow_partial_kernel, dim3(nchunk, (unsigned)frames), dim3(256), 0, s, scene, comp, valid, mask, T, (int)hw,
                       nchunk, tau_px, ws);
    hipLaunchKernelGGL(scene_flow_rows_kernel, dim3((unsigned)((frames * 8 + 255) / 256)), dim3(256), 0, s, ws, (int)frames, nchunk, rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_scene_flow_colors(l4p_stream s_, const float* scene, const unsigned char* valid, const unsigned char* lut, int B, int T, int H,
                          int W, const float* s_max, unsigned char* colors) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || T < 1 || H < 1 || W < 1 || !scene || !valid || !lut || !s_max || !colors) {
        l4p_set_error("l4p_scene_flow_colors: need B, T, H, W >= 1 and scene, valid, lut, s_max, colors (B=%d T=%d H=%d W=%d)", B, T, H, W);
        return L4P_E_INVALID;
    }
    const long long thw = (long long)T * H * W, n = (long long)B * thw;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_scene_flow_colors");
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(scene_flow_colors_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, scene, valid, lut, n,
                       thw, s_max, colors);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
