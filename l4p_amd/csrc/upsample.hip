// Guided (joint bilateral) up-sampling of the dense heads to the source video's resolution (DESIGN.md "Native-resolution results").
// A full-resolution pixel (X, Y) of the decoded frame lies at (x, y) of the network's low-resolution grid (the resize with half-pixel
// centres and the crop of prepare_clip, in f32, every operation rounded on its own: up_coord).  It takes the low-resolution values of
// the (2 radius + 1)^2 taps round (x, y), weighted by a spatial Gaussian and by a Gaussian of the colour distance between the decoded
// pixel and the tap's pixel of the network's input (Kopf et al. 2007), the latter floored so that a colour no tap has degrades to
// the spatial Gaussian.  The definition, operation by operation, is at l4p_guided_upsample in include/l4p_hip.h.
// The file is compiled with -ffp-contract=off (Makefile): coordinates, `inside` and the window centre are held bit for bit by the
// tests; the host forms the same coordinates with the same function to size the LDS footprint.  The weights and sums, which are
// held by tolerance, use fmaf where it is written.
#include "common.hpp"
#include "prof.hpp"

#include <algorithm>
#include <cmath>

constexpr int UP_TILE_W = 64;           // full-resolution columns of a tile: one wave per row, coalesced along X
constexpr int UP_TILE_H_MAX = 16;       // full-resolution rows of a tile: the largest of 16, 8, 4, 2, 1 whose footprint fits
constexpr int UP_LDS_BYTES = 48 * 1024; // what a launch may request (three workgroups per CU at the most)

// low-resolution coordinate of full-resolution index X along one axis: s = float(res) / float(src size), crop0 = float(crop offset)
__host__ __device__ __forceinline__ float up_coord(int X, float s, float crop0) { return ((float)X + 0.5f) * s - 0.5f - crop0; }

// window centre floor(x + 0.5) of a coordinate; x is first brought into [-2, n + 1] so that the conversion cannot overflow: that
// moves no pixel that is inside (-0.5 <= x < n - 0.5), and it is monotone, so a tile's first and last centre still bound all of them
__host__ __device__ __forceinline__ int up_centre(float x, int n) {
    const float hi = (float)n + 1.f;
    const float c = x < -2.f ? -2.f : (x > hi ? hi : x);
    return (int)floorf(c + 0.5f);
}

__device__ __forceinline__ bool up_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

struct UpParams {
    const unsigned char* guide_hi;
    const int* frame_index;
    const float* guide_lo;
    const float* src;
    float* out;
    unsigned char* valid;
    int C, T, Tg, H, W, h, w;
    int tile_h, tiles_x, bt0, lds_floats;
    float sx, sy, crop_x, crop_y;  // crop_* = float(crop_j0), float(crop_i0)
    float ks, kr, range_floor;     // -log2(e) / (2 sigma^2): the Gaussians as exp2
    float mean[3], stdv[3], scale[8];
};

// -------------------------------------------------------------------------------------------------
// Block = (tile of UP_TILE_W x tile_h full-resolution pixels, frame (b, t)); 256 threads, wave r takes the tile's rows r, r + 4, ...
// Staging: the low-resolution footprint of the tile (the window centres of its first and last pixel per axis, widened by R and cut to
// the image: x(X) is monotone in f32, so every tap of every inside pixel of the tile lies in it) goes to LDS once, one record of
// S = 4 + 4 C4 floats per tap: (de-normalised guide r, g, b, usable), then the C fields (0 when the tap is unusable, and in the
// padding channels).  A tap is one 16-byte LDS read for the guide and C4 for the fields.
// Pixel: 2 (2R + 1) exponentials for the separable spatial weight (the column factors once per thread, the row factor once per window
// row), then the (2R + 1)^2 taps in row-major order, one exponential each;
// a tap outside the footprint or unusable is read (index clamped) and given weight 0 by a select, so the order of the sum is fixed.
// -------------------------------------------------------------------------------------------------
template <int R, int C4>
__global__ __launch_bounds__(256) void guided_upsample_kernel(const UpParams p) {
    extern __shared__ __attribute__((aligned(16))) float up_lds[];
    constexpr int S = 4 + 4 * C4, NC = 4 * C4, K = 2 * R + 1;
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const int bt = p.bt0 + (int)blockIdx.y;
    const int b = bt / p.T, t = bt - b * p.T;
    const int X0 = tx * UP_TILE_W, Y0 = ty * p.tile_h;
    const int X1 = min(X0 + UP_TILE_W - 1, p.W - 1), Y1 = min(Y0 + p.tile_h - 1, p.H - 1);
    const int fi = p.frame_index ? p.frame_index[t] : t;
    const bool frame_ok = fi >= 0 && fi < p.Tg;

    const int qx0 = max(up_centre(up_coord(X0, p.sx, p.crop_x), p.w) - R, 0);
    const int qx1 = min(up_centre(up_coord(X1, p.sx, p.crop_x), p.w) + R, p.w - 1);
    const int qy0 = max(up_centre(up_coord(Y0, p.sy, p.crop_y), p.h) - R, 0);
    const int qy1 = min(up_centre(up_coord(Y1, p.sy, p.crop_y), p.h) + R, p.h - 1);
    const int fw = qx1 - qx0 + 1, fh = qy1 - qy0 + 1;
    // (the host sized the launch by the same arithmetic; a footprint it did not foresee is not staged and the tile comes out invalid)
    const int n = (frame_ok && fw > 0 && fh > 0 && (long long)fw * fh * S <= p.lds_floats) ? fw * fh : 0;

    const long long hw = (long long)p.h * p.w, thw = (long long)p.T * hw;
    const float* glo = p.guide_lo + ((long long)b * 3 * p.T + t) * hw;
    const float* slo = p.src + ((long long)b * p.C * p.T + t) * hw;
    for (int i = (int)threadIdx.x; i < n; i += 256) {
        const int ry = i / fw, rx = i - ry * fw;
        const long long q = (long long)(qy0 + ry) * p.w + (qx0 + rx);
        float v[NC];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            v[c] = c < p.C ? slo[c * thw + q] : 0.f;
            ok = ok && up_finite(v[c]);
        }
        f32x4* rec = reinterpret_cast<f32x4*>(up_lds + (long long)i * S);
        rec[0] = (f32x4){glo[q] * p.stdv[0] + p.mean[0], glo[thw + q] * p.stdv[1] + p.mean[1], glo[2 * thw + q] * p.stdv[2] + p.mean[2],
                         ok ? 1.f : 0.f};
#pragma unroll
        for (int g = 0; g < C4; ++g)
            rec[1 + g] = ok ? (f32x4){v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]} : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    const long long HW = (long long)p.H * p.W, THW = (long long)p.T * HW;
    const int X = X0 + ((int)threadIdx.x & 63);
    if (X >= p.W) return;
    const float x = up_coord(X, p.sx, p.crop_x);
    const bool in_x = x >= -0.5f && x < (float)p.w - 0.5f;
    const int cx = up_centre(x, p.w);
    float fxw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float d = x - (float)(cx + k - R);
        fxw[k] = __builtin_amdgcn_exp2f(d * d * p.ks);
    }
    for (int Y = Y0 + ((int)threadIdx.x >> 6); Y <= Y1; Y += 4) {
        const float y = up_coord(Y, p.sy, p.crop_y);
        const bool inside = in_x && y >= -0.5f && y < (float)p.h - 0.5f;
        float acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.f;
        float sum = 0.f;
        int used = 0;
        if (inside && n > 0) {
            const int cy = up_centre(y, p.h);
            const unsigned char* gp = p.guide_hi + ((((long long)b * p.Tg + fi) * p.H + Y) * p.W + X) * 3;
            const float r0 = (float)gp[0] / 255.f, r1 = (float)gp[1] / 255.f, r2 = (float)gp[2] / 255.f;
#pragma unroll 1  // (one window row at a time: unrolled, the K * K records in flight cost 150 to 256 registers)
            for (int ky = 0; ky < K; ++ky) {
                const int qy = cy + ky - R;
                const float dy = y - (float)qy;
                const float fy = __builtin_amdgcn_exp2f(dy * dy * p.ks);
                const bool row_in = qy >= qy0 && qy <= qy1;
                const int ry = min(max(qy - qy0, 0), fh - 1);
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int qx = cx + kx - R;
                    const bool tap_in = row_in && qx >= qx0 && qx <= qx1;
                    const int rx = min(max(qx - qx0, 0), fw - 1);
                    const f32x4* rec = reinterpret_cast<const f32x4*>(up_lds + (ry * fw + rx) * S);
                    const f32x4 g = rec[0];
                    const float d0 = r0 - g[0], d1 = r1 - g[1], d2 = r2 - g[2];
                    const float gw = __builtin_amdgcn_exp2f(fmaf(d2, d2, fmaf(d1, d1, d0 * d0)) * p.kr);
                    const bool use = tap_in && g[3] != 0.f;
                    const float wt = use ? fy * fxw[kx] * fmaxf(gw, p.range_floor) : 0.f;
                    used += use ? 1 : 0;
                    sum += wt;
#pragma unroll
                    for (int q4 = 0; q4 < C4; ++q4) {
                        const f32x4 s4 = rec[1 + q4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[4 * q4 + e] = fmaf(wt, s4[e], acc[4 * q4 + e]);
                    }
                }
            }
        }
        const bool ok = used > 0;
        const long long pix = (long long)Y * p.W + X;
        float* o = p.out + ((long long)b * p.C * p.T + t) * HW + pix;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < p.C) o[c * THW] = ok ? p.scale[c] * (acc[c] / sum) : 0.f;
        p.valid[((long long)b * p.T + t) * HW + pix] = ok ? 1 : 0;
    }
}

// the largest footprint extent along one axis over all tiles of `tile` full-resolution indices: the kernel's own arithmetic
static int up_footprint(int N, int tile, float s, float crop0, int n, int R) {
    int best = 0;
    for (int a = 0; a < N; a += tile) {
        const int last = a + tile - 1 < N - 1 ? a + tile - 1 : N - 1;
        const int q0 = std::max(up_centre(up_coord(a, s, crop0), n) - R, 0);
        const int q1 = std::min(up_centre(up_coord(last, s, crop0), n) + R, n - 1);
        best = std::max(best, q1 - q0 + 1);
    }
    return best;
}

template <int R>
static void up_launch(int C4, dim3 grid, size_t lds, hipStream_t s, const UpParams& p) {
    if (C4 == 1)
        hipLaunchKernelGGL((guided_upsample_kernel<R, 1>), grid, dim3(256), lds, s, p);
    else
        hipLaunchKernelGGL((guided_upsample_kernel<R, 2>), grid, dim3(256), lds, s, p);
}

extern "C" {

int l4p_guided_upsample(l4p_stream s_, const unsigned char* guide_hi, const int* frame_index, const float* guide_lo, const float* mean3,
                        const float* std3, const float* src, const float* scale, int B, int C, int T, int Tg, int H, int W, int res_h,
                        int res_w, int crop_i0, int crop_j0, int h, int w, int radius, float sigma_s, float sigma_r, float range_floor,
                        float* out, unsigned char* valid) {
    hipStream_t s = (hipStream_t)s_;
    const char* why = nullptr;
    if (B < 1 || C < 1 || T < 1 || Tg < 1 || H < 1 || W < 1 || res_h < 1 || res_w < 1 || h < 1 || w < 1) why = "a size below 1";
    else if (C > 8) why = "C > 8";
    else if (radius < 1 || radius > 3) why = "radius outside 1..3";
    else if (!(sigma_s > 0.f) || !(sigma_r > 0.f)) why = "sigma_s and sigma_r must be positive";
    else if (!(range_floor > 0.f && range_floor <= 1.f)) why = "range_floor outside (0, 1]";
    else if (res_h > H || res_w > W) why = "res_h > H or res_w > W: this is an up-sampler";
    else if (crop_i0 < 0 || crop_j0 < 0 || (long long)crop_i0 + h > res_h || (long long)crop_j0 + w > res_w) why = "the crop leaves the resized frame";
    else if (!frame_index && Tg != T) why = "Tg != T without frame_index";
    else if (!guide_hi || !guide_lo || !mean3 || !std3 || !src || !out || !valid) why = "a NULL pointer among guide_hi, guide_lo, mean3, std3, src, out, valid";
    if (why) {
        l4p_set_error("l4p_guided_upsample: %s (B=%d C=%d T=%d Tg=%d H=%d W=%d res=%dx%d crop=(%d, %d) h=%d w=%d radius=%d sigma_s=%g "
                      "sigma_r=%g range_floor=%g)", why, B, C, T, Tg, H, W, res_h, res_w, crop_i0, crop_j0, h, w, radius,
                      (double)sigma_s, (double)sigma_r, (double)range_floor);
        return L4P_E_INVALID;
    }
    UpParams p;
    p.guide_hi = guide_hi, p.frame_index = frame_index, p.guide_lo = guide_lo, p.src = src, p.out = out, p.valid = valid;
    p.C = C, p.T = T, p.Tg = Tg, p.H = H, p.W = W, p.h = h, p.w = w;
    p.sx = (float)res_w / (float)W, p.sy = (float)res_h / (float)H, p.crop_x = (float)crop_j0, p.crop_y = (float)crop_i0;
    const double log2e = 1.4426950408889634;
    p.ks = (float)(-log2e / (2.0 * (double)sigma_s * (double)sigma_s)), p.kr = (float)(-log2e / (2.0 * (double)sigma_r * (double)sigma_r));
    p.range_floor = range_floor;
    for (int k = 0; k < 3; ++k) p.mean[k] = mean3[k], p.stdv[k] = std3[k];
    for (int c = 0; c < 8; ++c) p.scale[c] = (scale && c < C) ? scale[c] : 1.f;
    // the tile height: the largest whose footprint record array fits the LDS request.  A one-row tile always does: at most
    // (64 + 2 radius + 1) x (2 radius + 1) records of 48 bytes, 24 KiB.
    const int C4 = C <= 4 ? 1 : 2, S = 4 + 4 * C4;
    const int fw = up_footprint(W, UP_TILE_W, p.sx, p.crop_x, w, radius);
    int tile_h = UP_TILE_H_MAX, fh = 0;
    for (;; tile_h >>= 1) {
        fh = up_footprint(H, tile_h, p.sy, p.crop_y, h, radius);
        if ((long long)fw * fh * S * 4 <= UP_LDS_BYTES || tile_h == 1) break;
    }
    const long long recs = (long long)std::max(fw, 0) * std::max(fh, 0);
    p.lds_floats = (int)(recs * S);
    p.tile_h = tile_h, p.tiles_x = (W + UP_TILE_W - 1) / UP_TILE_W;
    const long long tiles = (long long)p.tiles_x * ((H + tile_h - 1) / tile_h);
    if (tiles > 0x7FFFFFFFll) {
        l4p_set_error("l4p_guided_upsample: %lld tiles of a frame exceed the grid (H=%d W=%d)", tiles, H, W);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_guided_upsample");
    const long long frames = (long long)B * T;
    for (long long bt0 = 0; bt0 < frames; bt0 += 65535) {  // grid.y holds at most 65535 frames
        p.bt0 = (int)bt0;
        const dim3 grid((unsigned)tiles, (unsigned)std::min(frames - bt0, 65535ll));
        const size_t lds = (size_t)std::max(p.lds_floats, 4) * 4;
        if (radius == 1) up_launch<1>(C4, grid, lds, s, p);
        else if (radius == 2) up_launch<2>(C4, grid, lds, s, p);
        else up_launch<3>(C4, grid, lds, s, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
}
