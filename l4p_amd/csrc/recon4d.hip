// 4D reconstruction (reference generate_4D_visualization, l4p/utils/vis.py:107-221, with its helpers vis.py:621-766 and
// geometry_utils.py:13-143): world point clouds of every pixel of every frame, the camera path as frusta, and 3D track trails.
// The reference does this on the host (numpy loops over tracks x frames x trail segments); here every stage is a
// bandwidth- or latency-bound kernel.  All arithmetic is f32 (f64 where the reference itself computes in numpy float64: the
// frustum vertices, the trail interpolation, the hsv normalisation), and the file is compiled with -ffp-contract=off so that
// every f32 expression rounds operation by operation as ATen's unfused ops do (Makefile).
// Matrix layout everywhere: b44t / b16t of one clip, element (i, j) of frame t at [(i * 4 + j) * T + t].
#include "common.hpp"
#include "prof.hpp"
#include "unproject.hpp"
#include "stable_argsort.hpp"  // recon_argsort_kernel: the height order of the tracks (vis.py:722), shared with vis2d.hip

// 4x4 inverse in double, Gauss-Jordan with partial pivoting (row-major in and out)
__device__ void inv4_d(const double* a, double* o) {
    double m[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            m[i][j] = a[i * 4 + j];
            m[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (fabs(m[r][c]) > fabs(m[piv][c])) piv = r;
        if (piv != c)
            for (int j = 0; j < 8; ++j) {
                const double t = m[c][j];
                m[c][j] = m[piv][j];
                m[piv][j] = t;
            }
        const double ip = 1.0 / m[c][c];
        for (int j = 0; j < 8; ++j) m[c][j] *= ip;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double f = m[r][c];
                for (int j = 0; j < 8; ++j) m[r][j] -= f * m[c][j];
            }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[i * 4 + j] = m[i][4 + j];
}

// -------------------------------------------------------------------------------------------------
// Cameras, one thread per (clip b, frame t) (vis.py:138-141, get_cam_T_ref geometry_utils.py:128-143,
// generate_video_camera_trajectory vis.py:621-641).  A [B][16][T]: the camray head's pose traj3d (a_is_pose = 1:
// cam_T_world_t = A_t^-1, vis.py:138) or cam_T_world itself (a_is_pose = 0); cam_T_ref_t = cam_T_world_t cam_T_world_ref^-1,
// world_T_cam_t = cam_T_ref_t^-1 (of the stored f32 matrix), frustum vertices world_T_cam_t [v; 1] of create_camera_frustum's
// 8 camera-frame vertices (vis.py:529-618).  The chain runs in double and rounds once per stored matrix; the reference chains
// f32 inverses and products (numpy float64 for the frustum).  world_T_cam and verts may be NULL.
// -------------------------------------------------------------------------------------------------
__global__ void recon_cameras_kernel(const float* __restrict__ A, int B, int T, int ref, int a_is_pose, double tan_half_fov,
                                     double near_d, double far_d, float* __restrict__ cam_T_ref, float* __restrict__ world_T_cam,
                                     float* __restrict__ verts) {
    const int bt = blockIdx.x * blockDim.x + threadIdx.x;
    if (bt >= B * T) return;
    const int b = bt / T, t = bt % T;
    const float* a = A + (long long)b * 16 * T;
    double Ar[16], At[16], Ct[16], Rinv[16], R[16], Ci[16];
    for (int k = 0; k < 16; ++k) {
        Ar[k] = a[(long long)k * T + ref];
        At[k] = a[(long long)k * T + t];
    }
    if (a_is_pose) {
        inv4_d(At, Ct);  // cam_T_world_t
        for (int k = 0; k < 16; ++k) Rinv[k] = Ar[k];  // cam_T_world_ref^-1 = A_ref
    } else {
        for (int k = 0; k < 16; ++k) Ct[k] = At[k];
        inv4_d(Ar, Rinv);
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += Ct[i * 4 + k] * Rinv[k * 4 + j];
            R[i * 4 + j] = (double)(float)acc;  // the stored f32 cam_T_ref is what gets inverted
        }
    for (int k = 0; k < 16; ++k) cam_T_ref[((long long)b * 16 + k) * T + t] = (float)R[k];
    if (!world_T_cam && !verts) return;
    inv4_d(R, Ci);
    if (world_T_cam)
        for (int k = 0; k < 16; ++k) world_T_cam[((long long)b * 16 + k) * T + t] = (float)Ci[k];
    if (!verts) return;
    // create_camera_frustum(fov 45, near, far, aspect 1): height = 2 near tan(fov / 2), width = height
    const double nh = 2 * near_d * tan_half_fov, fh = 2 * far_d * tan_half_fov;
    const double sx[4] = {-1, 1, 1, -1}, sy[4] = {-1, -1, 1, 1};
    for (int v = 0; v < 8; ++v) {
        const double h = v < 4 ? nh : fh, z = v < 4 ? near_d : far_d;
        const double cv[3] = {sx[v & 3] * h / 2, sy[v & 3] * h / 2, z};
        for (int i = 0; i < 3; ++i) {
            const double w = cv[0] * Ci[i * 4 + 0] + cv[1] * Ci[i * 4 + 1] + cv[2] * Ci[i * 4 + 2] + Ci[i * 4 + 3];
            verts[((long long)bt * 8 + v) * 3 + i] = (float)w;
        }
    }
}

// Open3D's colour rule (PLY uchar): min(255, max(0, c * 255)) in double, truncated
__device__ __forceinline__ unsigned char colour_u8(double c) {
    const double v = c * 255.0;
    return (unsigned char)(v > 255.0 ? 255.0 : (v > 0.0 ? v : 0.0));
}

// -------------------------------------------------------------------------------------------------
// Dense point map (generate_point_map, geometry_utils.py:13-53, every pixel kept), one pixel per thread, grid-stride.
// depth [B][T][H*W]; K, P: [B][16][T]; point (b, t, pix) component c goes to xyz[b * bs + (t * HW + pix) * ps + c * cs].
// Optional colour (generate_4D_visualization vis.py:143, B = 1): rgb [3][T][H*W] * std[c] + mean[c], stored with Open3D's rule.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void recon_points_kernel(const float* __restrict__ depth, const float* __restrict__ K,
                                                           const float* __restrict__ P, int B, int T, int HW, int W,
                                                           float* __restrict__ xyz, long long ps, long long cs, long long bs,
                                                           const float* __restrict__ rgb, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, unsigned char* __restrict__ rgb_u8) {
    const long long n = (long long)B * T * HW, thw = (long long)T * HW;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / thw);
        const long long q = idx - b * thw;  // t * HW + pix
        const int t = (int)(q / HW), pix = (int)(q - (long long)t * HW);
        const long long mo = (long long)b * 16 * T + t;
        float ox, oy, oz;
        unproject_pixel(K + mo, P + mo, T, (float)(pix % W), (float)(pix / W), depth[idx], ox, oy, oz);
        float* o = xyz + b * bs + q * ps;
        o[0] = ox;
        o[cs] = oy;
        o[2 * cs] = oz;
        if (rgb_u8) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = rgb[c * thw + q] * stdv[c] + mean[c];
                rgb_u8[q * 3 + c] = colour_u8((double)v);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// 3D track points (generate_3d_track_point_map + unproject_2d_track_to_3d, geometry_utils.py:56-106): X = (x - cx) Z / fx,
// Y = (y - cy) Z / fy, then P [X Y Z 1].  traj [B][N][2][T], depth [B][N][T]; Z = scale[0] * depth when `scale` is given
// (vis.py:169); output row i takes track order[b * N + i] when `order` is given (the height sort of vis.py:722-727).
// out [B][N][3][T].  One thread per (b, i, t).
// -------------------------------------------------------------------------------------------------
__global__ void recon_track_points_kernel(const float* __restrict__ traj, const float* __restrict__ tdepth,
                                          const float* __restrict__ K, const float* __restrict__ P,
                                          const float* __restrict__ scale, const int* __restrict__ order, int B, int N, int T,
                                          float* __restrict__ out) {
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= (long long)B * N * T) return;
    const int t = (int)(idx % T);
    const long long bi = idx / T;
    const int b = (int)(bi / N), i = (int)(bi % N);
    const int n = order ? order[(long long)b * N + i] : i;
    const long long src = (long long)b * N + n;
    const float x = traj[(src * 2 + 0) * T + t], y = traj[(src * 2 + 1) * T + t];
    float Z = tdepth[src * T + t];
    if (scale) Z = scale[0] * Z;
    const float* k = K + (long long)b * 16 * T + t;
    const float* p = P + (long long)b * 16 * T + t;
    const float X = (x - k[2 * T]) * Z / k[0], Y = (y - k[6 * T]) * Z / k[5 * T];
    float* o = out + bi * 3 * T + t;
    for (int c = 0; c < 3; ++c) o[(long long)c * T] = p[(c * 4 + 0) * T] * X + p[(c * 4 + 1) * T] * Y + p[(c * 4 + 2) * T] * Z + p[(c * 4 + 3) * T];
}

// -------------------------------------------------------------------------------------------------
// Track preparation, one workgroup per frame t, tracks in sorted order i (vis.py:146-169 and the visibility test of
// vis.py:745): visible = sigmoid(logit) > vis_thr; the depth map sampled at the track position as grid_sample(mode="nearest",
// align_corners=False) does after the reference's normalisation by (W - 1), (H - 1) on the device: source index
// ((g + 1) W - 1) / 2 with g = x * (1 / (W - 1)) * 2 - 1, rounded half to even, 0 outside the image; ratio = sample / depth.
// ratios [T][N]: the ratio of a visible pair, the largest key of the select (NaN bits 0x7FFFFFFF) for an invisible one, so
// that rank (nvis - 1) / 2 of all T N values is the lower median of the visible ones; flag |= 1 for a visible NaN ratio.
// slot [T][N]: rank of a visible track among the visible tracks of its frame (sorted order), -1 if invisible.
// counts [T]: visible tracks per frame.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void recon_track_prep_kernel(const float* __restrict__ traj, const float* __restrict__ vis_logit,
                                                               const float* __restrict__ tdepth, const float* __restrict__ dmap,
                                                               const int* __restrict__ order, int N, int T, int H, int W,
                                                               float vis_thr, float* __restrict__ ratios, int* __restrict__ slot,
                                                               int* __restrict__ flag, int* __restrict__ counts) {
    __shared__ int wtot[4];
    const int t = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool vis = false;
        if (i < N) {
            const long long n = order[i];
            const float lg = vis_logit[n * T + t];
            vis = 1.f / (1.f + expf(-lg)) > vis_thr;
            float r = __int_as_float(0x7FFFFFFF);
            if (vis) {
                const float x = traj[(n * 2 + 0) * T + t], y = traj[(n * 2 + 1) * T + t];
                // ATen's device division by a host scalar is a product with its f32 reciprocal (div_true_kernel_cuda)
                const float gx = x * (1.f / (float)(W - 1)) * 2.f - 1.f, gy = y * (1.f / (float)(H - 1)) * 2.f - 1.f;
                const float ix = rintf(((gx + 1.f) * (float)W - 1.f) / 2.f), iy = rintf(((gy + 1.f) * (float)H - 1.f) / 2.f);
                float d = 0.f;
                if (ix >= 0.f && ix < (float)W && iy >= 0.f && iy < (float)H) d = dmap[((long long)t * H + (int)iy) * W + (int)ix];
                r = d / tdepth[n * T + t];
                if (r != r) atomicOr(flag, 1);
            }
            ratios[(long long)t * N + i] = r;
        }
        const unsigned long long m = __ballot(vis);
        if (lane == 0) wtot[wid] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wid; ++w) before += wtot[w];
        if (i < N) slot[(long long)t * N + i] = vis ? before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[t] = base;
}

// point offsets of the frames' trail blocks: off[0] = 0, off[t + 1] = off[t] + counts[t] * points(t), off[T + 1] = visible pairs
// points(t) = 1 when min(t, trail) = 0, else seg * min(t, trail) (vis.py:748-764)
__device__ __forceinline__ long long trail_points(int t, int trail, int seg) {
    const int L = t < trail ? t : trail;
    return L == 0 ? 1 : (long long)seg * L;
}
__global__ void recon_offsets_kernel(const int* __restrict__ counts, int T, int trail, int seg, long long* __restrict__ off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long acc = 0, vis = 0;
    off[0] = 0;
    for (int t = 0; t < T; ++t) {
        acc += counts[t] * trail_points(t, trail, seg);
        vis += counts[t];
        off[t + 1] = acc;
    }
    off[T + 1] = vis;
}

// scale = the order statistic found by l4p_select_rank, read as the key it leaves in ws[0] (umeyama.hip qsel_*: the exact
// element, where the lerp of its output would turn an infinite neighbour into NaN); NaN when a visible ratio is NaN or no pair
// is visible (torch.median)
__global__ void recon_scale_kernel(const unsigned* __restrict__ ws, const int* __restrict__ flag, int any, float* __restrict__ scale) {
    if (threadIdx.x != 0) return;
    if (!any || flag[0]) {
        scale[0] = __int_as_float(0x7FC00000);
        return;
    }
    const unsigned k = ws[0];
    scale[0] = __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// -------------------------------------------------------------------------------------------------
// Trails (generate_3d_track_point_clouds vis.py:738-766), one wave per (frame t, sorted track i), visible ones only:
// L = min(t, trail) segments over frames t - L .. t, each start + (stop - start) * linspace(0, 1, seg) in float64 as numpy
// computes it (f32 difference, f64 product and sum; the last alpha is exactly 1), or the single point X_t when L = 0.
// Points land at off[t] + slot * points(t); colour: matplotlib hsv of Normalize(0, N - 1)(i) (float64, times 256, truncated,
// 256 -> 255), through lut [256][3] (uchar, Open3D's rule).  X: [N][3][T] in sorted order.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void recon_trails_kernel(const float* __restrict__ X, const int* __restrict__ slot,
                                                           const long long* __restrict__ off, const unsigned char* __restrict__ lut,
                                                           int N, int T, int trail, int seg, float* __restrict__ xyz,
                                                           unsigned char* __restrict__ rgb) {
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pair >= (long long)T * N) return;
    const int t = (int)(pair / N), i = (int)(pair % N);
    const int s = slot[pair];
    if (s < 0) return;
    const int L = t < trail ? t : trail;
    const long long np = trail_points(t, trail, seg);
    const long long o0 = off[t] + (long long)s * np;
    double f = N > 1 ? (double)i / (double)(N - 1) : 0.0;
    f *= 256.0;
    const int ci = f >= 256.0 ? 255 : (int)f;
    const unsigned char c0 = lut[ci * 3], c1 = lut[ci * 3 + 1], c2 = lut[ci * 3 + 2];
    const float* x = X + (long long)i * 3 * T;
    const double step = 1.0 / (double)(seg - 1);
    for (long long p = lane; p < np; p += 64) {
        float v[3];
        if (L == 0) {
            for (int c = 0; c < 3; ++c) v[c] = x[(long long)c * T + t];
        } else {
            const int k = (int)(p / seg), a = (int)(p % seg), t0 = t - L + k;
            const double alpha = a == seg - 1 ? 1.0 : (double)a * step;
            for (int c = 0; c < 3; ++c) {
                const float st = x[(long long)c * T + t0], sp = x[(long long)c * T + t0 + 1];
                v[c] = (float)((double)st + (double)(sp - st) * alpha);
            }
        }
        float* o = xyz + (o0 + p) * 3;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        unsigned char* q = rgb + (o0 + p) * 3;
        q[0] = c0;
        q[1] = c1;
        q[2] = c2;
    }
}

static int grid_for(long long n, int cap) { return (int)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

extern "C" {

int l4p_recon_cameras(l4p_stream s_, const float* A, int B, int T, int ref, int a_is_pose, double tan_half_fov, double near_d,
                      double far_d, float* cam_T_ref, float* world_T_cam, float* frustum) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || T < 1 || ref < 0 || ref >= T || !A || !cam_T_ref) {
        l4p_set_error("l4p_recon_cameras: need B, T >= 1, 0 <= ref < T, A and cam_T_ref (B=%d T=%d ref=%d)", B, T, ref);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_recon_cameras");
    hipLaunchKernelGGL(recon_cameras_kernel, dim3((B * T + 63) / 64), dim3(64), 0, s, A, B, T, ref, a_is_pose & 1, tan_half_fov,
                       near_d, far_d, cam_T_ref, world_T_cam, frustum);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_point_map(l4p_stream s_, const float* depth, const float* K, const float* P, int B, int T, int H, int W, float* xyz,
                  long long ps, long long cs, long long bs, const float* rgb, const float* mean, const float* stdv,
                  unsigned char* rgb_u8) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || T < 1 || H < 1 || W < 1 || !depth || !K || !P || !xyz || (rgb_u8 && (B != 1 || !rgb || !mean || !stdv))) {
        l4p_set_error("l4p_point_map: bad arguments (B=%d T=%d H=%d W=%d; colour needs B = 1 and rgb, mean, std)", B, T, H, W);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_point_map");
    const long long n = (long long)B * T * H * W;
    hipLaunchKernelGGL(recon_points_kernel, dim3(grid_for(n, 8192)), dim3(256), 0, s, depth, K, P, B, T, H * W, W, xyz, ps, cs, bs,
                       rgb, mean, stdv, rgb_u8);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_track_point_map(l4p_stream s_, const float* traj, const float* tdepth, const float* K, const float* P, const float* scale,
                        const int* order, int B, int N, int T, float* out) {
    hipStream_t s = (hipStream_t)s_;
    if (B < 1 || N < 0 || T < 1 || !traj || !tdepth || !K || !P || !out) {
        l4p_set_error("l4p_track_point_map: bad arguments (B=%d N=%d T=%d)", B, N, T);
        return L4P_E_INVALID;
    }
    const long long n = (long long)B * N * T;
    if (n == 0) return 0;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_track_point_map");
    hipLaunchKernelGGL(recon_track_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, traj, tdepth, K, P, scale, order,
                       B, N, T, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_recon_track_prep(l4p_stream s_, const float* traj, const float* vis_logit, const float* tdepth, const float* dmap, int N,
                         int T, int H, int W, float vis_thr, int trail, int seg, int* order, int* slot, float* ratios, int* flag,
                         int* counts, long long* off) {
    hipStream_t s = (hipStream_t)s_;
    if (N < 1 || T < 1 || H < 2 || W < 2 || trail < 0 || seg < 2 || (long long)N * T > 0x7FFFFFFFll) {
        l4p_set_error("l4p_recon_track_prep: need N, T >= 1, H, W >= 2, trail >= 0, seg >= 2, N T < 2^31 (N=%d T=%d H=%d W=%d)", N, T,
                      H, W);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_recon_track_prep");
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(recon_argsort_kernel, dim3((N + 3) / 4), dim3(256), 0, s, traj, N, T, order);
    hipLaunchKernelGGL(recon_track_prep_kernel, dim3(T), dim3(256), 0, s, traj, vis_logit, tdepth, dmap, order, N, T, H, W, vis_thr,
                       ratios, slot, flag, counts);
    hipLaunchKernelGGL(recon_offsets_kernel, dim3(1), dim3(64), 0, s, counts, T, trail, seg, off);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_recon_track_scale(l4p_stream s_, const float* ratios, long long n, long long nvis, const int* flag, unsigned* ws,
                          float* sel, float* scale) {
    hipStream_t s = (hipStream_t)s_;
    if (n < 1 || nvis < 0 || nvis > n) {
        l4p_set_error("l4p_recon_track_scale: need n >= 1 and 0 <= nvis <= n (n=%lld nvis=%lld)", n, nvis);
        return L4P_E_INVALID;
    }
    if (nvis > 0) {
        const int rc = l4p_select_rank(s_, ratios, n, (nvis - 1) / 2, ws, sel);
        if (rc) return rc;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_recon_track_scale");
    hipLaunchKernelGGL(recon_scale_kernel, dim3(1), dim3(64), 0, s, ws, flag, nvis > 0 ? 1 : 0, scale);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_recon_trails(l4p_stream s_, const float* X, const int* slot, const long long* off, const unsigned char* lut, int N, int T,
                     int trail, int seg, long long total, float* xyz, unsigned char* rgb) {
    hipStream_t s = (hipStream_t)s_;
    if (N < 1 || T < 1 || trail < 0 || seg < 2 || total < 0) {
        l4p_set_error("l4p_recon_trails: bad arguments (N=%d T=%d trail=%d seg=%d total=%lld)", N, T, trail, seg, total);
        return L4P_E_INVALID;
    }
    if (total == 0) return 0;  // nothing visible: no launch
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_recon_trails");
    const long long pairs = (long long)N * T;
    hipLaunchKernelGGL(recon_trails_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, X, slot, off, lut, N, T, trail, seg,
                       xyz, rgb);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
