// Free-viewpoint renderer of the 4D reconstruction (what the reference shows through its viser viewer, l4p/utils/viser.py:58-75:
// the point cloud of frame t with its track trails and the camera frustum, from a camera the user moves): the device tensors of
// recon4d.hip splatted into a depth-tested image.  The viewer's own GPU rasteriser cannot be run or read here, so the rules are
// the project's own (include/l4p_hip.h states them; tests/view4d_restate.py restates them in numpy and is held bit for bit).
// Everything is f32, every operation rounds on its own in the order written (the file is compiled with -ffp-contract=off), and
// the depth test is an integer atomicMin on a 64-bit key, so the image does not depend on the order in which points arrive.
//
// Key of a pixel: (bits(z) << 32) | low word.  z >= near > 0 is finite, and a positive f32 orders as its bit pattern, so the
// smallest key is the nearest surface; among equal z the smallest low word wins.  Low word of a point: its local index i
// (dense pixels [0, HW), then the frame's trail points; i < 2^31).  Low word of a triangle: 0x80000000 | (frame << 4 | tri).
// An empty pixel holds all ones (a NaN pattern no surface can produce).
#include "common.hpp"
#include "prof.hpp"

#define VIEW_EMPTY 0xFFFFFFFFFFFFFFFFull

struct ViewCam {
    float m[12];  // rows 0..2 of cam_T_world
    float fx, fy, cx, cy;
};

__device__ __forceinline__ ViewCam view_cam(const float* __restrict__ cam_T_world, const float* __restrict__ intr, int v) {
    ViewCam c;
    const float* M = cam_T_world + (long long)v * 16;
#pragma unroll
    for (int k = 0; k < 12; ++k) c.m[k] = M[k];
    const float* K = intr + (long long)v * 4;
    c.fx = K[0];
    c.fy = K[1];
    c.cx = K[2];
    c.cy = K[3];
    return c;
}

__device__ __forceinline__ bool view_finite(float a) { return fabsf(a) <= 3.402823466e38f; }  // false for NaN and +-inf

// rule steps 1-4: camera coordinates and the continuous pixel position; false = the point is skipped
__device__ __forceinline__ bool view_project(const ViewCam& c, float X, float Y, float Z, float near_z, float& u, float& v, float& z) {
    const float x = ((c.m[0] * X + c.m[1] * Y) + c.m[2] * Z) + c.m[3];
    const float y = ((c.m[4] * X + c.m[5] * Y) + c.m[6] * Z) + c.m[7];
    z = ((c.m[8] * X + c.m[9] * Y) + c.m[10] * Z) + c.m[11];
    if (!view_finite(x) || !view_finite(y) || !view_finite(z) || z < near_z) return false;
    u = (c.fx * x) / z + c.cx;
    v = (c.fy * y) / z + c.cy;
    return fabsf(u) < 1048576.f && fabsf(v) < 1048576.f;
}

// the depth test: read first (the buffer only ever decreases, so a stale read costs an atomic, never a miss)
__device__ __forceinline__ void view_put(unsigned long long* __restrict__ p, unsigned long long key) {
    if (key < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, key);
}

// the trail block of frame t, or an empty one when the offsets do not describe a block inside track_xyz
__device__ __forceinline__ void view_trail_block(const long long* __restrict__ off, int t, long long n_track, long long& o0, long long& cnt) {
    o0 = 0;
    cnt = 0;
    if (!off || n_track <= 0) return;
    const long long a = off[t], b = off[t + 1];
    if (a < 0 || b < a || b > n_track) return;
    o0 = a;
    cnt = b - a;
}

// -------------------------------------------------------------------------------------------------
// Splat: grid (blocks, V); the blocks of a view stride over its points.  Each lane projects one point; a splat of at most 3 x 3
// pixels is written by its own lane, a larger one is spread over the wave (its rows of pixels are contiguous, so one
// wave-instruction touches few cache lines and the lanes of a wave do not wait for the one with the largest square).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void view_splat_kernel(const float* __restrict__ points, const float* __restrict__ track_xyz,
                                                         const long long* __restrict__ off, int T, int HW, long long n_track,
                                                         const float* __restrict__ cam_T_world, const float* __restrict__ intr,
                                                         const int* __restrict__ frame, int Ho, int Wo, float point_size,
                                                         float max_half, float near_z, unsigned long long* __restrict__ zbuf) {
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int t = frame[v];
    if (t < 0 || t >= T) return;  // a view of no frame stays empty
    long long o0, cnt;
    view_trail_block(off, t, n_track, o0, cnt);
    long long n = (long long)HW + cnt;
    if (n > 0x7FFFFFFFll) n = 0x7FFFFFFFll;  // the low word's point range
    const ViewCam c = view_cam(cam_T_world, intr, v);
    unsigned long long* zb = zbuf + (long long)v * Ho * Wo;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // uniform trip count
        const long long i = base + threadIdx.x;
        bool ok = i < n;
        int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        unsigned long long key = VIEW_EMPTY;
        if (ok) {
            const float* P = i < HW ? points + ((long long)t * HW + i) * 3 : track_xyz + (o0 + (i - HW)) * 3;
            float u, w, z;
            ok = view_project(c, P[0], P[1], P[2], near_z, u, w, z);
            if (ok) {
                const int px = (int)floorf(u + 0.5f), py = (int)floorf(w + 0.5f);
                const float r = ((point_size * c.fx) / z) * 0.5f;
                const float hf = floorf(r < max_half ? r : max_half);
                ok = hf >= 0.f;  // false for NaN (a non-finite or negative fx)
                if (ok) {
                    const int h = (int)hf;
                    x0 = px - h < 0 ? 0 : px - h;
                    x1 = px + h > Wo - 1 ? Wo - 1 : px + h;
                    y0 = py - h < 0 ? 0 : py - h;
                    y1 = py + h > Ho - 1 ? Ho - 1 : py + h;
                    ok = x0 <= x1 && y0 <= y1;
                    key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)i;
                }
            }
        }
        const int w = x1 - x0 + 1, hgt = y1 - y0 + 1;
        const bool big = ok && w * hgt > 9;
        if (ok && !big)
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) view_put(zb + (long long)y * Wo + x, key);
        unsigned long long m = __ballot(big);
        while (m) {  // wave-uniform
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int sx0 = __shfl(x0, src), sy0 = __shfl(y0, src), sw = __shfl(w, src), sn = sw * __shfl(hgt, src);
            const unsigned khi = __shfl((unsigned)(key >> 32), src), klo = __shfl((unsigned)key, src);
            const unsigned long long k = ((unsigned long long)khi << 32) | klo;
            for (int p = lane; p < sn; p += 64) view_put(zb + (long long)(sy0 + p / sw) * Wo + (sx0 + p % sw), k);
        }
    }
}

// create_camera_frustum's 12 triangles (l4p/utils/vis.py:529-618; FRUSTUM_TRIANGLES of utils/recon4d.py)
__constant__ int VIEW_TRI[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 3, 7}, {0, 7, 4},
                                    {1, 5, 6}, {1, 6, 2}, {0, 4, 5}, {0, 5, 1}, {3, 2, 6}, {3, 6, 7}};
// colour of triangle k: (255, 127, 127) * VIEW_SHADE[k] / 32 in integers (FRUSTUM_SHADE of utils/view4d.py)
__constant__ int VIEW_SHADE[12] = {32, 31, 18, 17, 27, 26, 23, 22, 29, 28, 21, 20};

// frame f is drawn in a view of frame t: f = t, or with stride s >= 1 every f <= t with f % s = 0
__device__ __forceinline__ bool view_frustum_drawn(int f, int t, int stride) { return f == t || (stride >= 1 && f < t && f % stride == 0); }

// -------------------------------------------------------------------------------------------------
// Frustum triangles, one workgroup per (triangle, frame f, view): two-sided raster over the clipped bounding box.
// Vertices P_k -> (u_k, v_k, z_k) by rule steps 1-4 (a skipped vertex skips the triangle).  With d(a, b, p) =
// (u_b - u_a) * (p_y - v_a) - (v_b - v_a) * (p_x - u_a):  A = d(0, 1, P_2); e0 = d(1, 2, p), e1 = d(2, 0, p), e2 = d(0, 1, p) at
// the pixel's integer coordinate p; b_k = e_k / A; the pixel is covered when b0, b1, b2 >= 0 (edges included, either
// orientation); z = 1 / ((b0 / z0 + b1 / z1) + b2 / z2), kept when finite and >= near.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float view_edge(float ua, float va, float ub, float vb, float px, float py) {
    return (ub - ua) * (py - va) - (vb - va) * (px - ua);
}

__global__ __launch_bounds__(256) void view_mesh_kernel(const float* __restrict__ frustum, int T, const float* __restrict__ cam_T_world,
                                                        const float* __restrict__ intr, const int* __restrict__ frame, int Ho, int Wo,
                                                        int stride, float near_z, unsigned long long* __restrict__ zbuf) {
    const int tri = blockIdx.x, f = blockIdx.y, v = blockIdx.z;
    const int t = frame[v];
    if (t < 0 || t >= T || !view_frustum_drawn(f, t, stride)) return;
    const ViewCam c = view_cam(cam_T_world, intr, v);
    float u[3], w[3], z[3];
    for (int k = 0; k < 3; ++k) {
        const float* P = frustum + ((long long)f * 8 + VIEW_TRI[tri][k]) * 3;
        if (!view_project(c, P[0], P[1], P[2], near_z, u[k], w[k], z[k])) return;
    }
    const float A = view_edge(u[0], w[0], u[1], w[1], u[2], w[2]);
    if (!(A != 0.f) || !view_finite(A)) return;  // zero area (or NaN)
    const float ulo = fminf(u[0], fminf(u[1], u[2])), uhi = fmaxf(u[0], fmaxf(u[1], u[2]));
    const float wlo = fminf(w[0], fminf(w[1], w[2])), whi = fmaxf(w[0], fmaxf(w[1], w[2]));
    // |u|, |v| < 2^20: the casts are exact
    int x0 = (int)ceilf(ulo), x1 = (int)floorf(uhi), y0 = (int)ceilf(wlo), y1 = (int)floorf(whi);
    x0 = x0 < 0 ? 0 : x0;
    y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > Wo - 1 ? Wo - 1 : x1;
    y1 = y1 > Ho - 1 ? Ho - 1 : y1;
    if (x0 > x1 || y0 > y1) return;
    const int bw = x1 - x0 + 1;
    const long long np = (long long)bw * (y1 - y0 + 1);
    const unsigned low = 0x80000000u | ((unsigned)f << 4) | (unsigned)tri;
    unsigned long long* zb = zbuf + (long long)v * Ho * Wo;
    for (long long p = threadIdx.x; p < np; p += 256) {
        const int y = y0 + (int)(p / bw), x = x0 + (int)(p % bw);
        const float px = (float)x, py = (float)y;
        const float b0 = view_edge(u[1], w[1], u[2], w[2], px, py) / A;
        const float b1 = view_edge(u[2], w[2], u[0], w[0], px, py) / A;
        const float b2 = view_edge(u[0], w[0], u[1], w[1], px, py) / A;
        if (!(b0 >= 0.f && b1 >= 0.f && b2 >= 0.f)) continue;
        const float zp = 1.f / ((b0 / z[0] + b1 / z[1]) + b2 / z[2]);
        if (!view_finite(zp) || zp < near_z) continue;
        view_put(zb + (long long)y * Wo + x, ((unsigned long long)__float_as_uint(zp) << 32) | low);
    }
}

// -------------------------------------------------------------------------------------------------
// Resolve, one pixel per thread: the winner's colour, camera z and low word.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void view_resolve_kernel(const unsigned long long* __restrict__ zbuf, const unsigned char* __restrict__ colors,
                                                           const unsigned char* __restrict__ track_colors, const long long* __restrict__ off,
                                                           int T, int HW, long long n_track, const int* __restrict__ frame, int V,
                                                           long long HoWo, unsigned bg, unsigned char* __restrict__ image,
                                                           float* __restrict__ depth, int* __restrict__ index) {
    const long long n = (long long)V * HoWo;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = zbuf[q];
        unsigned char r = (unsigned char)(bg & 255u), g = (unsigned char)((bg >> 8) & 255u), b = (unsigned char)((bg >> 16) & 255u);
        float z = __uint_as_float(0x7F800000u);
        int idx = -1;
        if (key != VIEW_EMPTY) {
            const unsigned lo = (unsigned)key;
            z = __uint_as_float((unsigned)(key >> 32));
            idx = (int)lo;
            if (lo & 0x80000000u) {
                const int s = VIEW_SHADE[(lo & 15u) < 12u ? (lo & 15u) : 0];
                r = (unsigned char)((255 * s) >> 5);
                g = b = (unsigned char)((127 * s) >> 5);
            } else {
                const int t = frame[(int)(q / HoWo)];
                const unsigned char* col = nullptr;
                if (t >= 0 && t < T) {
                    if ((long long)lo < HW) {
                        col = colors + ((long long)t * HW + lo) * 3;
                    } else if (track_colors) {
                        long long o0, cnt;
                        view_trail_block(off, t, n_track, o0, cnt);
                        if ((long long)lo - HW < cnt) col = track_colors + (o0 + ((long long)lo - HW)) * 3;
                    }
                }
                if (col) {  // always, for a buffer the launchers of this file filled with the same arguments
                    r = col[0];
                    g = col[1];
                    b = col[2];
                }
            }
        }
        image[q * 3] = r;
        image[q * 3 + 1] = g;
        image[q * 3 + 2] = b;
        depth[q] = z;
        index[q] = idx;
    }
}

static bool view_common_ok(const void* cam_T_world, const void* intr, const void* frame, int T, int V, int Ho, int Wo, const void* zbuf) {
    return cam_T_world && intr && frame && zbuf && T >= 1 && V >= 1 && V <= 65535 && Ho >= 1 && Wo >= 1 &&
           (long long)Ho * Wo <= 0x7FFFFFFFll;
}

extern "C" {

int l4p_view_splat(l4p_stream s_, const float* points, const float* track_xyz, const long long* off, int T, int HW, long long n_track,
                   const float* cam_T_world, const float* intr, const int* frame, int V, int Ho, int Wo, float point_size,
                   int max_half, float near_z, unsigned long long* zbuf) {
    hipStream_t s = (hipStream_t)s_;
    const bool tracks = track_xyz && off && n_track > 0;
    if (!view_common_ok(cam_T_world, intr, frame, T, V, Ho, Wo, zbuf) || !points || HW < 1 || n_track < 0 ||
        (long long)HW + n_track > 0x7FFFFFFFll || !(point_size >= 0.f) || !(point_size <= 3.0e38f) || max_half < 0 || max_half > 64 ||
        !(near_z > 0.f)) {
        l4p_set_error("l4p_view_splat: bad arguments (T=%d HW=%d n_track=%lld V=%d Ho=%d Wo=%d point_size=%g max_half=%d near=%g): "
                      "1 <= V <= 65535, HW + n_track < 2^31, finite point_size >= 0, 0 <= max_half <= 64, near > 0",
                      T, HW, n_track, V, Ho, Wo, (double)point_size, max_half, (double)near_z);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_view_splat");
    HIP_TRY(hipMemsetAsync(zbuf, 0xFF, (size_t)V * Ho * Wo * sizeof(unsigned long long), s));
    const long long most = (long long)HW + (tracks ? n_track : 0), blocks = (most + 255) / 256;
    hipLaunchKernelGGL(view_splat_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048), V), dim3(256), 0, s, points,
                       tracks ? track_xyz : nullptr, tracks ? off : nullptr, T, HW, tracks ? n_track : 0, cam_T_world, intr, frame, Ho, Wo,
                       point_size, (float)max_half, near_z, zbuf);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_view_mesh(l4p_stream s_, const float* frustum, int T, const float* cam_T_world, const float* intr, const int* frame, int V,
                  int Ho, int Wo, int stride, float near_z, unsigned long long* zbuf) {
    hipStream_t s = (hipStream_t)s_;
    if (!view_common_ok(cam_T_world, intr, frame, T, V, Ho, Wo, zbuf) || !frustum || T > 65535 || stride < 0 || !(near_z > 0.f)) {
        l4p_set_error("l4p_view_mesh: bad arguments (T=%d V=%d Ho=%d Wo=%d stride=%d near=%g): 1 <= T, V <= 65535, stride >= 0, near > 0",
                      T, V, Ho, Wo, stride, (double)near_z);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_view_mesh");
    hipLaunchKernelGGL(view_mesh_kernel, dim3(12, T, V), dim3(256), 0, s, frustum, T, cam_T_world, intr, frame, Ho, Wo, stride, near_z,
                       zbuf);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_view_resolve(l4p_stream s_, const unsigned long long* zbuf, const unsigned char* colors, const unsigned char* track_colors,
                     const long long* off, int T, int HW, long long n_track, const int* frame, int V, int Ho, int Wo, int bg_r, int bg_g,
                     int bg_b, unsigned char* image, float* depth, int* index) {
    hipStream_t s = (hipStream_t)s_;
    const bool tracks = track_colors && off && n_track > 0;
    if (!zbuf || !colors || !frame || !image || !depth || !index || T < 1 || HW < 1 || n_track < 0 || V < 1 || Ho < 1 || Wo < 1 ||
        (long long)Ho * Wo > 0x7FFFFFFFll || (bg_r | bg_g | bg_b) < 0 || (bg_r | bg_g | bg_b) > 255) {
        l4p_set_error("l4p_view_resolve: bad arguments (T=%d HW=%d n_track=%lld V=%d Ho=%d Wo=%d background %d %d %d)", T, HW, n_track, V,
                      Ho, Wo, bg_r, bg_g, bg_b);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_view_resolve");
    const long long n = (long long)V * Ho * Wo, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(view_resolve_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, zbuf, colors,
                       tracks ? track_colors : nullptr, tracks ? off : nullptr, T, HW, tracks ? n_track : 0, frame, V, (long long)Ho * Wo,
                       (unsigned)bg_r | ((unsigned)bg_g << 8) | ((unsigned)bg_b << 16), image, depth, index);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
