// The output tail of the SAM-style point tracker (reference sparse_heads.py, sam/mask_decoder.py): the hyper-network mask product,
// the gather of the mask up-scaling's partial sums, and the fused (trilinear up-sampling + soft-argmax + spatial means) read-out that
// never materialises the [N,3,16,224,224] logits.  The rest of the tracker's kernels: track.hip.  Which form a launch gets, its grid
// and its LDS size: track_select.hpp (pure, checked on the host by tests/test_track_select_cpu.py).
#include "common.hpp"
#include "launchers.hpp"
#include "track_select.hpp"

// -------------------------------------------------------------------------------------------------
// masks[n][m][vox] = sum_c hyper[n][m][c] * up[n][vox][c]   (mask_decoder.py:139), up channels-last T.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mask_product_kernel(const T* __restrict__ up, const float* __restrict__ hyper,
                                                           float* __restrict__ masks, long long vox, int Cc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* hs = (float*)smem;  // [3][Cc]
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < 3 * Cc; i += 256) hs[i] = hyper[(long long)n * 3 * Cc + i];
    __syncthreads();
    for (long long p = blockIdx.x * 256LL + threadIdx.x; p < vox; p += (long long)gridDim.x * 256) {
        const T* xp = up + ((long long)n * vox + p) * Cc;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int c0 = 0; c0 < Cc; c0 += 8) {
            float x[8];
            Vec8<T>::load(xp + c0, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a0 += x[e] * hs[c0 + e];
                a1 += x[e] * hs[Cc + c0 + e];
                a2 += x[e] * hs[2 * Cc + c0 + e];
            }
        }
        masks[((long long)n * 3 + 0) * vox + p] = a0;
        masks[((long long)n * 3 + 1) * vox + p] = a1;
        masks[((long long)n * 3 + 2) * vox + p] = a2;
    }
}

// LDS-staged form (VT threads, one voxel each; 45 KB of LDS at bf16, three workgroups per CU so one's copy overlaps
// another's arithmetic): the workgroup copies VT voxels x Cc channels (one contiguous span of `up`) into LDS with coalesced
// 16-byte LDS-DMA and each thread then walks its own voxel row from LDS.  The direct form above reads 16 bytes per lane at
// a Cc*sizeof(T) stride (64 distinct lines per load instruction): 1.1 TB/s measured, this one streams.  Same summation order.
template <typename T, int VT>
__global__ __launch_bounds__(VT) void mask_product_lds_kernel(const T* __restrict__ up, const float* __restrict__ hyper,
                                                               float* __restrict__ masks, long long vox, int Cc) {
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* hs = (float*)smem;                 // [3][Cc]
    char* tile = smem + mask_product_tile_off(Cc);  // [VT][Cc] T
    const int n = blockIdx.y, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long p0 = (long long)blockIdx.x * VT;
    const int nvox = (int)(vox - p0 < VT ? vox - p0 : VT);
    const int chunks = nvox * Cc * (int)sizeof(T) / 16;
    const char* src = (const char*)(up + ((long long)n * vox + p0) * Cc);
    for (int c = 0; c < chunks; c += VT)
        if (c + tid < chunks)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + (long long)(c + tid) * 16), (lptr_t)(tile + (c + wave * 64) * 16), 16, 0, 0);
    for (int i = tid; i < 3 * Cc; i += VT) hs[i] = hyper[(long long)n * 3 * Cc + i];
    __syncthreads();
    if (tid < nvox) {
        const T* xp = (const T*)tile + (long long)tid * Cc;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int c0 = 0; c0 < Cc; c0 += 8) {
            float x[8];
            Vec8<T>::load(xp + c0, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a0 += x[e] * hs[c0 + e];
                a1 += x[e] * hs[Cc + c0 + e];
                a2 += x[e] * hs[2 * Cc + c0 + e];
            }
        }
        const long long p = p0 + tid;
        masks[((long long)n * 3 + 0) * vox + p] = a0;
        masks[((long long)n * 3 + 1) * vox + p] = a1;
        masks[((long long)n * 3 + 2) * vox + p] = a2;
    }
}

int launch_mask_product(int dtype, const void* up, const float* hyper, float* masks, int N, long long vox, int Cc,
                        hipStream_t stream) {
    const char* err = "";
    const TrackChoice c = mask_product_select(dtype, N, vox, Cc, &err);
    if (track_refused(c)) return l4p_refuse(err);
    ProfScope prof(PROF_TRACK, stream, "%s", mask_product_form_tag());
    L4P_WITH_T(dtype, T, {
        const bool staged = c.form == MASK_PRODUCT_LDS;
        auto kern = staged ? mask_product_lds_kernel<T, MASK_PRODUCT_VT> : mask_product_kernel<T>;
        static lds_attr_state attr_staged, attr_direct;
        HIP_TRY(lds_attr_once(staged ? attr_staged : attr_direct, kern, (int)c.lds_bytes));
        hipLaunchKernelGGL(kern, grid_of(c), dim3(c.block), c.lds_bytes, stream, (const T*)up, hyper, masks, vox, Cc);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// masks[n][i][t][y][x] = sum over the chunks of tap (y%2, x%2) of the L4P_EPI_MASKDOT partial sums [chunk][i][m] of row
// m = ((n*T + t)*h + y/2)*w + x/2 (see include/l4p_hip.h).  One thread per output voxel, fixed summation order.
__global__ void mask_gather_kernel(const float* __restrict__ partial, float* __restrict__ masks, int N, int T, int h, int w,
                                   int cpt) {
    const int H2 = 2 * h, W2 = 2 * w;
    const long long vox = (long long)T * H2 * W2, total = vox * N, M = (long long)N * T * h * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W2);
        long long r = i / W2;
        const int y = (int)(r % H2);
        r /= H2;
        const int t = (int)(r % T), n = (int)(r / T);
        const long long m = (((long long)n * T + t) * h + (y >> 1)) * w + (x >> 1);
        const int tap = (y & 1) * 2 + (x & 1);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int c = 0; c < cpt; ++c) {
            const float* pp = partial + (long long)(tap * cpt + c) * 3 * M + m;
            a0 += pp[0];
            a1 += pp[M];
            a2 += pp[2 * M];
        }
        const long long p = ((long long)t * H2 + y) * W2 + x;
        masks[((long long)n * 3 + 0) * vox + p] = a0;
        masks[((long long)n * 3 + 1) * vox + p] = a1;
        masks[((long long)n * 3 + 2) * vox + p] = a2;
    }
}

int launch_mask_gather(const float* partial, float* masks, int N, int T, int h, int w, int cpt, hipStream_t stream) {
    const long long total = (long long)N * T * 4 * h * w;
    ProfScope prof(PROF_TRACK, stream, "mask_gather");
    hipLaunchKernelGGL(mask_gather_kernel, dim3(grid1d(total, 16384)), dim3(256), 0, stream, partial, masks, N, T, h, w, cpt);
    HIP_TRY(hipGetLastError());
    return 0;
}

// -------------------------------------------------------------------------------------------------
// Read-out (sparse_heads.py:572-589,645-647) fused: trilinear resize (align_corners=False; identity in
// time when Tl == T) of the low-res logits [N][3][Tl][h][w] to H x W, then per (n, t):
//   channel 0 -> soft-argmax xy over H*W with pixel-centre grid (+0.5);  channel 1 -> spatial mean (vis);
//   channel 2 -> exp(spatial mean) (depth).
// One workgroup per (n, t); the three low-res maps sit in LDS.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void src_idx_nc(int dst, int in, int out, int& i0, int& i1, float& lam) {
    float src = ((float)in / (float)out) * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// The soft-argmax's shift.  Softmax is shift-invariant, so any shift that keeps the exponents non-positive and the sum z of the samples'
// exponentials far from underflow gives the reference's value.  Pass 1 takes max(source): bilinear interpolation is a convex
// combination, so it bounds the up-sampled maximum from ABOVE - but it is attained only where an output sample falls on the source
// maximum.  An isolated peak between the samples of a 4x resize reaches weight 0.875^2 at best (largest exponent -0.234 (peak -
// neighbours)), and a down-sampling grid can skip the source maximum altogether: for peaked logits every exponential underflows, z = 0
// and sx / z is NaN.  With the TRUE up-sampled maximum as the shift the largest sample is exp(0), so z >= 1; with max(source) it is
// z_true * exp(max(up) - max(source)).  z < READOUT_Z_MIN = 2^-64 therefore says that the bound overshot by more than 64 ln 2 = 44.4,
// and the workgroup (z is block-uniform) takes the rare path: one walk for the exact max(lerp2) over the H x W samples, then pass 2
// again with it.  While z >= 2^-64 the largest sample is >= 2^-64 / (H W) >= 2^-94 for H W <= 2^30, and every sample a float sum can still
// see beside it (>= 2^-24 of it, i.e. >= 2^-118) is a normal float above 2^-126: nothing that matters was flushed or denormal, and the
// common path's result stands as it was, bit for bit.  The exact maximum is a max over the same lerp2 values in both kernels (order
// does not matter to a max), so the two forms agree bit for bit on the rare path as well.
constexpr float READOUT_Z_MIN = 0x1p-64f;

// ---- what the two read-out kernels share: the same values in the same sums come from ONE text ----
// the bilinear sample of map b at source rows r0 / r1 (offsets, already times w) and columns x0 / x1
__device__ __forceinline__ float readout_lerp2(const float* b, int r0, int r1, int x0, int x1, float lx, float ly) {
    const float top = (1.f - lx) * b[r0 + x0] + lx * b[r0 + x1];
    const float bot = (1.f - lx) * b[r1 + x0] + lx * b[r1 + x1];
    return (1.f - ly) * top + ly * bot;
}
// wxs[i] / wys[i] = the total weight source column / row i receives from the W / H output positions, accumulated per source index in
// a fixed order (one thread per index, whatever the number of threads nt)
__device__ __forceinline__ void readout_source_weights(float* wxs, float* wys, int h, int w, int H, int W, int tid, int nt) {
    for (int i = tid; i < w + h; i += nt) {
        const bool isx = i < w;
        const int idx = isx ? i : i - w, in = isx ? w : h, out = isx ? W : H;
        float acc = 0.f;
        for (int d = 0; d < out; ++d) {
            int i0, i1;
            float lam;
            src_idx_nc(d, in, out, i0, i1, lam);
            if (i0 == idx) acc += 1.f - lam;
            if (i1 == idx) acc += lam;
        }
        (isx ? wxs : wys)[idx] = acc;
    }
}
// three per-thread values of threads 0 .. 255 (summing: those threads; the 1024-thread form's other waves only read the result) ->
// their workgroup totals in every thread, through red: wave sums, then waves 0 .. 3 in order.  MAX0: the first value is a maximum.
// Block-uniform: every thread reads the same four partial results.
template <bool MAX0>
__device__ __forceinline__ void readout_reduce3(bool summing, int tid, float (*red)[8], float& a, float& b, float& c) {
    if (summing) {
        a = MAX0 ? wave_max(a) : wave_sum(a);
        b = wave_sum(b);
        c = wave_sum(c);
        if ((tid & 63) == 0) {
            red[tid >> 6][0] = a;
            red[tid >> 6][1] = b;
            red[tid >> 6][2] = c;
        }
    }
    __syncthreads();
    a = MAX0 ? fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0])) : red[0][0] + red[1][0] + red[2][0] + red[3][0];
    b = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    c = red[0][2] + red[1][2] + red[2][2] + red[3][2];
}
// pass 1: an upper bound of channel 0 (max(source) >= the up-sampled maximum; not tight, see READOUT_Z_MIN) and the spatial sums of
// the up-sampled channels 1 and 2, all from the 64 x 64 source.  The sum of an up-sampled channel is
// sum_r b[r] * wy[row(r)] * wx[col(r)] with wx / wy of readout_source_weights.  Replaces a second walk over all H x W samples of
// three channels (12 LDS reads + 9 lerps per sample): 171 -> ~90 us per 64-track window.  Thread tid < 256 takes r = tid, tid + 256, ...
__device__ __forceinline__ void readout_pass1(const float* lo, const float* wxs, const float* wys, int hw, int w, bool summing, int tid,
                                              float (*red)[8], float& mx, float& s1, float& s2) {
    mx = -INFINITY, s1 = 0.f, s2 = 0.f;
    if (summing) {
        for (int r = tid; r < hw; r += 256) {
            const float wgt = wys[r / w] * wxs[r % w];
            mx = fmaxf(mx, lo[r]);
            s1 += lo[hw + r] * wgt;
            s2 += lo[2 * hw + r] * wgt;
        }
    }
    readout_reduce3<true>(summing, tid, red, mx, s1, s2);
    __syncthreads();
}
__device__ __forceinline__ void readout_store(float* __restrict__ traj, float* __restrict__ vis, float* __restrict__ depth, int n, int t, int T,
                                              int H, int W, float z, float sx, float sy, float s1, float s2) {
    traj[((long long)n * 2 + 0) * T + t] = sx / z;
    traj[((long long)n * 2 + 1) * T + t] = sy / z;
    vis[(long long)n * T + t] = s1 / (float)(H * W);
    depth[(long long)n * T + t] = expf(s2 / (float)(H * W));
}

// A thread owns output columns x = tid, tid + 256, ... and walks down the rows: its x source indices / weight stay in
// registers and the row's y indices / weight are wave-uniform, so a sample is 4 LDS reads + 3 lerps (the flat-index form
// recomputed two source indices and an integer division per sample and was VALU-bound: 242 us per clip).
__global__ __launch_bounds__(256) void track_readout_kernel(const float* __restrict__ masks, float* __restrict__ traj,
                                                            float* __restrict__ vis, float* __restrict__ depth, int T,
                                                            int h, int w, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lo = (float*)smem;  // [3][h*w]   (track_select.hpp readout_lds_bytes)
    __shared__ float red[4][8];
    const int n = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
    const int hw = h * w;
    for (int i = tid; i < 3 * hw; i += 256) {
        const int m = i / hw, r = i % hw;
        lo[i] = masks[(((long long)n * 3 + m) * T + t) * hw + r];
    }
    __syncthreads();
    float* wxs = lo + 3 * hw;  // [w]
    float* wys = wxs + w;      // [h]
    readout_source_weights(wxs, wys, h, w, H, W, tid, 256);
    __syncthreads();
    float mx, s1, s2;
    readout_pass1(lo, wxs, wys, hw, w, true, tid, red, mx, s1, s2);
    // pass 2: soft-argmax (a second time with the exact maximum when the first sum says that max(source) overshot: READOUT_Z_MIN)
    float z, sx, sy;
    for (int exact = 0;; ++exact) {
        z = 0.f, sx = 0.f, sy = 0.f;
        for (int x = tid; x < W; x += 256) {
            int x0, x1;
            float lx;
            src_idx_nc(x, w, W, x0, x1, lx);
            const float xc = (float)x + 0.5f;
#pragma unroll 2  // (two independent expf chains per trip, the sums in row order as before)
            for (int y = 0; y < H; ++y) {
                int y0, y1;
                float ly;
                src_idx_nc(y, h, H, y0, y1, ly);
                // (expf, not v_exp_f32: the bare instruction is 13 us per launch faster, but its last-ulp differences moved one
                //  re-seeded query of the 4-window full-size bf16 run onto another frame - the track then differs by 7e-2 in depth)
                const float e = expf(readout_lerp2(lo, y0 * w, y1 * w, x0, x1, lx, ly) - mx);
                z += e;
                sx += e * xc;
                sy += e * ((float)y + 0.5f);
            }
        }
        readout_reduce3<false>(true, tid, red, z, sx, sy);
        if (exact || z >= READOUT_Z_MIN) break;  // block-uniform
        __syncthreads();
        float m2 = -INFINITY;
        for (int x = tid; x < W; x += 256) {
            int x0, x1;
            float lx;
            src_idx_nc(x, w, W, x0, x1, lx);
            for (int y = 0; y < H; ++y) {
                int y0, y1;
                float ly;
                src_idx_nc(y, h, H, y0, y1, ly);
                m2 = fmaxf(m2, readout_lerp2(lo, y0 * w, y1 * w, x0, x1, lx, ly));
            }
        }
        m2 = wave_max(m2);
        if ((tid & 63) == 0) red[tid >> 6][0] = m2;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
        __syncthreads();
    }
    if (tid == 0) readout_store(traj, vis, depth, n, t, T, H, W, z, sx, sy, s1, s2);
}

// The same read-out on a 1024-thread workgroup (W <= 256; knob "readout_wide").  In the kernel above a thread owns an output column and
// walks its H rows: H x (bilinear sample + expf) serially per thread on 224 of 256 threads - 58 us per launch whatever the number of
// tracks, one launch per window.  Here the samples exp(logit - max) of RB rows at a time are formed by ALL threads into LDS, and the
// column threads then add them up in the SAME order (row after row: z, sum e x, sum e y per column, then the wave / workgroup sums of
// the kernel above): the same values in the same sums, bit for bit - the sample, the source weights, pass 1, the reductions and the
// final store are the helpers above in both kernels.
__global__ __launch_bounds__(1024) void track_readout_wide_kernel(const float* __restrict__ masks, float* __restrict__ traj,
                                                                  float* __restrict__ vis, float* __restrict__ depth, int T,
                                                                  int h, int w, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lo = (float*)smem;  // [3][h*w]   (track_select.hpp readout_wide_lds_bytes)
    __shared__ float red[4][8];
    const int n = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
    const int hw = h * w;
    float* wxs = lo + 3 * hw;        // [w]
    float* wys = wxs + w;            // [h]
    float* tlx = wys + h;            // [W] x interpolation weight
    float* tly = tlx + W;            // [H]
    int* tx0 = (int*)(tly + H);      // [W] x0 | x1 << 16
    int* ty0 = tx0 + W;              // [H] y0 * w | (y1 * w) << 16
    float* eb = (float*)(ty0 + H);   // [RB][W]
    for (int i = tid; i < 3 * hw; i += 1024) {
        const int m = i / hw, r = i % hw;
        lo[i] = masks[(((long long)n * 3 + m) * T + t) * hw + r];
    }
    for (int i = tid; i < W + H; i += 1024) {
        const bool isx = i < W;
        const int d = isx ? i : i - W;
        int i0, i1;
        float lam;
        src_idx_nc(d, isx ? w : h, isx ? W : H, i0, i1, lam);
        if (isx) {
            tlx[d] = lam;
            tx0[d] = i0 | (i1 << 16);
        } else {
            tly[d] = lam;
            ty0[d] = (i0 * w) | ((i1 * w) << 16);
        }
    }
    __syncthreads();
    readout_source_weights(wxs, wys, h, w, H, W, tid, 1024);
    __syncthreads();
    float mx, s1, s2;
    readout_pass1(lo, wxs, wys, hw, w, tid < 256, tid, red, mx, s1, s2);
    // pass 2: soft-argmax (a second time with the exact maximum when the first sum says that max(source) overshot: READOUT_Z_MIN)
    float z, sx, sy;
    const float xc = (float)tid + 0.5f;
    for (int exact = 0;; ++exact) {
        z = 0.f, sx = 0.f, sy = 0.f;
        for (int yb = 0; yb < H; yb += READOUT_RB) {
            const int rows = H - yb < READOUT_RB ? H - yb : READOUT_RB;
            for (int i = tid; i < rows * W; i += 1024) {
                const int yy = i / W, x = i - yy * W;
                const int px = tx0[x], py = ty0[yb + yy];
                eb[i] = expf(readout_lerp2(lo, py & 0xFFFF, py >> 16, px & 0xFFFF, px >> 16, tlx[x], tly[yb + yy]) - mx);
            }
            __syncthreads();
            if (tid < W) {
#pragma unroll 8  // (eight LDS reads in flight per trip, the sums in row order as before)
                for (int yy = 0; yy < rows; ++yy) {
                    const float e = eb[yy * W + tid];
                    z += e;
                    sx += e * xc;
                    sy += e * ((float)(yb + yy) + 0.5f);
                }
            }
            __syncthreads();
        }
        readout_reduce3<false>(tid < 256, tid, red, z, sx, sy);
        if (exact || z >= READOUT_Z_MIN) break;  // block-uniform
        __syncthreads();
        float m2 = -INFINITY;
        for (int i = tid; i < H * W; i += 1024) {
            const int y = i / W, x = i - y * W;
            const int px = tx0[x], py = ty0[y];
            m2 = fmaxf(m2, readout_lerp2(lo, py & 0xFFFF, py >> 16, px & 0xFFFF, px >> 16, tlx[x], tly[y]));
        }
        m2 = wave_max(m2);
        float* redw = &red[0][0];  // 16 waves: one float each of the 32
        if ((tid & 63) == 0) redw[tid >> 6] = m2;
        __syncthreads();
        mx = -INFINITY;
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, redw[i]);
        __syncthreads();
    }
    if (tid == 0) readout_store(traj, vis, depth, n, t, T, H, W, z, sx, sy, s1, s2);
}

int launch_track_readout(const float* masks, float* traj, float* vis, float* depth, int N, int T, int h, int w, int H,
                         int W, hipStream_t stream) {
    const TrackKnobs knobs = {knob(KNOB_TRACK_DEEP), knob(KNOB_READOUT_WIDE)};
    const char* err = READOUT_ERR_ARGS;
    TrackChoice c = {};
    if (masks && traj && vis && depth) c = track_readout_select(N, T, h, w, H, W, knobs, &err);
    if (c.form == TRACK_FORM_INVALID) return l4p_refuse(err, N, T, h, w, H, W);
    if (c.form == TRACK_FORM_LDS_REFUSED) return l4p_refuse(err, h, w, c.lds_bytes, LDS_DEVICE_LIMIT);
    auto kern = c.form == READOUT_WIDE ? track_readout_wide_kernel : track_readout_kernel;
    static lds_attr_state attr_wide, attr_column;
    HIP_TRY(lds_attr_once(c.form == READOUT_WIDE ? attr_wide : attr_column, kern, (int)c.lds_bytes));
    ProfScope prof(PROF_TRACK, stream, "%s", track_readout_form_tag(c.form));
    hipLaunchKernelGGL(kern, grid_of(c), dim3(c.block), c.lds_bytes, stream, masks, traj, vis, depth, T, h, w, H, W);
    HIP_TRY(hipGetLastError());
    return 0;
}
