// Moving objects: connected-component labelling of the motion mask over (t, y, x), frames linked through the backward flow, and the
// per-object tables that follow from the labels (DESIGN.md "Moving objects").  Union-find on a parent array with parent[i] <= i and
// atomicMin as the only write after the first: a component's label is its smallest pixel index, so no output depends on the order in
// which edges are processed.  Three passes: a tile-local union-find in LDS, the edges across tile borders and across frames on the
// global array, and a flatten pass in a launch of its own; then a leader scan over the roots numbers the kept components in the
// order of their first pixel (the static map's scan).  Every per-object quantity is an integer sum, a minimum or a maximum (float
// minima and maxima go through an order-preserving integer key): no float is accumulated by atomics.  The rule - include/l4p_hip.h
// states it operation by operation - is f32 and the emitted 3D centre f64, compiled with -ffp-contract=off (Makefile): the tests
// hold every output bit for bit to a numpy restatement (tests/moving_objects_restate.py).
//
// Termination: parent[i] <= i from the first write on and only smaller values are written afterwards, so every find chain descends
// and every union loop ends; each loop still carries a cap of T H W steps and counts in counters.n_guard instead of spinning.
#include "common.hpp"
#include "prof.hpp"

#define OB_TW 64      // tile width: a row of a tile is one wave's contiguous 256-byte read
#define OB_TH 16      // tile height: 256 threads x 4 pixels
#define OB_BLOCK 1024  // pixels per block of the leader scan: 256 threads x 4 chunks, in pixel order
enum { OB_P_FG, OB_P_COMP, OB_P_KEPT, OB_P_KEPTPIX, OB_P_N = 4 };  // columns of a block's partial sums (ws.part)
#define OB_MAX_PIXELS (1ll << 30)
#define OB_MAX_ROWS (1ll << 27)  // K T rows of the per-object tables

struct ObWs {
    int* parent;      // [M]: -1 background, else a pixel of the same component with a smaller or equal index
    int* cnt;         // [M]: at a root, the component's pixels
    int* lastf;       // [M]: at a root, the component's last frame
    unsigned* part;   // [nblk][OB_P_N]
    unsigned* kept_off;  // [nblk]: kept roots in earlier blocks
    unsigned long long* guard;  // [1]: loops that hit their cap
    long long nblk;
    size_t bytes;
};

static ObWs ob_layout(void* ws, long long M) {
    ObWs w;
    w.nblk = (M + OB_BLOCK - 1) / OB_BLOCK;
    auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
    char* p = (char*)ws;
    size_t o = 0;
    w.parent = (int*)(p + o), o += up((size_t)M * 4);
    w.cnt = (int*)(p + o), o += up((size_t)M * 4);
    w.lastf = (int*)(p + o), o += up((size_t)M * 4);
    w.part = (unsigned*)(p + o), o += up((size_t)w.nblk * OB_P_N * 4);
    w.kept_off = (unsigned*)(p + o), o += up((size_t)w.nblk * 4);
    w.guard = (unsigned long long*)(p + o), o += 64;
    w.bytes = o;
    return w;
}

static bool ob_sizes_ok(int T, int H, int W) {
    return T >= 1 && H >= 1 && W >= 1 && (long long)T * H <= OB_MAX_PIXELS && (long long)T * H * W <= OB_MAX_PIXELS;
}

__device__ __forceinline__ bool ob_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// The foreground rule.
__device__ __forceinline__ bool ob_foreground(const float* __restrict__ mask, const float* __restrict__ depth,
                                              const unsigned char* __restrict__ keep, long long m) {
    if (!(mask[m] > 0.f)) return false;  // a NaN logit is not > 0
    if (keep && keep[m] == 0) return false;
    if (depth) {
        const float d = depth[m];
        if (!(ob_finite(d) && d > 0.f)) return false;
    }
    return true;
}

__device__ __forceinline__ bool ob_gate(bool has_depth, float ratio, float da, float db) {
    return !has_depth || ratio <= 0.f || fmaxf(da, db) <= ratio * fminf(da, db);
}

// parent[] is rewritten by other workgroups (global: other CUs and XCDs) while a find runs: the loads are relaxed atomics of the
// scope of the writers, so that no value is served from this CU's L1 or kept in a register across the loop.
template <bool GLOBAL>
__device__ __forceinline__ int ob_load(const int* p) {
    return GLOBAL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool GLOBAL>
__device__ __forceinline__ int ob_find(const int* p, int a, long long cap, bool& gave_up) {
    for (long long n = 0; n < cap; ++n) {
        const int q = ob_load<GLOBAL>(p + a);
        if (q == a) return a;
        a = q;
    }
    gave_up = true;
    return a;
}

// union(a, b): the larger root is hung below the smaller one.  When another thread got to parent[hi] first, atomicMin returns what
// it wrote: that value and lo are in one component and still to be joined.
template <bool GLOBAL>
__device__ __forceinline__ void ob_union(int* p, int a, int b, long long cap, unsigned long long* guard) {
    bool gave_up = false;
    for (long long n = 0; n < cap; ++n) {
        a = ob_find<GLOBAL>(p, a, cap, gave_up);
        b = ob_find<GLOBAL>(p, b, cap, gave_up);
        if (gave_up) break;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(p + hi, lo);
        if (old == hi) return;
        a = old, b = lo;
    }
    atomicAdd(guard, 1ull);
}

// -------------------------------------------------------------------------------------------------
// Tile-local pass: one workgroup, one 64 x 16 tile of one frame; the spatial edges inside the tile in LDS.  The order of the local
// indices is the order of the global ones, so the local root is the tile's smallest pixel of the component.  Writes parent, and
// clears the statistics, of every pixel of the tile.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ob_tile_kernel(const float* __restrict__ mask, const float* __restrict__ depth,
                                                      const unsigned char* __restrict__ keep, int H, int W, int ntx, int nty, int conn8,
                                                      float ratio, int* __restrict__ parent, int* __restrict__ cnt, int* __restrict__ lastf,
                                                      unsigned long long* __restrict__ guard) {
    __shared__ int lp[OB_TW * OB_TH];
    __shared__ float ld[OB_TW * OB_TH];
    const long long b = blockIdx.x;
    const int tx = (int)(b % ntx), ty = (int)((b / ntx) % nty);
    const long long t = b / ((long long)ntx * nty);
    const int x0 = tx * OB_TW, y0 = ty * OB_TH;
    // (a chain has at most 1024 links; a union retries once per foreign write to its root, and the tile's 1024 entries only fall)
    const long long cap = (long long)OB_TW * OB_TH * OB_TW * OB_TH;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 63), y = y0 + (i >> 6);
        const long long m = (t * H + y) * W + x;
        fg[k] = x < W && y < H && ob_foreground(mask, depth, keep, m);
        lp[i] = fg[k] ? i : -1;
        ld[i] = fg[k] && depth ? depth[m] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!fg[k]) continue;
        const int i = threadIdx.x + 256 * k, lx = i & 63, ly = i >> 6;
        const int nb[4] = {lx > 0 ? i - 1 : -1, ly > 0 ? i - 64 : -1, conn8 && lx > 0 && ly > 0 ? i - 65 : -1,
                           conn8 && ly > 0 && lx < 63 ? i - 63 : -1};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = nb[e];
            if (j < 0 || ob_load<false>(lp + j) < 0) continue;
            if (ob_gate(depth != nullptr, ratio, ld[i], ld[j])) ob_union<false>(lp, i, j, cap, guard);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & 63), y = y0 + (i >> 6);
        if (x >= W || y >= H) continue;
        const long long m = (t * H + y) * W + x;
        int root = -1;
        if (fg[k]) {
            bool gave_up = false;
            const int r = ob_find<false>(lp, i, cap, gave_up);
            if (gave_up) atomicAdd(guard, 1ull);
            root = (int)((t * H + y0 + (r >> 6)) * W + x0 + (r & 63));
        }
        parent[m] = root;
        cnt[m] = 0;
        lastf[m] = 0;
    }
}

// -------------------------------------------------------------------------------------------------
// Seam pass, one thread per pixel: its spatial edges that cross a tile border and its temporal edge, joined on the global array.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ob_seam_kernel(const float* __restrict__ depth, const float* __restrict__ flow, int T, int H, int W,
                                                      int conn8, float ratio, int* __restrict__ parent,
                                                      unsigned long long* __restrict__ guard) {
    const long long M = (long long)T * H * W;
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M || ob_load<true>(parent + m) < 0) return;
    const int x = (int)(m % W), y = (int)((m / W) % H), t = (int)(m / ((long long)W * H));
    const bool bx = (x & (OB_TW - 1)) == 0, by = (y & (OB_TH - 1)) == 0, bx1 = (x & (OB_TW - 1)) == OB_TW - 1;
    const bool edge[4] = {x > 0 && bx, y > 0 && by, conn8 && x > 0 && y > 0 && (bx || by), conn8 && y > 0 && x + 1 < W && (bx1 || by)};
    const long long off[4] = {-1, -(long long)W, -(long long)W - 1, -(long long)W + 1};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!edge[e]) continue;
        const long long n = m + off[e];
        if (ob_load<true>(parent + n) < 0) continue;
        if (ob_gate(depth != nullptr, ratio, depth ? depth[m] : 0.f, depth ? depth[n] : 0.f))
            ob_union<true>(parent, (int)m, (int)n, M, guard);
    }
    if (t < 1) return;
    int xq = x, yq = y;
    if (flow) {
        const float u = flow[m], v = flow[M + m];
        if (!(ob_finite(u) && ob_finite(v))) return;
        const float gx = floorf(((float)x + u) + 0.5f), gy = floorf(((float)y + v) + 0.5f);
        if (!(gx >= 0.f && gx < (float)W && gy >= 0.f && gy < (float)H)) return;
        xq = (int)gx, yq = (int)gy;
    }
    const long long n = ((long long)(t - 1) * H + yq) * W + xq;
    if (ob_load<true>(parent + n) >= 0) ob_union<true>(parent, (int)m, (int)n, M, guard);
}

// -------------------------------------------------------------------------------------------------
// Flatten pass (a launch of its own: the launch boundary hands the finished parent array over): label = the root, and the root's
// pixel count and last frame.  A run of consecutive lanes with one label sends its first lane with the run's length.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ob_flatten_kernel(const int* __restrict__ parent, long long M, long long HW, int* __restrict__ label,
                                                         int* __restrict__ cnt, int* __restrict__ lastf,
                                                         unsigned long long* __restrict__ guard) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    int lab = -2;  // a lane past the end: a run of its own
    if (m < M) {
        lab = parent[m];
        if (lab >= 0) {
            bool gave_up = false;
            lab = ob_find<true>(parent, lab, M, gave_up);
            if (gave_up) atomicAdd(guard, 1ull);
        }
        label[m] = lab;
    }
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(lab, 1, 64);
    const bool head = lane == 0 || before != lab;
    const unsigned long long heads = __ballot(head);  // by all lanes, before any leaves
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    if (!head || lab < 0) return;
    const int len = later ? __ffsll((long long)later) : 64 - lane;
    atomicAdd(cnt + lab, len);
    atomicMax(lastf + lab, (int)((m + len - 1) / HW));
}

// -------------------------------------------------------------------------------------------------
// Numbering.  Pixel m is a root when label[m] == m; its component is kept with min_pixels pixels and min_frames frames (frames are
// contiguous: last - first + 1).  ob_partial_kernel adds per block of OB_BLOCK pixels the foreground pixels, the roots, the kept
// roots and their pixels; ob_scan_kernel (one block) turns the kept column into exclusive block offsets and the totals into the
// counters; ob_number_kernel writes object_id at the roots and ob_spread_kernel everywhere else.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ob_kept(const int* __restrict__ cnt, const int* __restrict__ lastf, long long m, long long HW,
                                        int min_pixels, int min_frames) {
    return cnt[m] >= min_pixels && lastf[m] - (int)(m / HW) + 1 >= min_frames;
}

__global__ __launch_bounds__(256) void ob_partial_kernel(const int* __restrict__ label, const int* __restrict__ cnt,
                                                         const int* __restrict__ lastf, long long M, long long HW, int min_pixels,
                                                         int min_frames, unsigned* __restrict__ part) {
    __shared__ unsigned wsum[4][OB_P_N];
    unsigned a[OB_P_N] = {0, 0, 0, 0};
    for (int k = 0; k < OB_BLOCK / 256; ++k) {
        const long long m = (long long)blockIdx.x * OB_BLOCK + k * 256 + threadIdx.x;
        if (m >= M) break;
        const int lab = label[m];
        if (lab < 0) continue;
        a[OB_P_FG] += 1;
        if (lab != m) continue;
        a[OB_P_COMP] += 1;
        if (ob_kept(cnt, lastf, m, HW, min_pixels, min_frames)) a[OB_P_KEPT] += 1, a[OB_P_KEPTPIX] += (unsigned)cnt[m];
    }
#pragma unroll
    for (int k = 0; k < OB_P_N; ++k) {
        unsigned v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < OB_P_N)
        part[(long long)blockIdx.x * OB_P_N + threadIdx.x] =
            wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
}

// counters [6] = n_pixels, n_foreground, n_components, n_kept, n_kept_pixels, n_guard
__global__ __launch_bounds__(1024) void ob_scan_kernel(const unsigned* __restrict__ part, long long nblk, long long M,
                                                       const unsigned long long* __restrict__ guard, unsigned* __restrict__ kept_off,
                                                       unsigned long long* __restrict__ counters) {
    __shared__ unsigned wtot[16][OB_P_N];
    const long long per = (nblk + 1023) / 1024;
    const long long b0 = threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned a[OB_P_N] = {0, 0, 0, 0};
    for (long long b = b0; b < b1; ++b)
        for (int k = 0; k < OB_P_N; ++k) a[k] += part[b * OB_P_N + k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = a[OB_P_KEPT];  // inclusive scan of the kept column inside the wave
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
#pragma unroll
    for (int k = 0; k < OB_P_N; ++k) {
        unsigned v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) wtot[wave][k] = v;
    }
    __syncthreads();
    unsigned run = incl - a[OB_P_KEPT];
    for (int w = 0; w < wave; ++w) run += wtot[w][OB_P_KEPT];
    for (long long b = b0; b < b1; ++b) {
        kept_off[b] = run;
        run += part[b * OB_P_N + OB_P_KEPT];
    }
    if (threadIdx.x == 0) {
        unsigned long long tot[OB_P_N];
        for (int k = 0; k < OB_P_N; ++k) {
            tot[k] = 0;
            for (int w = 0; w < 16; ++w) tot[k] += wtot[w][k];
        }
        counters[0] = (unsigned long long)M, counters[1] = tot[OB_P_FG], counters[2] = tot[OB_P_COMP], counters[3] = tot[OB_P_KEPT];
        counters[4] = tot[OB_P_KEPTPIX], counters[5] = guard[0];
    }
}

__global__ __launch_bounds__(256) void ob_number_kernel(const int* __restrict__ label, const int* __restrict__ cnt,
                                                        const int* __restrict__ lastf, const unsigned* __restrict__ kept_off, long long M,
                                                        long long HW, int min_pixels, int min_frames, int* __restrict__ object_id) {
    __shared__ unsigned wcnt[4];
    unsigned run = kept_off[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < OB_BLOCK / 256; ++k) {
        const long long m = (long long)blockIdx.x * OB_BLOCK + k * 256 + threadIdx.x;
        const bool root = m < M && label[m] == m;
        const bool kept = root && ob_kept(cnt, lastf, m, HW, min_pixels, min_frames);
        const unsigned long long votes = __ballot(kept);
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(votes);
        __syncthreads();
        unsigned idx = run + (unsigned)__popcll(votes & ((1ull << lane) - 1));
        for (int w = 0; w < wave; ++w) idx += wcnt[w];
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
        if (root) object_id[m] = kept ? (int)idx : -1;
    }
}

// (only root entries of object_id are read here and only the others written: a launch after ob_number_kernel)
__global__ __launch_bounds__(256) void ob_spread_kernel(const int* __restrict__ label, long long M, int* __restrict__ object_id) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M) return;
    const int lab = label[m];
    if (lab != m) object_id[m] = lab < 0 ? -1 : object_id[lab];
}

__global__ __launch_bounds__(256) void ob_roots_kernel(const int* __restrict__ label, const int* __restrict__ object_id,
                                                       const int* __restrict__ cnt, const int* __restrict__ lastf, long long M, long long HW,
                                                       long long n_kept, int* __restrict__ root, int* __restrict__ n_pixels,
                                                       int* __restrict__ first_frame, int* __restrict__ last_frame) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M || label[m] != m) return;
    const int k = object_id[m];
    if (k < 0 || k >= n_kept) return;
    root[k] = (int)m, n_pixels[k] = cnt[m], first_frame[k] = (int)(m / HW), last_frame[k] = lastf[m];
}

// -------------------------------------------------------------------------------------------------
// Per-object tables.  One accumulator per (object, frame); float minima and maxima as integers whose order is the floats' order
// (-0 below +0).  A run of consecutive lanes on one (object, frame) is combined by shuffles (a segmented suffix reduction over the
// wave) and its first lane goes to memory: integer sums, minima and maxima, the same table as with one set of atomics per pixel.
// -------------------------------------------------------------------------------------------------
struct ObAcc {
    unsigned long long sx, sy;
    long long s3[3];
    int cnt, n3, x0, y0, x1, y1, lo[3], hi[3];
};
static_assert(sizeof(ObAcc) == 88, "ObAcc layout");

__device__ __forceinline__ int ob_fkey(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float ob_funkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

__global__ __launch_bounds__(256) void ob_acc_clear_kernel(ObAcc* __restrict__ acc, long long rows) {
    const long long r = blockIdx.x * 256ll + threadIdx.x;
    if (r >= rows) return;
    ObAcc e;
    e.sx = e.sy = 0, e.s3[0] = e.s3[1] = e.s3[2] = 0, e.cnt = e.n3 = 0;
    e.x0 = e.y0 = 0x7FFFFFFF, e.x1 = e.y1 = -1;
    for (int a = 0; a < 3; ++a) e.lo[a] = 0x7FFFFFFF, e.hi[a] = (int)0x80000000;
    acc[r] = e;
}

__global__ __launch_bounds__(256) void ob_acc_kernel(const int* __restrict__ object_id, const float* __restrict__ points,
                                                     const float* __restrict__ grid, int T, int H, int W, int K, ObAcc* __restrict__ acc) {
    const long long M = (long long)T * H * W;
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    int row = -1, x = 0, y = 0;
    if (m < M) {
        const int k = object_id[m];
        if (k >= 0 && k < K) {
            x = (int)(m % W), y = (int)((m / W) % H);
            row = k * T + (int)(m / ((long long)W * H));
        }
    }
    const bool live = row >= 0;
    if (__ballot(live) == 0) return;  // a wave off every object (most are): the whole wave leaves together
    unsigned cnt = live ? 1 : 0, n3 = 0;
    unsigned long long sx = (unsigned long long)x, sy = (unsigned long long)y;  // 64 lanes of x < 2^30 do not fit 32 bits
    int x0 = x, x1 = x, y0 = y, y1 = y;
    long long s3[3] = {0, 0, 0};
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    if (live && points) {
        const float v = grid[3];
        const float p[3] = {points[m * 3], points[m * 3 + 1], points[m * 3 + 2]};
        bool ok = v > 0.f && ob_finite(v) && ob_finite(p[0]) && ob_finite(p[1]) && ob_finite(p[2]);
        float s[3] = {0.f, 0.f, 0.f};
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float q = (p[a] - grid[a]) / v;
                s[a] = floorf(q * 256.0f);
                ok = ok && s[a] >= -268435456.f && s[a] < 268435456.f;  // a NaN s fails
            }
        }
        if (ok) {
            n3 = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) s3[a] = (long long)s[a], lo[a] = hi[a] = ob_fkey(p[a]);
        }
    }
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(row, 1, 64);
    const bool head = live && (lane == 0 || before != row);
    const unsigned run = (unsigned)__popcll(__ballot(lane == 0 || before != row) & (~0ull >> (63 - lane)));
    for (int d = 1; d < 64; d <<= 1) {
        const bool same = __shfl_down(run, d, 64) == run && lane + d < 64 && live;
        const unsigned o_cnt = __shfl_down(cnt, d, 64), o_n3 = __shfl_down(n3, d, 64);
        const unsigned long long o_sx = __shfl_down(sx, d, 64), o_sy = __shfl_down(sy, d, 64);
        const int o_x0 = __shfl_down(x0, d, 64), o_x1 = __shfl_down(x1, d, 64), o_y0 = __shfl_down(y0, d, 64), o_y1 = __shfl_down(y1, d, 64);
        if (same) {
            cnt += o_cnt, sx += o_sx, sy += o_sy, n3 += o_n3;
            x0 = min(x0, o_x0), x1 = max(x1, o_x1), y0 = min(y0, o_y0), y1 = max(y1, o_y1);
        }
        if (points) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const long long o_s = __shfl_down(s3[a], d, 64);
                const int o_lo = __shfl_down(lo[a], d, 64), o_hi = __shfl_down(hi[a], d, 64);
                if (same) s3[a] += o_s, lo[a] = min(lo[a], o_lo), hi[a] = max(hi[a], o_hi);
            }
        }
    }
    if (!head) return;
    ObAcc* r = acc + row;
    atomicAdd(&r->sx, sx);
    atomicAdd(&r->sy, sy);
    atomicAdd(&r->cnt, (int)cnt);
    atomicMin(&r->x0, x0), atomicMin(&r->y0, y0), atomicMax(&r->x1, x1), atomicMax(&r->y1, y1);
    if (n3 == 0) return;
    atomicAdd(&r->n3, (int)n3);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicAdd((unsigned long long*)&r->s3[a], (unsigned long long)s3[a]);  // two's complement: the signed sum
        atomicMin(&r->lo[a], lo[a]), atomicMax(&r->hi[a], hi[a]);
    }
}

struct ObTables {
    int *count, *bbox;
    float* centroid_px;
    int* count3d;
    float *centroid_xyz, *box3d, *step, *speed;
};

// the 3D centre of one accumulator, f64, every operation rounded on its own; false (and zeros) without a valid point
__device__ __forceinline__ bool ob_centre(const ObAcc& e, const float* __restrict__ grid, float* c) {
    c[0] = c[1] = c[2] = 0.f;
    if (e.n3 == 0) return false;
    const double n = (double)e.n3, v = (double)grid[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double f = ((double)e.s3[a] + 0.5 * n) / (n * 256.0);
        c[a] = (float)((double)grid[a] + f * v);
    }
    return true;
}

__global__ __launch_bounds__(256) void ob_tables_kernel(const ObAcc* __restrict__ acc, const float* __restrict__ grid, int T, long long rows,
                                                        ObTables o) {
    const long long r = blockIdx.x * 256ll + threadIdx.x;
    if (r >= rows) return;
    const ObAcc e = acc[r];
    const bool any = e.cnt > 0;
    o.count[r] = e.cnt;
    o.bbox[r * 4] = any ? e.x0 : 0, o.bbox[r * 4 + 1] = any ? e.y0 : 0, o.bbox[r * 4 + 2] = any ? e.x1 : -1, o.bbox[r * 4 + 3] = any ? e.y1 : -1;
    o.centroid_px[r * 2] = any ? (float)((double)e.sx / (double)e.cnt) : 0.f;
    o.centroid_px[r * 2 + 1] = any ? (float)((double)e.sy / (double)e.cnt) : 0.f;
    if (!o.count3d) return;
    float c[3], cp[3], d[3] = {0.f, 0.f, 0.f};
    const bool here = ob_centre(e, grid, c);
    o.count3d[r] = e.n3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o.centroid_xyz[r * 3 + a] = c[a];
        o.box3d[r * 6 + a] = here ? ob_funkey(e.lo[a]) : 0.f;
        o.box3d[r * 6 + 3 + a] = here ? ob_funkey(e.hi[a]) : 0.f;
    }
    if (r % T != 0 && here) {
        const ObAcc ep = acc[r - 1];
        if (ob_centre(ep, grid, cp))
            for (int a = 0; a < 3; ++a) d[a] = c[a] - cp[a];
    }
    for (int a = 0; a < 3; ++a) o.step[r * 3 + a] = d[a];
    o.speed[r] = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// -------------------------------------------------------------------------------------------------
// Tracks on objects, one thread per track: the id under the track's pixel per frame, then the id with the most frames (the
// smallest such id).  The vote re-reads the thread's own row of track_object_nt: T^2 loads from L1, no scratch.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ob_tracks_kernel(const int* __restrict__ object_id, const float* __restrict__ traj,
                                                       const float* __restrict__ vis, int N, int T, int H, int W, int* nt,
                                                       int* __restrict__ track_object, int* __restrict__ votes) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    int* row = nt + (long long)n * T;
    for (int t = 0; t < T; ++t) {
        int id = -1;
        const float x = traj[((long long)n * 2) * T + t], y = traj[((long long)n * 2 + 1) * T + t];
        if (vis[(long long)n * T + t] > 0.f && ob_finite(x) && ob_finite(y)) {
            const float gx = floorf(x + 0.5f), gy = floorf(y + 0.5f);
            if (gx >= 0.f && gx < (float)W && gy >= 0.f && gy < (float)H) id = object_id[((long long)t * H + (int)gy) * W + (int)gx];
        }
        row[t] = id;
    }
    int best = -1, best_n = 0;
    for (int t = 0; t < T; ++t) {
        const int id = row[t];
        if (id < 0) continue;
        int c = 0;
        for (int u = 0; u < T; ++u) c += row[u] == id ? 1 : 0;
        if (c > best_n || (c == best_n && id < best)) best = id, best_n = c;
    }
    track_object[n] = best, votes[n] = best_n;
}

__global__ __launch_bounds__(256) void ob_overlay_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ object_id,
                                                         const unsigned char* __restrict__ lut, long long M, int K, int alpha,
                                                         unsigned char* __restrict__ out) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M) return;
    const int k = object_id[m];
    const bool on = k >= 0 && k < K;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = frames[m * 3 + c];
        out[m * 3 + c] = on ? (unsigned char)((v * (256 - alpha) + (int)lut[k * 3 + c] * alpha + 128) >> 8) : (unsigned char)v;
    }
}

static unsigned ob_blocks(long long n) { return (unsigned)((n + 255) / 256); }

extern "C" {

size_t l4p_objects_ws_bytes(int T, int H, int W) {
    if (!ob_sizes_ok(T, H, W)) return 0;
    return ob_layout(nullptr, (long long)T * H * W).bytes;
}

int l4p_objects_label(l4p_stream s_, const float* mask_logit, const float* depth, const float* flow, const unsigned char* keep, int T,
                      int H, int W, int connectivity, float max_depth_ratio, int min_pixels, int min_frames, void* ws, int* label,
                      int* object_id, unsigned long long* counters) {
    hipStream_t s = (hipStream_t)s_;
    if (!ob_sizes_ok(T, H, W) || (connectivity != 4 && connectivity != 8) || min_pixels < 1 || min_frames < 1 || !mask_logit || !ws ||
        !label || !object_id || !counters) {
        l4p_set_error("l4p_objects_label: need T, H, W >= 1, T H W <= 2^30, connectivity 4 or 8, min_pixels, min_frames >= 1 and "
                      "mask_logit, ws, label, object_id, counters (T=%d H=%d W=%d connectivity=%d min_pixels=%d min_frames=%d)", T, H, W,
                      connectivity, min_pixels, min_frames);
        return L4P_E_INVALID;
    }
    const long long HW = (long long)H * W, M = HW * T;
    const ObWs w = ob_layout(ws, M);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_label");
    const int ntx = (W + OB_TW - 1) / OB_TW, nty = (H + OB_TH - 1) / OB_TH, conn8 = connectivity == 8;
    HIP_TRY(hipMemsetAsync(w.guard, 0, 64, s));
    hipLaunchKernelGGL(ob_tile_kernel, dim3((unsigned)((long long)ntx * nty * T)), dim3(256), 0, s, mask_logit, depth, keep, H, W, ntx, nty,
                       conn8, max_depth_ratio, w.parent, w.cnt, w.lastf, w.guard);
    hipLaunchKernelGGL(ob_seam_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, depth, flow, T, H, W, conn8, max_depth_ratio, w.parent, w.guard);
    hipLaunchKernelGGL(ob_flatten_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, w.parent, M, HW, label, w.cnt, w.lastf, w.guard);
    hipLaunchKernelGGL(ob_partial_kernel, dim3((unsigned)w.nblk), dim3(256), 0, s, label, w.cnt, w.lastf, M, HW, min_pixels, min_frames,
                       w.part);
    hipLaunchKernelGGL(ob_scan_kernel, dim3(1), dim3(1024), 0, s, w.part, w.nblk, M, w.guard, w.kept_off, counters);
    hipLaunchKernelGGL(ob_number_kernel, dim3((unsigned)w.nblk), dim3(256), 0, s, label, w.cnt, w.lastf, w.kept_off, M, HW, min_pixels,
                       min_frames, object_id);
    hipLaunchKernelGGL(ob_spread_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, label, M, object_id);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_objects_roots(l4p_stream s_, const void* ws, const int* label, const int* object_id, int T, int H, int W, long long n_kept,
                      int* root, int* n_pixels, int* first_frame, int* last_frame) {
    hipStream_t s = (hipStream_t)s_;
    const long long HW = (long long)H * W, M = HW * T;
    const bool rows = n_kept == 0 || (root && n_pixels && first_frame && last_frame);
    if (!ob_sizes_ok(T, H, W) || n_kept < 0 || n_kept > M || !ws || !label || !object_id || !rows) {
        l4p_set_error("l4p_objects_roots: need the sizes of l4p_objects_label, 0 <= n_kept <= T H W, ws, label, object_id and, with "
                      "n_kept > 0, the four per-object outputs (T=%d H=%d W=%d n_kept=%lld)", T, H, W, n_kept);
        return L4P_E_INVALID;
    }
    if (n_kept == 0) return 0;
    const ObWs w = ob_layout((void*)ws, M);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_roots");
    hipLaunchKernelGGL(ob_roots_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, label, object_id, w.cnt, w.lastf, M, HW, n_kept, root, n_pixels,
                       first_frame, last_frame);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t l4p_objects_tables_ws_bytes(int K, int T) {
    if (K < 1 || T < 1 || (long long)K * T > OB_MAX_ROWS) return 0;
    return (size_t)K * T * sizeof(ObAcc);
}

int l4p_objects_tables(l4p_stream s_, const int* object_id, const float* points, const float* grid, int T, int H, int W, int K, void* ws,
                       int* count, int* bbox, float* centroid_px, int* count3d, float* centroid_xyz, float* box3d, float* step,
                       float* speed) {
    hipStream_t s = (hipStream_t)s_;
    const bool rows2 = K == 0 || (ws && count && bbox && centroid_px);
    const bool rows3 = !points || (grid && (K == 0 || (count3d && centroid_xyz && box3d && step && speed)));
    if (!ob_sizes_ok(T, H, W) || K < 0 || (long long)K * T > OB_MAX_ROWS || !object_id || !rows2 || !rows3) {
        l4p_set_error("l4p_objects_tables: need the sizes of l4p_objects_label, 0 <= K, K T <= 2^27, object_id, with K > 0 ws, count, "
                      "bbox, centroid_px, and with points also grid and the five 3D outputs (T=%d H=%d W=%d K=%d)", T, H, W, K);
        return L4P_E_INVALID;
    }
    if (K == 0) return 0;
    const long long M = (long long)T * H * W, rows = (long long)K * T;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_tables");
    ObAcc* acc = (ObAcc*)ws;
    ObTables o = {count, bbox, centroid_px, points ? count3d : nullptr, centroid_xyz, box3d, step, speed};
    hipLaunchKernelGGL(ob_acc_clear_kernel, dim3(ob_blocks(rows)), dim3(256), 0, s, acc, rows);
    hipLaunchKernelGGL(ob_acc_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, object_id, points, grid, T, H, W, K, acc);
    hipLaunchKernelGGL(ob_tables_kernel, dim3(ob_blocks(rows)), dim3(256), 0, s, acc, grid, T, rows, o);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_objects_tracks(l4p_stream s_, const int* object_id, const float* traj, const float* vis, int N, int T, int H, int W,
                       int* track_object_nt, int* track_object, int* votes) {
    hipStream_t s = (hipStream_t)s_;
    const bool rows = N == 0 || (traj && vis && track_object_nt && track_object && votes);
    if (!ob_sizes_ok(T, H, W) || N < 0 || (long long)N * T > OB_MAX_PIXELS || !object_id || !rows) {
        l4p_set_error("l4p_objects_tracks: need the sizes of l4p_objects_label, 0 <= N, N T <= 2^30, object_id and, with N > 0, traj, "
                      "vis and the three outputs (N=%d T=%d H=%d W=%d)", N, T, H, W);
        return L4P_E_INVALID;
    }
    if (N == 0) return 0;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_tracks");
    hipLaunchKernelGGL(ob_tracks_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, object_id, traj, vis, N, T, H, W, track_object_nt,
                       track_object, votes);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_objects_overlay(l4p_stream s_, const unsigned char* frames, const int* object_id, const unsigned char* lut, int T, int H, int W,
                        int K, int alpha, unsigned char* out) {
    hipStream_t s = (hipStream_t)s_;
    if (!ob_sizes_ok(T, H, W) || K < 0 || alpha < 0 || alpha > 256 || !frames || !object_id || (K > 0 && !lut) || !out) {
        l4p_set_error("l4p_objects_overlay: need the sizes of l4p_objects_label, K >= 0, alpha in [0, 256], frames, object_id, out and, "
                      "with K > 0, lut (T=%d H=%d W=%d K=%d alpha=%d)", T, H, W, K, alpha);
        return L4P_E_INVALID;
    }
    const long long M = (long long)T * H * W;
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_objects_overlay");
    hipLaunchKernelGGL(ob_overlay_kernel, dim3(ob_blocks(M)), dim3(256), 0, s, frames, object_id, lut, M, K, alpha, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
