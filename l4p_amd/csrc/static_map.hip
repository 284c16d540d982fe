// Static scene map: the frame-major world points of a clip fused into one voxel map (DESIGN.md "Static scene map").  A hash
// table on a 63-bit voxel key, open addressing with atomicCAS, one 64-byte slot per voxel.  Every per-voxel quantity is an integer
// (counts, sums of 16-bit in-voxel fractions, colour sums, smallest point index, frame marks), so the map does not depend on the
// order in which points arrive; the slot a voxel lands in does, and never leaves this file: voxels are emitted in the order of
// their first point (a leader scan over the points, no sort).  The point rule - include/l4p_hip.h states it operation by operation
// - is f32 and the emitted position f64, compiled with -ffp-contract=off (Makefile): the tests hold every output bit for bit to a
// numpy restatement (tests/static_map_restate.py).
#include "common.hpp"
#include "prof.hpp"

#define SM_EMPTY 0xFFFFFFFFFFFFFFFFull
#define SM_BLOCK 1024  // points per block of the leader scan: 256 threads x 4 chunks, in point order
// what ws.slot_of[m] holds instead of a slot index for a point that is in no voxel
enum : unsigned { SM_OVERFLOW = 0xFFFFFFFCu, SM_RANGE = 0xFFFFFFFDu, SM_MASKED = 0xFFFFFFFEu, SM_NONFINITE = 0xFFFFFFFFu };
// columns of a block's partial sums (ws.part)
enum { SM_P_LEAD, SM_P_KEPT, SM_P_USED, SM_P_NONFINITE, SM_P_MASKED, SM_P_RANGE, SM_P_OVERFLOW, SM_P_N = 8 };

// One voxel.  cnt_r = count | sum_red << 32 and g_b = sum_green | sum_blue << 32: two 32-bit sums per 64-bit atomic add (no carry
// crosses while T HW <= 2^24: 255 * 2^24 < 2^32).  last_frame1 = last frame + 1, 0 while empty.  out_idx: written by the voxel's
// leader, 0 / -1 (kept / filtered) by l4p_static_map_count, then the output index by l4p_static_map_emit.
struct SmSlot {
    unsigned long long key, sum_f[3], cnt_r, g_b;
    unsigned first_point, last_frame1, n_frames;
    int out_idx;
};
static_assert(sizeof(SmSlot) == 64, "one slot = half a 128-byte line");

struct SmWs {
    SmSlot* slots;      // [capacity]
    unsigned* slot_of;  // [M]: the point's slot, or one of the codes above
    unsigned* part;     // [nblk][SM_P_N]
    unsigned* kept_off; // [nblk]: kept voxels whose leader lies in an earlier block
    long long nblk;
    size_t bytes;
};

static SmWs sm_layout(void* ws, long long capacity, long long M) {
    SmWs w;
    w.nblk = (M + SM_BLOCK - 1) / SM_BLOCK;
    auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
    char* p = (char*)ws;
    size_t o = 0;
    w.slots = (SmSlot*)(p + o), o += (size_t)capacity * sizeof(SmSlot);
    w.slot_of = (unsigned*)(p + o), o += up((size_t)M * 4);
    w.part = (unsigned*)(p + o), o += up((size_t)w.nblk * SM_P_N * 4);
    w.kept_off = (unsigned*)(p + o), o += up((size_t)w.nblk * 4);
    w.bytes = o;
    return w;
}

static bool sm_sizes_ok(int T, int HW, long long capacity) {
    return T >= 1 && HW >= 1 && (long long)T * HW <= (1ll << 24) && capacity >= 1 && capacity <= (1ll << 30) &&
           (capacity & (capacity - 1)) == 0;
}

__device__ __forceinline__ bool sm_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// The point rule.  Returns 0 and the key / the three in-voxel fractions, or the code of the reason the point is dropped.
__device__ __forceinline__ unsigned sm_point(float x, float y, float z, bool masked, const float* __restrict__ grid,
                                             unsigned long long& key, unsigned* f) {
    if (!(sm_finite(x) && sm_finite(y) && sm_finite(z))) return SM_NONFINITE;
    if (masked) return SM_MASKED;
    const float v = grid[3];
    if (!(v > 0.f && sm_finite(v))) return SM_RANGE;  // no grid: nothing is inside it
    const float p[3] = {x, y, z};
    key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = (p[a] - grid[a]) / v;
        const float i = floorf(q);
        if (!(i >= -1048576.f && i <= 1048575.f)) return SM_RANGE;  // a NaN or infinite q (a non-finite origin) as well
        f[a] = (unsigned)(int)floorf((q - i) * 65536.0f);
        key |= (unsigned long long)((int)i + (1 << 20)) << (21 * a);
    }
    return 0;
}

__global__ __launch_bounds__(256) void sm_clear_kernel(SmSlot* __restrict__ slots, long long capacity) {
    for (long long s = blockIdx.x * 256ll + threadIdx.x; s < capacity; s += (long long)gridDim.x * 256) {
        SmSlot e;
        e.key = SM_EMPTY, e.sum_f[0] = e.sum_f[1] = e.sum_f[2] = 0, e.cnt_r = 0, e.g_b = 0;
        e.first_point = 0xFFFFFFFFu, e.last_frame1 = 0, e.n_frames = 0, e.out_idx = -1;
        slots[s] = e;
    }
}

// -------------------------------------------------------------------------------------------------
// Insert, one launch over all points: the probe, then the point's sums and the smallest point index.  The probe loop runs at
// most `capacity` steps: a full table marks the point SM_OVERFLOW.  A relaxed load in front of the CAS and of the minimum saves
// the atomic where it cannot change anything; a stale load only costs that atomic (keys never change once set, first_point only
// falls).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_insert_kernel(const float* __restrict__ points, const unsigned char* __restrict__ colors,
                                                        const float* __restrict__ mask, const unsigned char* __restrict__ keep,
                                                        const float* __restrict__ grid, long long M, unsigned long long cmask,
                                                        SmSlot* __restrict__ slots, unsigned* __restrict__ slot_of) {
    const long long pt = blockIdx.x * 256ll + threadIdx.x;
    const bool inb = pt < M;
    const long long m = inb ? pt : 0;
    unsigned long long key;
    unsigned f[3] = {0, 0, 0};
    unsigned res = SM_NONFINITE;
    if (inb) {
        const bool masked = (mask && mask[m] > 0.f) || (keep && keep[m] == 0);  // a NaN logit is not > 0
        res = sm_point(points[m * 3], points[m * 3 + 1], points[m * 3 + 2], masked, grid, key, f);
    }
    if (res == 0) {
        unsigned long long h = key;  // murmur3's 64-bit finaliser
        h ^= h >> 33, h *= 0xff51afd7ed558ccdull, h ^= h >> 33, h *= 0xc4ceb9fe1a85ec53ull, h ^= h >> 33;
        unsigned long long s = h & cmask;
        res = SM_OVERFLOW;
        for (unsigned long long n = 0; n <= cmask; ++n) {
            unsigned long long cur = __atomic_load_n(&slots[s].key, __ATOMIC_RELAXED);
            if (cur == SM_EMPTY) {
                cur = atomicCAS(&slots[s].key, SM_EMPTY, key);
                if (cur == SM_EMPTY) cur = key;  // this thread claimed the slot
            }
            if (cur == key) {
                res = (unsigned)s;
                break;
            }
            s = (s + 1) & cmask;
        }
    }
    if (inb) slot_of[m] = res;
    const bool live = res < SM_OVERFLOW;
    // what the point adds to its voxel: the three fractions, one point, the three colour bytes
    unsigned a[7] = {f[0], f[1], f[2], 1, 0, 0, 0};
    if (live) a[4] = colors[m * 3], a[5] = colors[m * 3 + 1], a[6] = colors[m * 3 + 2];
    // Neighbouring pixels often share a voxel: a run of consecutive lanes with one slot is summed by shuffles first (a segmented
    // suffix sum over the wave) and only the run's first lane, which holds the run's smallest m, goes to memory.  Integer sums:
    // the same table as with one set of atomics per point, which measured slower (insert 1271 against 1073 us at 64 x 224 x 224,
    // DESIGN.md).
    const int lane = threadIdx.x & 63;
    const unsigned before = __shfl_up(res, 1, 64);
    const bool head = live && (lane == 0 || before != res);
    const unsigned run = (unsigned)__popcll(__ballot(head) & (~0ull >> (63 - lane)));
    if (!live)  // a lane without a voxel sits inside the run in front of it and must add nothing to it
        for (int k = 0; k < 7; ++k) a[k] = 0;
    for (int d = 1; d < 64; d <<= 1) {
        const bool same = __shfl_down(run, d, 64) == run && lane + d < 64;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const unsigned o = __shfl_down(a[k], d, 64);
            if (same && live) a[k] += o;
        }
    }
    if (!head) return;
    SmSlot* sl = slots + res;
    atomicAdd(&sl->sum_f[0], (unsigned long long)a[0]);
    atomicAdd(&sl->sum_f[1], (unsigned long long)a[1]);
    atomicAdd(&sl->sum_f[2], (unsigned long long)a[2]);
    atomicAdd(&sl->cnt_r, (unsigned long long)a[3] | (unsigned long long)a[4] << 32);
    atomicAdd(&sl->g_b, (unsigned long long)a[5] | (unsigned long long)a[6] << 32);
    if ((unsigned)m < __atomic_load_n(&sl->first_point, __ATOMIC_RELAXED)) atomicMin(&sl->first_point, (unsigned)m);
}

// -------------------------------------------------------------------------------------------------
// Frame marks, one launch per frame t in stream order: the marks of the frames before t are in the table when this one starts,
// so the thread whose atomicMax(last_frame1, t + 1) returns less than t + 1 is the only one of frame t to see the voxel without
// its frame, and counts the frame.  A run of lanes with one slot sends its first lane; the relaxed load in front saves the atomic
// once the frame is marked (last_frame1 only rises: a stale load only costs that atomic).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_frame_kernel(const unsigned* __restrict__ slot_of, int t, int HW, SmSlot* __restrict__ slots) {
    const long long pix = blockIdx.x * 256ll + threadIdx.x;
    const unsigned res = pix < HW ? slot_of[(long long)t * HW + pix] : SM_NONFINITE;
    const unsigned before = __shfl_up(res, 1, 64);
    if (res >= SM_OVERFLOW || ((threadIdx.x & 63) != 0 && before == res)) return;
    SmSlot* sl = slots + res;
    const unsigned t1 = (unsigned)t + 1;
    if (__atomic_load_n(&sl->last_frame1, __ATOMIC_RELAXED) < t1 && atomicMax(&sl->last_frame1, t1) < t1) atomicAdd(&sl->n_frames, 1u);
}

// -------------------------------------------------------------------------------------------------
// Leader scan.  Point m leads its voxel when m is the voxel's first_point; the voxel is kept when it has min_frames frames and
// min_points points.  Pass 1 (sm_partial_kernel) marks every voxel kept or filtered through its leader and adds, per block of
// SM_BLOCK points, the leaders, the kept leaders and the points per drop reason; pass 2 (sm_scan_kernel, one block) turns the kept
// column into exclusive block offsets and the column totals into the eight counters.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_partial_kernel(SmSlot* __restrict__ slots, const unsigned* __restrict__ slot_of, long long M,
                                                         unsigned min_frames, unsigned min_points, unsigned* __restrict__ part) {
    __shared__ unsigned wsum[4][SM_P_N];
    unsigned a[SM_P_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < SM_BLOCK / 256; ++k) {
        const long long m = (long long)blockIdx.x * SM_BLOCK + k * 256 + threadIdx.x;
        if (m >= M) break;
        const unsigned code = slot_of[m];
        if (code < SM_OVERFLOW) {
            SmSlot* sl = slots + code;
            a[SM_P_USED] += 1;
            if (sl->first_point == (unsigned)m) {
                const bool kept = sl->n_frames >= min_frames && (unsigned)(sl->cnt_r & 0xFFFFFFFFull) >= min_points;
                sl->out_idx = kept ? 0 : -1;
                a[SM_P_LEAD] += 1;
                a[SM_P_KEPT] += kept ? 1 : 0;
            }
        } else if (code == SM_OVERFLOW) {
            a[SM_P_USED] += 1;  // the point has a key; the table had no room for it
            a[SM_P_OVERFLOW] += 1;
        } else {
            a[code == SM_NONFINITE ? SM_P_NONFINITE : (code == SM_MASKED ? SM_P_MASKED : SM_P_RANGE)] += 1;
        }
    }
#pragma unroll
    for (int k = 0; k < SM_P_N; ++k) {
        unsigned v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < SM_P_N)
        part[(long long)blockIdx.x * SM_P_N + threadIdx.x] =
            wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
}

// counters [8] = n_points, n_used, n_nonfinite, n_masked, n_out_of_range, n_voxels, n_kept, n_overflow
__global__ __launch_bounds__(1024) void sm_scan_kernel(const unsigned* __restrict__ part, long long nblk, long long M,
                                                       unsigned* __restrict__ kept_off, unsigned long long* __restrict__ counters) {
    __shared__ unsigned wtot[16][SM_P_N];
    const long long per = (nblk + 1023) / 1024;
    const long long b0 = threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned a[SM_P_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long b = b0; b < b1; ++b)
        for (int k = 0; k < SM_P_N; ++k) a[k] += part[b * SM_P_N + k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = a[SM_P_KEPT];  // inclusive scan of the kept column inside the wave
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
#pragma unroll
    for (int k = 0; k < SM_P_N; ++k) {
        unsigned v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) wtot[wave][k] = v;
    }
    __syncthreads();
    unsigned run = incl - a[SM_P_KEPT];
    for (int w = 0; w < wave; ++w) run += wtot[w][SM_P_KEPT];
    for (long long b = b0; b < b1; ++b) {
        kept_off[b] = run;
        run += part[b * SM_P_N + SM_P_KEPT];
    }
    if (threadIdx.x == 0) {
        unsigned long long tot[SM_P_N];
        for (int k = 0; k < SM_P_N; ++k) {
            tot[k] = 0;
            for (int w = 0; w < 16; ++w) tot[k] += wtot[w][k];
        }
        counters[0] = (unsigned long long)M, counters[1] = tot[SM_P_USED], counters[2] = tot[SM_P_NONFINITE];
        counters[3] = tot[SM_P_MASKED], counters[4] = tot[SM_P_RANGE], counters[5] = tot[SM_P_LEAD];
        counters[6] = tot[SM_P_KEPT], counters[7] = tot[SM_P_OVERFLOW];
    }
}

struct SmOut {
    float* xyz;
    unsigned char* rgb;
    int *count, *n_frames, *first_frame, *last_frame, *first_point;
    long long* key;
};

// Emit: the leader of kept voxel number idx (kept leaders counted in point order) writes row idx of every output and leaves idx in
// its slot for sm_voxel_id_kernel.  f64 position, every operation rounded on its own; colour rounded half up in integers.
__global__ __launch_bounds__(256) void sm_emit_kernel(SmSlot* __restrict__ slots, const unsigned* __restrict__ slot_of,
                                                      const unsigned* __restrict__ kept_off, const float* __restrict__ grid, long long M,
                                                      int HW, long long n_kept, SmOut o) {
    __shared__ unsigned wcnt[4];
    unsigned run = kept_off[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < SM_BLOCK / 256; ++k) {
        const long long m = (long long)blockIdx.x * SM_BLOCK + k * 256 + threadIdx.x;
        SmSlot* sl = nullptr;
        bool kept = false;
        if (m < M) {
            const unsigned code = slot_of[m];
            if (code < SM_OVERFLOW && slots[code].first_point == (unsigned)m) {
                sl = slots + code;
                kept = sl->out_idx >= 0;
            }
        }
        const unsigned long long votes = __ballot(kept);
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(votes);
        __syncthreads();
        unsigned idx = run + (unsigned)__popcll(votes & ((1ull << lane) - 1));
        for (int w = 0; w < wave; ++w) idx += wcnt[w];
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
        if (kept && (long long)idx < n_kept) {
            const unsigned long long key = sl->key;
            const unsigned cnt = (unsigned)(sl->cnt_r & 0xFFFFFFFFull);
            const unsigned long long rgb[3] = {sl->cnt_r >> 32, sl->g_b & 0xFFFFFFFFull, sl->g_b >> 32};
            const double c = (double)cnt, v = (double)grid[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int i = (int)((key >> (21 * a)) & 0x1FFFFFull) - (1 << 20);
                const double fr = ((double)sl->sum_f[a] + 0.5 * c) / (c * 65536.0);
                o.xyz[(long long)idx * 3 + a] = (float)((double)grid[a] + ((double)i + fr) * v);
                o.rgb[(long long)idx * 3 + a] = (unsigned char)((2 * rgb[a] + cnt) / (2ull * cnt));
            }
            o.count[idx] = (int)cnt, o.n_frames[idx] = (int)sl->n_frames;
            o.first_frame[idx] = (int)(m / HW), o.last_frame[idx] = (int)sl->last_frame1 - 1, o.first_point[idx] = (int)m;
            o.key[idx] = (long long)key;
            sl->out_idx = (int)idx;
        }
    }
}

__global__ __launch_bounds__(256) void sm_voxel_id_kernel(const SmSlot* __restrict__ slots, const unsigned* __restrict__ slot_of, long long M,
                                                          int* __restrict__ voxel_id) {
    const long long m = blockIdx.x * 256ll + threadIdx.x;
    if (m >= M) return;
    const unsigned code = slot_of[m];
    voxel_id[m] = code < SM_OVERFLOW ? slots[code].out_idx : -1;
}

extern "C" {

size_t l4p_static_map_ws_bytes(long long capacity, long long M) {
    if (M < 1 || M > (1ll << 24) || !sm_sizes_ok(1, 1, capacity)) return 0;
    return sm_layout(nullptr, capacity, M).bytes;
}

int l4p_static_map_insert(l4p_stream s_, const float* points, const unsigned char* colors, const float* mask_logit,
                          const unsigned char* keep, const float* grid, int T, int HW, long long capacity, void* ws) {
    hipStream_t s = (hipStream_t)s_;
    if (!sm_sizes_ok(T, HW, capacity) || !points || !colors || !grid || !ws) {
        l4p_set_error("l4p_static_map_insert: need T, HW >= 1, T HW <= 2^24, a power-of-two capacity in [1, 2^30] and points, colors, "
                      "grid, ws (T=%d HW=%d capacity=%lld)", T, HW, capacity);
        return L4P_E_INVALID;
    }
    const SmWs w = sm_layout(ws, capacity, (long long)T * HW);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_static_map_insert");
    const long long cb = (capacity + 255) / 256;
    hipLaunchKernelGGL(sm_clear_kernel, dim3((unsigned)(cb < 8192 ? cb : 8192)), dim3(256), 0, s, w.slots, capacity);
    const long long M = (long long)T * HW;
    hipLaunchKernelGGL(sm_insert_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, points, colors, mask_logit, keep, grid, M,
                       (unsigned long long)(capacity - 1), w.slots, w.slot_of);
    for (int t = 0; t < T; ++t)
        hipLaunchKernelGGL(sm_frame_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, w.slot_of, t, HW, w.slots);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_static_map_count(l4p_stream s_, void* ws, int T, int HW, long long capacity, int min_frames, int min_points,
                         unsigned long long* counters) {
    hipStream_t s = (hipStream_t)s_;
    if (!sm_sizes_ok(T, HW, capacity) || min_frames < 1 || min_points < 1 || !ws || !counters) {
        l4p_set_error("l4p_static_map_count: need the sizes of l4p_static_map_insert, min_frames, min_points >= 1 and ws, counters "
                      "(T=%d HW=%d capacity=%lld min_frames=%d min_points=%d)", T, HW, capacity, min_frames, min_points);
        return L4P_E_INVALID;
    }
    const long long M = (long long)T * HW;
    const SmWs w = sm_layout(ws, capacity, M);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_static_map_count");
    hipLaunchKernelGGL(sm_partial_kernel, dim3((unsigned)w.nblk), dim3(256), 0, s, w.slots, w.slot_of, M, (unsigned)min_frames,
                       (unsigned)min_points, w.part);
    hipLaunchKernelGGL(sm_scan_kernel, dim3(1), dim3(1024), 0, s, w.part, w.nblk, M, w.kept_off, counters);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_static_map_emit(l4p_stream s_, void* ws, const float* grid, int T, int HW, long long capacity, long long n_kept, float* xyz,
                        unsigned char* rgb, int* count, int* n_frames, int* first_frame, int* last_frame, int* first_point,
                        long long* key, int* voxel_id) {
    hipStream_t s = (hipStream_t)s_;
    const long long M = (long long)T * HW;
    const bool rows = n_kept == 0 || (xyz && rgb && count && n_frames && first_frame && last_frame && first_point && key);
    if (!sm_sizes_ok(T, HW, capacity) || n_kept < 0 || n_kept > M || !ws || !grid || !voxel_id || !rows) {
        l4p_set_error("l4p_static_map_emit: need the sizes of l4p_static_map_insert, 0 <= n_kept <= T HW, ws, grid, voxel_id and, "
                      "with n_kept > 0, the eight per-voxel outputs (T=%d HW=%d capacity=%lld n_kept=%lld)", T, HW, capacity, n_kept);
        return L4P_E_INVALID;
    }
    const SmWs w = sm_layout(ws, capacity, M);
    ProfScope prof(PROF_ELEMENTWISE, s, "l4p_static_map_emit");
    const SmOut o = {xyz, rgb, count, n_frames, first_frame, last_frame, first_point, key};
    hipLaunchKernelGGL(sm_emit_kernel, dim3((unsigned)w.nblk), dim3(256), 0, s, w.slots, w.slot_of, w.kept_off, grid, M, HW, n_kept, o);
    hipLaunchKernelGGL(sm_voxel_id_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, w.slots, w.slot_of, M, voxel_id);
    HIP_TRY(hipGetLastError());
    return 0;
}
}
