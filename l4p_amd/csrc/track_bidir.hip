// Tracking in both time directions (estimation_directions [1, -1]): the recipe the reference states in its own assert
// (sparse_heads.py:242-245: "Run twice, with and without video flipping, and then combine outputs") around its causal
// recursion (sparse_heads.py:306-316: a frame is estimated iff frame centre - query time >= 0).
//   reversed pass : the same recursion on the time-flipped clip; frame f' of it is frame T-1-f' of the input, the query
//                   (tq, x, y) becomes ((float)T - tq, x, y)
//   merge         : output frame g of a track is the forward pass's iff ((float)g + 0.5f) - tq >= 0 (track_prepare_kernel's f32
//                   expression, track.hip), else the reversed pass's at frame T-1-g
// Three memory-bound kernels: the clip flip (the only one that moves real data: 3 T H W floats per clip), the query map with the
// count of queries that own at least one reversed frame (what the caller reads back to skip the reversed pass), the merge.
#include "common.hpp"

// [outer][T][inner] -> the same with the T axis reversed.  blockIdx.y walks the (outer, T) rows, blockIdx.x the row.
template <typename V>
__global__ void time_reverse_kernel(const V* __restrict__ src, V* __restrict__ dst, long long rows, int T, long long inner) {
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const long long o = row / T;
        const int t = (int)(row - o * T);
        const V* s = src + (o * T + (T - 1 - t)) * inner;
        V* d = dst + row * inner;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < inner; i += (long long)gridDim.x * blockDim.x)
            d[i] = s[i];
    }
}

// q_rev = ((float)T - tq, x, y); need_count += #{n : (0.5f - tq) < 0} (one atomic per wave)
__global__ void track_bidir_queries_kernel(const float* __restrict__ q, int T, float* __restrict__ q_rev,
                                           int* __restrict__ need_count, int BN) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    bool need = false;
    if (n < BN) {
        const float tq = q[n * 3];
        q_rev[n * 3] = (float)T - tq;
        q_rev[n * 3 + 1] = q[n * 3 + 1];
        q_rev[n * 3 + 2] = q[n * 3 + 2];
        need = (0.5f - tq) < 0.f;
    }
    const unsigned long long m = __ballot(need);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(need_count, __popcll(m));
}

// one thread per (track, frame).  The outputs may be the forward buffers themselves: a thread reads and writes the same elements of them.
__global__ void track_bidir_merge_kernel(const float* __restrict__ q, const float* traj_f, const float* vis_f, const float* dep_f,
                                         const float* __restrict__ traj_r, const float* __restrict__ vis_r,
                                         const float* __restrict__ dep_r, float* traj, float* vis, float* dep, long long BN, int T,
                                         int mode) {
    const long long total = BN * T;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / T;
        const int g = (int)(i - n * T);
        const bool fwd = (((float)g + 0.5f) - q[n * 3]) >= 0.f;
        const long long x0 = (n * 2 + 0) * T, x1 = (n * 2 + 1) * T;
        if (fwd) {
            const bool have = mode == 0;
            const float v = have ? vis_f[i] : -10.f, d = have ? dep_f[i] : 0.f;
            const float a = have ? traj_f[x0 + g] : 0.f, b = have ? traj_f[x1 + g] : 0.f;
            vis[i] = v;
            dep[i] = d;
            traj[x0 + g] = a;
            traj[x1 + g] = b;
        } else {
            const int r = T - 1 - g;
            vis[i] = vis_r[n * T + r];
            dep[i] = dep_r[n * T + r];
            traj[x0 + g] = traj_r[x0 + r];
            traj[x1 + g] = traj_r[x1 + r];
        }
    }
}

extern "C" {

int l4p_time_reverse(l4p_stream s_, const float* src, float* dst, int outer, int T, long long inner) {
    hipStream_t s = (hipStream_t)s_;
    if (!src || !dst || src == dst || outer < 1 || T < 1 || inner < 1) {
        l4p_set_error("l4p_time_reverse: need src != dst, both non-null, and outer, T, inner >= 1 (outer=%d T=%d inner=%lld)", outer, T,
                      inner);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_ELEMENTWISE, s, "time_reverse");
    const long long rows = (long long)outer * T;
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    const bool wide = inner % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const long long per_row = wide ? inner / 4 : inner, bx = (per_row + 255) / 256;
    const dim3 grid((unsigned)(bx < 1024 ? bx : 1024), gy), block(256);
    if (wide)
        hipLaunchKernelGGL(time_reverse_kernel<f32x4>, grid, block, 0, s, (const f32x4*)src, (f32x4*)dst, rows, T, per_row);
    else
        hipLaunchKernelGGL(time_reverse_kernel<float>, grid, block, 0, s, src, dst, rows, T, per_row);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_track_bidir_queries(l4p_stream s_, const float* q_bn3, int T, float* q_rev_bn3, int* need_count, int BN) {
    hipStream_t s = (hipStream_t)s_;
    if (!q_bn3 || !q_rev_bn3 || !need_count || T < 1 || BN < 1) {
        l4p_set_error("l4p_track_bidir_queries: need every pointer and T, BN >= 1 (T=%d BN=%d)", T, BN);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_TRACK, s, "track_bidir_queries");
    hipLaunchKernelGGL(track_bidir_queries_kernel, dim3((BN + 255) / 256), dim3(256), 0, s, q_bn3, T, q_rev_bn3, need_count, BN);
    HIP_TRY(hipGetLastError());
    return 0;
}

int l4p_track_bidir_merge(l4p_stream s_, const float* q_bn3, const float* traj_f, const float* vis_f, const float* dep_f,
                          const float* traj_r, const float* vis_r, const float* dep_r, float* traj, float* vis, float* dep, int B, int N,
                          int T, int mode) {
    hipStream_t s = (hipStream_t)s_;
    const bool fwd_ok = mode == 1 || (mode == 0 && traj_f && vis_f && dep_f);
    if (!q_bn3 || !fwd_ok || !traj_r || !vis_r || !dep_r || !traj || !vis || !dep || B < 1 || N < 1 || T < 1) {
        l4p_set_error("l4p_track_bidir_merge: need B, N, T >= 1, mode 0 (both passes) or 1 (no forward pass), the queries, the reversed "
                      "pass, the outputs and for mode 0 the forward pass (B=%d N=%d T=%d mode=%d)", B, N, T, mode);
        return L4P_E_INVALID;
    }
    ProfScope prof(PROF_TRACK, s, "track_bidir_merge");
    const long long BN = (long long)B * N, blocks = (BN * T + 255) / 256;
    hipLaunchKernelGGL(track_bidir_merge_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, q_bn3, traj_f, vis_f,
                       dep_f, traj_r, vis_r, dep_r, traj, vis, dep, BN, T, mode);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
