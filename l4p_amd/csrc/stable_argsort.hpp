// Shared by recon4d.hip and vis2d.hip (static: each file launches its own copy).
#pragma once
#include "common.hpp"

// -------------------------------------------------------------------------------------------------
// Stable argsort of the N initial y values (torch.argsort(traj[:, :, 1, 0], stable=True); vis.py:722 for the 3D
// trails, vis.py:454 for the 2D track panel): the rank of element
// n is the number of elements that sort before it, ties to the lower index, NaN last.  O(N^2) comparisons spread over N waves
// (the query counts of the demo: 625).
// -------------------------------------------------------------------------------------------------
static __device__ __forceinline__ bool sorts_before(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return (!na && nb) || (na && nb && ia < ib);
    return a < b || (a == b && ia < ib);
}
// one wave per element: the lanes count over strided slices of the N keys (L2-resident), then a butterfly sum
static __global__ __launch_bounds__(256) void recon_argsort_kernel(const float* __restrict__ traj, int N, int T, int* __restrict__ order) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;  // (wave-uniform)
    const float y = traj[((long long)n * 2 + 1) * T];
    int rank = 0;
    for (int j = lane; j < N; j += 64) rank += sorts_before(traj[((long long)j * 2 + 1) * T], j, y, n) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) rank += __shfl_xor(rank, o);
    if (lane == 0) order[rank] = n;
}
