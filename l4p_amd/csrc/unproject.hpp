// Per-pixel unprojection shared by the sampled point maps of the joint aligner (umeyama.hip pointmap_kernel) and the dense 4D
// point clouds (recon4d.hip): generate_point_map, geometry_utils.py:13-53, X = P [depth K^-1 [x, y, 1]^T; 1] for one pixel.
#pragma once
#include <hip/hip_runtime.h>

// k, p: the 4x4 intrinsics and world_T_cam of one frame, element (i, j) at [(i * 4 + j) * ks] (ks = 1: row-major [16];
// ks = T: the b44t layout of frame t).  The upper-left 3x3 of k is inverted by cofactors (general, as torch.inverse is).
__device__ __forceinline__ void unproject_pixel(const float* __restrict__ k, const float* __restrict__ p, int ks, float x, float y,
                                                float z, float& ox, float& oy, float& oz) {
    const float a = k[0], b = k[1 * ks], c = k[2 * ks], d = k[4 * ks], e = k[5 * ks], g = k[6 * ks], h = k[8 * ks], l = k[9 * ks],
                m = k[10 * ks];
    const float det = a * (e * m - g * l) - b * (d * m - g * h) + c * (d * l - e * h);
    const float id = 1.f / det;
    const float i00 = (e * m - g * l) * id, i01 = (c * l - b * m) * id, i02 = (b * g - c * e) * id;
    const float i10 = (g * h - d * m) * id, i11 = (a * m - c * h) * id, i12 = (c * d - a * g) * id;
    const float i20 = (d * l - e * h) * id, i21 = (b * h - a * l) * id, i22 = (a * e - b * d) * id;
    const float cx = (i00 * x + i01 * y + i02) * z, cy = (i10 * x + i11 * y + i12) * z, cz = (i20 * x + i21 * y + i22) * z;
    ox = p[0] * cx + p[1 * ks] * cy + p[2 * ks] * cz + p[3 * ks];
    oy = p[4 * ks] * cx + p[5 * ks] * cy + p[6 * ks] * cz + p[7 * ks];
    oz = p[8 * ks] * cx + p[9 * ks] * cy + p[10 * ks] * cz + p[11 * ks];
}
