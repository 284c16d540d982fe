"""Numpy restatement of the free-viewpoint renderer's three rules (include/l4p_hip.h: l4p_view_splat, l4p_view_mesh,
l4p_view_resolve; csrc/view4d.hip), used by tests/test_view4d_cpu.py and tests/test_view4d_gpu.py.

``dtype`` switches the arithmetic: np.float32 is the rule itself (numpy rounds every array operation in f32, in the order written,
so the kernels are held to it bit for bit), np.float64 is the same rule on the same f32 inputs without the f32 rounding (how far the
rounding moves the picture).  The depth test is restated as (z, low word) compared lexicographically, which for f32 is the
kernels' 64-bit key order: a positive f32 orders as its bit pattern."""
from __future__ import annotations

import numpy as np

from l4p_amd.utils.recon4d import FRUSTUM_TRIANGLES
from l4p_amd.utils.view4d import MESH_BIT, mesh_colours

EMPTY_LOW = np.int64(2 ** 62)  # the low word of an empty pixel: above every point index and triangle code


class ZBuffer:
    """One view: z [Ho, Wo] (dtype, +inf where empty) and the winner's low word [Ho, Wo] int64."""

    def __init__(self, Ho, Wo, dtype):
        self.z = np.full((Ho, Wo), np.inf, dtype=dtype)
        self.low = np.full((Ho, Wo), EMPTY_LOW, dtype=np.int64)
        self.writes = 0  # pixel writes offered to the depth test

    def put(self, ys, xs, z, low):
        """Offer (z, low) to the pixels [ys, xs] (slices, or index arrays of distinct pixels); z scalar or array."""
        zc, lc = self.z[ys, xs], self.low[ys, xs]
        win = (z < zc) | ((z == zc) & (low < lc))
        self.writes += int(np.size(win))
        self.z[ys, xs] = np.where(win, z, zc)
        self.low[ys, xs] = np.where(win, low, lc)


def project(P, M, K, near, dtype):
    """Rule steps 1-4 for points P [n, 3] under the view matrix M [4, 4] and K = (fx, fy, cx, cy): (u, v, z, ok)."""
    dt = dtype
    P, M = np.asarray(P, dtype=np.float32).astype(dt).reshape(-1, 3), np.asarray(M, dtype=np.float32).astype(dt)
    fx, fy, cx, cy = (dt(np.float32(k)) for k in K)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        x = ((M[0, 0] * X + M[0, 1] * Y) + M[0, 2] * Z) + M[0, 3]
        y = ((M[1, 0] * X + M[1, 1] * Y) + M[1, 2] * Z) + M[1, 3]
        z = ((M[2, 0] * X + M[2, 1] * Y) + M[2, 2] * Z) + M[2, 3]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(z < dt(np.float32(near)))
        u = (fx * x) / z + cx
        v = (fy * y) / z + cy
        ok &= (np.abs(u) < dt(2 ** 20)) & (np.abs(v) < dt(2 ** 20))
    assert x.dtype == dt and u.dtype == dt
    return u, v, z, ok


def splat(zb: ZBuffer, P, M, K, point_size, max_half, near, dtype):
    """Rule steps 1-8 for the points P [n, 3] of one view (local index = row)."""
    dt = dtype
    Ho, Wo = zb.z.shape
    u, v, z, ok = project(P, M, K, near, dt)
    fx = dt(np.float32(K[0]))
    with np.errstate(all="ignore"):
        px, py = np.floor(u + dt(0.5)), np.floor(v + dt(0.5))
        r = ((dt(np.float32(point_size)) * fx) / z) * dt(0.5)
        m = dt(max_half)
        h = np.floor(np.where(r < m, r, m))
        ok &= h >= 0
    assert r.dtype == dt
    for i in np.nonzero(ok)[0]:
        a, b, hh = int(px[i]), int(py[i]), int(h[i])
        x0, x1, y0, y1 = max(a - hh, 0), min(a + hh, Wo - 1), max(b - hh, 0), min(b + hh, Ho - 1)
        if x0 > x1 or y0 > y1:
            continue
        zb.put(slice(y0, y1 + 1), slice(x0, x1 + 1), z[i], np.int64(i))


def _edge(ua, va, ub, vb, px, py):
    return (ub - ua) * (py - va) - (vb - va) * (px - ua)


def drawn_frusta(t: int, stride: int):
    """The frames whose frustum a view of frame t draws: t, and with stride >= 1 every earlier multiple of the stride."""
    return [f for f in range(t + 1) if f == t or (stride >= 1 and f % stride == 0)]


def mesh(zb: ZBuffer, frustum, t, stride, M, K, near, dtype):
    """The triangle rule for one view of frame t: frustum [T, 8, 3]."""
    dt = dtype
    Ho, Wo = zb.z.shape
    for f in drawn_frusta(t, stride):
        for tri in range(12):
            u, v, z, ok = project(frustum[f][FRUSTUM_TRIANGLES[tri]], M, K, near, dt)
            if not ok.all():
                continue
            A = _edge(u[0], v[0], u[1], v[1], u[2], v[2])
            if not (A != 0 and np.isfinite(A)):
                continue
            x0, x1 = max(int(np.ceil(u.min())), 0), min(int(np.floor(u.max())), Wo - 1)
            y0, y1 = max(int(np.ceil(v.min())), 0), min(int(np.floor(v.max())), Ho - 1)
            if x0 > x1 or y0 > y1:
                continue
            yy, xx = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
            px, py = xx.astype(dt), yy.astype(dt)
            with np.errstate(all="ignore"):
                b0 = _edge(u[1], v[1], u[2], v[2], px, py) / A
                b1 = _edge(u[2], v[2], u[0], v[0], px, py) / A
                b2 = _edge(u[0], v[0], u[1], v[1], px, py) / A
                zp = dt(1) / ((b0 / z[0] + b1 / z[1]) + b2 / z[2])
                keep = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & np.isfinite(zp) & ~(zp < dt(np.float32(near)))
            assert zp.dtype == dt
            if keep.any():
                zb.put(yy[keep], xx[keep], zp[keep], np.int64(MESH_BIT | (f << 4) | tri))


def resolve(zb: ZBuffer, colors, track_colors, hw, background):
    """image [Ho, Wo, 3] uint8, depth [Ho, Wo] (the buffer's dtype), index [Ho, Wo] int32 of one view: colors [hw, 3] of the frame's
    dense points, track_colors [n, 3] of its trail points (or None)."""
    low = zb.low
    empty, tri = low == EMPTY_LOW, (low >= MESH_BIT) & (low != EMPTY_LOW)
    point = ~empty & ~tri
    image = np.empty(low.shape + (3,), dtype=np.uint8)
    image[empty] = np.asarray(background, dtype=np.uint8)
    image[tri] = mesh_colours()[low[tri] & 15]
    allc = colors if track_colors is None else np.concatenate([colors, track_colors])
    image[point] = allc[low[point]]
    index = np.where(empty, np.int64(0xFFFFFFFF), low).astype(np.uint32).view(np.int32)  # -1 where empty, triangles negative
    return image, zb.z.copy(), index


def render(rec, T, hw, cam_T_world, intrinsics, size, frames, point_size=0.02, max_half=16, near=1e-3, background=(0, 0, 0),
           tracks=True, stride=0, dtype=np.float32):
    """render_4d_views restated on numpy inputs: rec holds points, colors, frustum and (with tracks) track_xyz, track_colors,
    track_offsets; stride as l4p_view_mesh takes it (-1: no frusta).  Returns image, depth (dtype), index and, for the record,
    writes (pixel writes offered to the depth test) and covered (pixels that ended up non-empty)."""
    cams = np.asarray(cam_T_world, dtype=np.float32)
    V = cams.shape[0]
    K = np.asarray(intrinsics, dtype=np.float32)
    K = np.broadcast_to(K.reshape(1, 4), (V, 4)) if K.size == 4 else K.reshape(V, 4)
    Ho, Wo = size
    img, dep, idx = [], [], []
    writes = covered = 0
    use_tracks = tracks and "track_xyz" in rec and rec["track_xyz"].shape[0] > 0
    for v in range(V):
        t = int(frames[v])
        zb = ZBuffer(Ho, Wo, dtype)
        tcol = None
        if 0 <= t < T:
            P, C = rec["points"][t * hw:(t + 1) * hw], rec["colors"][t * hw:(t + 1) * hw]
            if use_tracks:
                a, b = int(rec["track_offsets"][t]), int(rec["track_offsets"][t + 1])
                P, tcol = np.concatenate([P, rec["track_xyz"][a:b]]), rec["track_colors"][a:b]
            splat(zb, P, cams[v], K[v], point_size, max_half, near, dtype)
            if stride >= 0:
                mesh(zb, rec["frustum"], t, stride, cams[v], K[v], near, dtype)
        else:
            C = rec["colors"][:hw]
        i, d, n = resolve(zb, C, tcol, hw, background)
        img.append(i), dep.append(d), idx.append(n)
        writes += zb.writes
        covered += int((zb.low != EMPTY_LOW).sum())
    return {"image": np.stack(img), "depth": np.stack(dep), "index": np.stack(idx), "writes": writes, "covered": covered}
