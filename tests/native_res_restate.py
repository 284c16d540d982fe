"""numpy restatement of guided up-sampling (include/l4p_hip.h at l4p_guided_upsample, DESIGN.md "Native-resolution results"), the
yardstick of csrc/upsample.hip, with the seeded cases and the edge scene the tests run it on.

The coordinates x, y, `inside` and the window centre are formed in np.float32 exactly as the definition states (every operation
rounded on its own), so the discrete decisions - which pixels are inside, which taps a pixel has - are the kernel's by construction.
Weights and sums are float64; mean3 / std3 are the f32 values the kernel receives.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DEFAULT_KNOBS = dict(radius=2, sigma_s=1.0, sigma_r=0.1, range_floor=1e-4)


def coords(N, res, crop0, n):
    """(x f32 [N], inside bool [N], centre int64 [N]) of the full-resolution indices 0..N-1 along one axis."""
    s = F32(res) / F32(N)
    x = (np.arange(N).astype(F32) + F32(0.5)) * s - F32(0.5) - F32(crop0)
    inside = (x >= F32(-0.5)) & (x < F32(n) - F32(0.5))
    c = np.floor(x + F32(0.5)).astype(np.int64)
    return x, inside, c


def restate(guide_hi, frame_index, guide_lo, src, res_hw, crop_ij, scale=None, mean=MEAN, std=STD, radius=2, sigma_s=1.0, sigma_r=0.1,
            range_floor=1e-4, spatial_only=False):
    """guide_hi uint8 [B,Tg,H,W,3], frame_index a sequence of T ints or None, guide_lo f32 [B,3,T,h,w], src f32 [B,C,T,h,w].
    Returns (out float64 [B,C,T,H,W], valid uint8 [B,1,T,H,W]).  ``spatial_only``: every range weight is 1 (the spatial Gaussian a
    pixel degrades to when its colour matches no tap, up to the common factor range_floor)."""
    guide_hi, guide_lo, src = np.asarray(guide_hi), np.asarray(guide_lo, dtype=F32), np.asarray(src, dtype=F32)
    B, Tg, H, W, _ = guide_hi.shape
    _, C, T, h, w = src.shape
    fidx = list(range(T)) if frame_index is None else [int(f) for f in frame_index]
    mean64, std64 = np.asarray(mean, dtype=F32).astype(np.float64), np.asarray(std, dtype=F32).astype(np.float64)
    scale64 = np.ones(C) if scale is None else np.asarray(scale, dtype=F32).astype(np.float64)
    x, in_x, cx = coords(W, res_hw[1], crop_ij[1], w)
    y, in_y, cy = coords(H, res_hw[0], crop_ij[0], h)
    inside = in_y[:, None] & in_x[None, :]
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    out = np.zeros((B, C, T, H, W))
    valid = np.zeros((B, 1, T, H, W), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            if not 0 <= fidx[t] < Tg:
                continue
            hi = guide_hi[b, fidx[t]].astype(np.float64) / 255.0
            lo = guide_lo[b, :, t].astype(np.float64) * std64[:, None, None] + mean64[:, None, None]
            s = src[b, :, t]
            usable = np.isfinite(s).all(axis=0)
            s64 = np.where(usable[None], s, 0).astype(np.float64)
            num, den, cnt = np.zeros((C, H, W)), np.zeros((H, W)), np.zeros((H, W), dtype=np.int64)
            for dy in range(-radius, radius + 1):
                qy = cy + dy
                oky = (qy >= 0) & (qy < h)
                qyc = np.clip(qy, 0, h - 1)
                for dx in range(-radius, radius + 1):
                    qx = cx + dx
                    okx = (qx >= 0) & (qx < w)
                    qxc = np.clip(qx, 0, w - 1)
                    use = inside & oky[:, None] & okx[None, :] & usable[qyc][:, qxc]
                    f = np.exp(-((x64 - qx)[None, :] ** 2 + (y64 - qy)[:, None] ** 2) / (2.0 * sigma_s ** 2))
                    d2 = ((hi - np.moveaxis(lo[:, qyc][:, :, qxc], 0, -1)) ** 2).sum(axis=-1)
                    g = np.ones_like(d2) if spatial_only else np.maximum(np.exp(-d2 / (2.0 * sigma_r ** 2)), range_floor)
                    wt = np.where(use, f * g, 0.0)
                    den += wt
                    cnt += use
                    num += wt[None] * s64[:, qyc][:, :, qxc]
            ok = cnt > 0
            out[b, :, t] = np.where(ok[None], scale64[:, None, None] * num / np.where(ok, den, 1.0)[None], 0.0)
            valid[b, 0, t] = ok
    return out, valid


def window_hits(changed_lo, H, W, res_hw, crop_ij, radius):
    """bool [H, W]: the full-resolution pixels whose window meets a changed low-resolution pixel (``changed_lo`` bool [h, w])."""
    h, w = changed_lo.shape
    _, in_x, cx = coords(W, res_hw[1], crop_ij[1], w)
    _, in_y, cy = coords(H, res_hw[0], crop_ij[0], h)
    hit = np.zeros((H, W), dtype=bool)
    for dy in range(-radius, radius + 1):
        qy = cy + dy
        for dx in range(-radius, radius + 1):
            qx = cx + dx
            ok = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            hit |= ok & changed_lo[np.clip(qy, 0, h - 1)][:, np.clip(qx, 0, w - 1)]
    return hit & in_y[:, None] & in_x[None, :]


def _resize_axis(a, axis, out_size):
    """Bilinear resize of one axis with half-pixel centres (F.interpolate, align_corners=False, no antialiasing), float64."""
    n = a.shape[axis]
    c = np.maximum((np.arange(out_size) + 0.5) * (n / out_size) - 0.5, 0.0)
    i0 = np.minimum(np.floor(c).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    lam = (c - i0).reshape([-1 if k == axis else 1 for k in range(a.ndim)])
    return np.take(a, i0, axis=axis) * (1.0 - lam) + np.take(a, i1, axis=axis) * lam


def downsample_guide(guide_hi, frame_index, res_hw, crop_ij, out_hw, mean=MEAN, std=STD):
    """guide_lo f32 [B,3,T,h,w] of guide_hi uint8 [B,Tg,H,W,3]: / 255, the bilinear half-pixel-centre down-sample to ``res_hw``, the
    crop, the frames of ``frame_index`` (entries outside [0, Tg) take frame 0: they are never used), (v - mean) / std."""
    B, Tg = guide_hi.shape[:2]
    v = guide_hi.astype(np.float64) / 255.0
    v = _resize_axis(_resize_axis(v, 2, res_hw[0]), 3, res_hw[1])
    v = v[:, :, crop_ij[0]:crop_ij[0] + out_hw[0], crop_ij[1]:crop_ij[1] + out_hw[1]]
    fidx = [f if 0 <= f < Tg else 0 for f in (range(Tg) if frame_index is None else frame_index)]
    v = np.moveaxis(v[:, fidx], -1, 1)  # [B,3,T,h,w]
    m, s = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    return np.ascontiguousarray(((v - m[None, :, None, None, None]) / s[None, :, None, None, None]).astype(F32))


# (name, B, C, T, Tg, (H, W), res (h, w), crop (i0, j0), (h, w), radius, frame_index)
PARITY_CASES = (
    ("a", 1, 1, 1, 1, (5, 7), (5, 7), (0, 0), (5, 7), 2, None),           # scale 1: every pixel on a tap
    ("b", 2, 4, 3, 3, (23, 40), (12, 20), (0, 0), (12, 20), 2, None),     # anisotropic, non-integer
    ("c", 1, 3, 2, 2, (30, 53), (14, 25), (0, 5), (14, 14), 2, None),     # a spatial crop: cropped-away columns invalid and zero
    ("d", 1, 2, 2, 2, (3, 200), (3, 70), (0, 0), (3, 70), 1, None),       # many tiles along X, a ragged last one, fewer rows than a tile
    ("e", 1, 8, 1, 1, (70, 150), (20, 40), (0, 0), (20, 40), 3, None),    # several tiles on both axes, the largest C and window
    ("f", 1, 1, 5, 3, (9, 11), (5, 6), (0, 0), (5, 6), 1, (0, 1, 2, 1, 0)),  # mirror padding
)


def make_case(seed, B, C, T, Tg, HW, res_hw, crop_ij, out_hw, radius, frame_index):
    """A seeded case: a smooth colour pattern plus noise as guide_hi, its down-sample as guide_lo, smooth fields of different
    magnitudes plus noise as src, a per-channel scale.  Returns the keyword arguments of ``restate`` (numpy)."""
    rng = np.random.default_rng(seed)
    H, W = HW
    h, w = out_hw
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, size=(B, Tg, 1, 1, 3))
    fr = rng.uniform(1.0, 4.0, size=(B, Tg, 1, 1, 3, 2))
    pat = 0.5 + 0.35 * np.sin(2 * np.pi * (fr[..., 0] * xx[None, None, :, :, None] + fr[..., 1] * yy[None, None, :, :, None]) + ph)
    guide_hi = np.clip(np.rint((pat + rng.normal(0, 0.04, size=pat.shape)) * 255), 0, 255).astype(np.uint8)
    guide_lo = downsample_guide(guide_hi, frame_index, res_hw, crop_ij, out_hw)
    v, u = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    amp = (10.0 ** rng.uniform(-1, 1.5, size=(B, C, 1, 1, 1)))
    k = rng.uniform(0.5, 3.0, size=(B, C, T, 1, 1, 2))
    src = amp * (np.sin(2 * np.pi * (k[..., 0] * u + k[..., 1] * v)) + 0.2 * rng.normal(size=(B, C, T, h, w)))
    scale = rng.uniform(0.5, 4.0, size=C).astype(F32)
    return dict(guide_hi=guide_hi, frame_index=frame_index, guide_lo=guide_lo, src=src.astype(F32), res_hw=res_hw, crop_ij=crop_ij,
                scale=scale, radius=radius)


def parity_case(name):
    """(keyword arguments of ``restate``) of the named parity case; the seed is the case's position."""
    for i, c in enumerate(PARITY_CASES):
        if c[0] == name:
            return make_case(100 + i, *c[1:])
    raise KeyError(name)


# ---- the edge scene: (H, W), res (h, w), crop (i0, j0), (h, w) ----
EDGE_SHAPES = (((46, 77), (12, 20), (0, 0), (12, 20)), ((30, 53), (14, 25), (0, 5), (14, 14)), ((23, 40), (12, 20), (0, 0), (12, 20)))
EDGE_COLOURS = ((0.8, 0.25, 0.2), (0.2, 0.7, 0.8))
EDGE_GUIDED_BOUND = 2e-3  # step * 10 * range_floor: about ten wrong-side taps at the floor against one right-side tap
EDGE_BILINEAR_BOUND = 0.5


def edge_scene(HW, res_hw, crop_ij, out_hw, seed=3):
    """A slanted step between two colours.  Full resolution: a pixel is on side B when its centre lies beyond the line
    X + 0.37 Y = 0.55 W (pixel-centre coordinates); its value is 1 on side A and 3 on side B, its colour EDGE_COLOURS[side] plus
    uniform noise of +-0.02 per channel.  Low resolution: guide_lo is the bilinear down-sample of that picture, and the field is
    what a network that sees only guide_lo gives: 1 where the pixel's colour is nearer colour A, 3 where it is nearer colour B.
    Returns (keyword arguments of ``restate`` with B = C = T = 1, truth float64 [H, W])."""
    rng = np.random.default_rng(seed)
    H, W = HW
    Y, X = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    side = (X + 0.37 * Y) > 0.55 * W
    col = np.where(side[..., None], np.asarray(EDGE_COLOURS[1]), np.asarray(EDGE_COLOURS[0])) + rng.uniform(-0.02, 0.02, size=(H, W, 3))
    guide_hi = np.clip(np.rint(col * 255), 0, 255).astype(np.uint8)[None, None]
    guide_lo = downsample_guide(guide_hi, None, res_hw, crop_ij, out_hw)
    lo = guide_lo[0, :, 0].astype(np.float64) * np.asarray(STD)[:, None, None] + np.asarray(MEAN)[:, None, None]
    dA = ((lo - np.asarray(EDGE_COLOURS[0])[:, None, None]) ** 2).sum(axis=0)
    dB = ((lo - np.asarray(EDGE_COLOURS[1])[:, None, None]) ** 2).sum(axis=0)
    src = np.where(dB < dA, 3.0, 1.0).astype(F32)[None, None, None]
    truth = np.where(side, 3.0, 1.0)
    return dict(guide_hi=guide_hi, frame_index=None, guide_lo=guide_lo, src=src, res_hw=res_hw, crop_ij=crop_ij, **DEFAULT_KNOBS), truth


def bilinear_reference(src_hw, valid_hw):
    """F.interpolate(bilinear, align_corners=False) of the low-resolution field [h, w] onto the bounding box of the valid
    full-resolution pixels (bool [H, W]; a box, since validity is separable here).  Returns (field float64, row slice, column slice)."""
    import torch
    import torch.nn.functional as F

    rows, cols = np.flatnonzero(valid_hw.any(axis=1)), np.flatnonzero(valid_hw.any(axis=0))
    ys, xs = slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1)
    up = F.interpolate(torch.from_numpy(np.asarray(src_hw, dtype=np.float64))[None, None], size=(len(rows), len(cols)), mode="bilinear",
                       align_corners=False)
    return up[0, 0].numpy(), ys, xs
