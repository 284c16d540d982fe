"""float64 numpy restatement of the scene-flow definitions (include/l4p_hip.h at l4p_scene_flow, DESIGN.md "Scene flow"), the
yardstick of csrc/sceneflow.hip, and the seeded cases the tests run it on.

Everything is float64 (inverses by numpy.linalg.inv of the f32 matrices) with three exceptions, which make the discrete decisions
identical to the kernel's by construction:
  * q = (i + F_x, j + F_y) and the bilinear weights are formed in np.float32 exactly as the definitions state, so `inside`, the
    tap indices and the weights are the kernel's;
  * the summary's magnitudes are restated in np.float32 from the fields under test (only the summation order differs);
  * the D > 0 test is evaluated on the f32 input.
"""
from __future__ import annotations

import numpy as np

from l4p_amd.utils.recon4d import colour_bytes
from l4p_amd.utils.vis2d import turbo_table

F32 = np.float32


def _taps(flow_t, H, W):
    """q, inside, tap indices and weights of one frame's flow [2, H, W] (f32), in f32 as the kernel forms them."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        qx = ii.astype(F32) + flow_t[0].astype(F32)
        qy = jj.astype(F32) + flow_t[1].astype(F32)
        inside = (qx >= F32(0)) & (qx <= F32(W - 1)) & (qy >= F32(0)) & (qy <= F32(H - 1))  # NaN fails
    qxs, qys = np.where(inside, qx, F32(0)), np.where(inside, qy, F32(0))
    flx, fly = np.floor(qxs), np.floor(qys)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = qxs - flx, qys - fly  # f32
    one = F32(1)
    w = ((one - ay) * (one - ax), (one - ay) * ax, ay * (one - ax), ay * ax)  # f32 products
    return ii, jj, qx, qy, qxs, qys, inside, (x0, x1, y0, y1), w


def restate(depth, flow, P, K):
    """depth [B,1,T,H,W], flow [B,2,T,H,W], P = world_T_cam and K [B,4,4,T], all f32 numpy.  Returns float64 fields scene
    [B,3,T,H,W], rigid, comp [B,2,T,H,W], valid uint8 [B,1,T,H,W], and for the tests X (X_t) and Xp (X'_{t-1}) [B,3,T,H,W], xcz
    (x_c.z) and the f32 q [B,2,T,H,W], inside [B,1,T,H,W], dprev (d') [B,1,T,H,W]."""
    depth, flow, P, K = (np.asarray(a, dtype=F32) for a in (depth, flow, P, K))
    B, _, T, H, W = depth.shape
    z = lambda c, dt=np.float64: np.zeros((B, c, T, H, W), dtype=dt)  # noqa: E731
    res = dict(scene=z(3), rigid=z(2), comp=z(2), valid=z(1, np.uint8), X=z(3), Xp=z(3), xcz=z(1), q=z(2, F32), inside=z(1, bool),
               dprev=z(1))
    for b in range(B):
        for t in range(T):
            Kt, Pt = K[b, :3, :3, t].astype(np.float64), P[b, :, :, t].astype(np.float64)
            jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            pix = np.stack([ii, jj, np.ones_like(ii)]).reshape(3, -1).astype(np.float64)
            D = depth[b, 0, t]
            with np.errstate(all="ignore"):
                X = Pt[:3, :3] @ (np.linalg.inv(Kt) @ pix * D.reshape(1, -1).astype(np.float64)) + Pt[:3, 3:]
            res["X"][b, :, t] = X.reshape(3, H, W)
            if t == 0:
                continue
            Kp, Pp = K[b, :3, :3, t - 1].astype(np.float64), P[b, :, :, t - 1].astype(np.float64)
            _, _, qx, qy, qxs, qys, inside, (x0, x1, y0, y1), w = _taps(flow[b, :, t], H, W)
            Dp = depth[b, 0, t - 1].astype(np.float64)
            with np.errstate(all="ignore"):
                dp = (w[0].astype(np.float64) * Dp[y0, x0] + w[1].astype(np.float64) * Dp[y0, x1]
                      + w[2].astype(np.float64) * Dp[y1, x0] + w[3].astype(np.float64) * Dp[y1, x1])
                qh = np.stack([qxs, qys, np.ones_like(qxs)]).reshape(3, -1).astype(np.float64)
                Xp = Pp[:3, :3] @ (np.linalg.inv(Kp) @ qh * dp.reshape(1, -1)) + Pp[:3, 3:]
                S = Xp - X
                Pinv = np.linalg.inv(Pp)
                xc = Pinv[:3, :3] @ X + Pinv[:3, 3:]
                front = xc[2] > 1e-6
                zc = np.where(front, xc[2], 1.0)
                R = (Kp[:2] @ xc) / zc - pix[:2]
                R = np.where(front, R, 0.0)
                C = flow[b, :, t].reshape(2, -1).astype(np.float64) - R
                finite = np.isfinite(S).all(0) & np.isfinite(R).all(0) & np.isfinite(C).all(0)
                ok = inside.reshape(-1) & (D.reshape(-1) > F32(0)) & (dp.reshape(-1) > 0) & front & finite
            res["scene"][b, :, t] = np.where(ok, S, 0.0).reshape(3, H, W)
            res["rigid"][b, :, t] = np.where(ok, R, 0.0).reshape(2, H, W)
            res["comp"][b, :, t] = np.where(ok, C, 0.0).reshape(2, H, W)
            res["valid"][b, 0, t] = ok.reshape(H, W)
            res["Xp"][b, :, t] = Xp.reshape(3, H, W)
            res["xcz"][b, 0, t] = xc[2].reshape(H, W)
            res["q"][b, 0, t], res["q"][b, 1, t] = qx, qy
            res["inside"][b, 0, t] = inside
            res["dprev"][b, 0, t] = dp
    return res


def magnitudes(scene, comp):
    """(|S| [B,T,H,W], |C| [B,T,H,W]) in f32: sqrt of the unfused sum of squares, left to right."""
    s, c = np.asarray(scene, dtype=F32), np.asarray(comp, dtype=F32)
    ms = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
    mc = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1])
    return ms, mc


def restate_summary(scene, comp, valid, mask=None, tau_px=1.0):
    """[B, T, 8] float64 from f32 fields (the ones under test), a uint8 valid plane and optional f32 mask logits."""
    ms, mc = magnitudes(scene, comp)
    v = np.asarray(valid)[:, 0] != 0
    m = np.zeros(v.shape, dtype=F32) if mask is None else np.asarray(mask, dtype=F32)[:, 0]
    with np.errstate(invalid="ignore"):
        st, dy = v & (m <= F32(0)), v & (m > F32(0))
    f = lambda sel, x=None: (sel if x is None else np.where(sel, x.astype(np.float64), 0.0)).sum(axis=(2, 3), dtype=np.float64)  # noqa: E731
    return np.stack([f(v), f(st), f(dy), f(st, mc), f(dy, mc), f(st, ms), f(dy, ms), f(v & (mc > F32(tau_px)))], axis=-1)


def restate_colors(scene, valid, s_max):
    """uint8 [B, T*H*W, 3]: entry floor(255 min(1, |S| / s_max)) (f32) of colour_bytes(turbo_table()), (128, 128, 128) where invalid."""
    s = np.asarray(scene, dtype=F32)
    B = s.shape[0]
    ms, _ = magnitudes(s, np.zeros((B, 2) + s.shape[2:], dtype=F32))
    lut = colour_bytes(turbo_table())
    r = ms / F32(s_max)
    k = np.floor(F32(255) * np.minimum(r, F32(1))).astype(np.int64)
    col = lut[np.clip(k, 0, 255)]
    col[np.asarray(valid)[:, 0] == 0] = (128, 128, 128)
    return col.reshape(B, -1, 3)


def _rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_case(seed, B, T, H, W, flow_noise=1.5, border=1e-3):
    """Well-conditioned seeded inputs (f32 numpy): depth in [1, 4] (smooth plus noise), fx, fy in [0.8, 1.5] max(H, W), principal
    point near the centre, K different per frame and batch element, poses = small rigid motions different per batch element, flow =
    the exact rigid flow of that depth plus a seeded perturbation on a rectangular "object", mask logits +-2 matching the object.

    Asserts what lets `valid` be compared exactly: every pixel valid apart from the x_c.z test has |x_c.z| >= 0.1, and no q
    coordinate lies within `border` of 0, W - 1 (x) or 0, H - 1 (y); flow values that would are moved by 1 / 16 px first."""
    g = np.random.default_rng(seed)
    m = max(H, W)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.empty((B, 1, T, H, W), dtype=F32)
    K = np.zeros((B, 4, 4, T), dtype=F32)
    P = np.zeros((B, 4, 4, T), dtype=F32)
    for b in range(B):
        ph = g.uniform(0, 6.28, 2)
        axis, dirn = g.normal(size=3), g.normal(size=3)
        dirn /= np.linalg.norm(dirn)
        for t in range(T):
            d = 2.5 + 0.9 * np.sin(ii / (0.35 * W + 1) + ph[0] + 0.2 * t) * np.cos(jj / (0.35 * H + 1) + ph[1]) + g.uniform(-0.5, 0.5, (H, W))
            depth[b, 0, t] = np.clip(d, 1.0, 4.0)
            fx, fy = g.uniform(0.8, 1.5, 2) * m
            K[b, :, :, t] = np.array([[fx, 0.01 * m * g.uniform(-1, 1), (W - 1) / 2 + g.uniform(-0.5, 0.5), 0],
                                      [0, fy, (H - 1) / 2 + g.uniform(-0.5, 0.5), 0], [0, 0, 1, 0], [0, 0, 0, 1]])
            M = np.eye(4)
            M[:3, :3] = _rodrigues(axis, 0.012 * t * (1 + 0.3 * g.uniform(-1, 1)))
            M[:3, 3] = dirn * 0.06 * t + g.uniform(-0.01, 0.01, 3)
            P[b, :, :, t] = M
    flow = np.zeros((B, 2, T, H, W), dtype=F32)
    mask = np.empty((B, 1, T, H, W), dtype=F32)
    r0, r1, c0, c1 = H // 4, max(H // 4 + 1, H // 2 + 1), W // 3, max(W // 3 + 1, 2 * W // 3)
    obj = np.zeros((H, W), dtype=bool)
    obj[r0:r1, c0:c1] = True
    for b in range(B):
        for t in range(T):
            mask[b, 0, t] = np.where(obj, 2.0, -2.0) + g.uniform(-0.5, 0.5, (H, W))
            if t == 0:
                flow[b, :, t] = g.uniform(-1, 1, (2, H, W))  # never read by the definitions
                continue
            f = _rigid_only(depth, P, K, b, t) + np.where(obj, g.uniform(-flow_noise, flow_noise, (2, H, W)), 0.0)
            f = f.astype(F32)
            for c, hi in ((0, W - 1), (1, H - 1)):
                base = (ii if c == 0 else jj).astype(F32)
                q = base + f[c]
                near = (np.abs(q) < 16 * border) | (np.abs(q - F32(hi)) < 16 * border)
                f[c] = np.where(near, f[c] + F32(0.0625), f[c])
            flow[b, :, t] = f
    chk = restate(depth, flow, P, K)
    for c, hi in ((0, W - 1), (1, H - 1)):
        q = chk["q"][:, c, 1:].astype(np.float64)
        assert (np.abs(q) >= border).all() and (np.abs(q - hi) >= border).all(), ("q too close to the border", seed, B, T, H, W)
    pre = chk["inside"][:, 0, 1:] & (depth[:, 0, 1:] > 0) & (chk["dprev"][:, 0, 1:] > 0)
    assert (np.abs(chk["xcz"][:, 0, 1:][pre]) >= 0.1).all(), ("x_c.z too close to 0", seed, B, T, H, W)
    return dict(depth=depth, flow=flow, P=P, K=K, mask=mask)


def _rigid_only(depth, P, K, b, t):
    """float64 [2, H, W]: the flow a static scene of depth[b, 0, t] shows between frames t and t - 1 (no validity)."""
    H, W = depth.shape[-2:]
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pix = np.stack([ii, jj, np.ones_like(ii)]).reshape(3, -1).astype(np.float64)
    Kt, Pt = K[b, :3, :3, t].astype(np.float64), P[b, :, :, t].astype(np.float64)
    Kp, Pp = K[b, :3, :3, t - 1].astype(np.float64), P[b, :, :, t - 1].astype(np.float64)
    X = Pt[:3, :3] @ (np.linalg.inv(Kt) @ pix * depth[b, 0, t].reshape(1, -1).astype(np.float64)) + Pt[:3, 3:]
    Pinv = np.linalg.inv(Pp)
    xc = Pinv[:3, :3] @ X + Pinv[:3, 3:]
    return ((Kp[:2] @ xc) / xc[2] - pix[:2]).reshape(2, H, W)


def extent(a) -> float:
    return float(np.abs(np.asarray(a)).max())


# (seed, B, T, H, W) of the parity tests: the smallest shapes at which the kernel can go wrong
PARITY_CASES = [(11, 1, 1, 5, 7), (12, 1, 2, 5, 7), (13, 2, 3, 17, 19), (14, 1, 3, 3, 70), (15, 1, 3, 40, 52)]
ADVERSARIAL_CASE = (16, 1, 3, 9, 11)
