"""numpy restatement of l4p_metric_tracks3d and l4p_metric_depth_full (csrc/metrics.hip), written from the definitions at those
entries of include/l4p_hip.h, and the seeded 3D-track inputs of the tests.  Per-element terms are np.float32, one operation at a
time; sums are np.float64; medians are np.partition at (c - 1) // 2; the inverse-depth least squares is np.linalg.lstsq in
float64; logs are np.log on float64.  One clip per call.  Not a test module.
"""
import numpy as np

from tests.metrics_restate import F, NAN, TAP_THRESHOLDS, _ratio, depth_align, depth_valid, make_track_case

LN10 = 2.302585092994046
SCALES = ("none", "median", "track_median", "query")


def _norm3(x, y, z):
    xx, yy, zz = (x * x).astype(F), (y * y).astype(F), (z * z).astype(F)
    return np.sqrt(((xx + yy).astype(F) + zz).astype(F)).astype(F)


def _unproject(x, y, z, fx, fy, cx, cy):
    X = (((x - cx).astype(F) * z).astype(F) / fx).astype(F)
    Y = (((y - cy).astype(F) * z).astype(F) / fy).astype(F)
    return X, Y, z


def _lower_median(r):
    c = r.size
    return np.partition(r, (c - 1) // 2)[(c - 1) // 2] if c else F(NAN)


def tracks3d(traj_est, depth_est, traj_gt, depth_gt, vis_logit, vis_gt, valid, queries, intrinsics, hw, scale="median"):
    """traj [N, 2, T], depth_est / depth_gt / vis_logit / vis_gt / valid [N, (1,) T], queries [N, 3], intrinsics [4, 4, T] of one
    clip; hw = (H, W).  The names of metrics_restate.tracks, plus "scale" (out[31]) and "track_scales" [N]."""
    te, tg = np.asarray(traj_est, F), np.asarray(traj_gt, F)
    N, _, T = te.shape
    ze, zg = np.asarray(depth_est, F).reshape(N, T), np.asarray(depth_gt, F).reshape(N, T)
    logit = np.asarray(vis_logit, F).reshape(N, T)
    gv = np.asarray(vis_gt).reshape(N, T) != 0
    set_ = np.ones((N, T), bool) if valid is None else np.asarray(valid).reshape(N, T) != 0
    K = np.asarray(intrinsics, F)
    fx, fy, cx, cy = K[0, 0][None], K[1, 1][None], K[0, 2][None], K[1, 2][None]
    qt = np.floor(np.asarray(queries, F)[:, 0]).astype(np.int64)
    with np.errstate(all="ignore"):
        scored = set_ & (np.arange(T)[None, :] != qt[:, None]) & np.isfinite(zg) & (zg > F(0))
        eligible = scored & gv & np.isfinite(ze) & (ze > F(0))
        Gx, Gy, Gz = _unproject(tg[:, 0], tg[:, 1], zg, fx, fy, cx, cy)
        Ex, Ey, Ez = _unproject(te[:, 0], te[:, 1], ze, fx, fy, cx, cy)
        r = (_norm3(Gx, Gy, Gz) / _norm3(Ex, Ey, Ez)).astype(F)
        if scale == "none":
            s = np.full(N, F(1))
            out31 = 1.0
        elif scale == "median":
            s = np.full(N, _lower_median(r[eligible]))
            out31 = float(s[0])
        elif scale == "track_median":
            s = np.asarray([_lower_median(r[i][eligible[i]]) for i in range(N)], F)
            out31 = float(np.isfinite(s).sum())
        elif scale == "query":
            s = np.full(N, F(NAN))
            for i in range(N):
                t = int(qt[i])
                if 0 <= t < T and set_[i, t] and np.isfinite(zg[i, t]) and zg[i, t] > 0 and np.isfinite(ze[i, t]) and ze[i, t] > 0:
                    s[i] = zg[i, t] / ze[i, t]
            out31 = float(np.isfinite(s).sum())
        else:
            raise ValueError(scale)
        sc = s[:, None]
        dx, dy, dz = ((sc * Ex).astype(F) - Gx).astype(F), ((sc * Ey).astype(F) - Gy).astype(F), ((sc * Ez).astype(F) - Gz).astype(F)
        d = _norm3(dx, dy, dz)
        sx, sy = F(256) / F(hw[1]), F(256) / F(hw[0])
        f = np.sqrt(((fx * sx).astype(F) * (fy * sy).astype(F)).astype(F)).astype(F)
        u = (zg / f).astype(F)
        pv = logit > F(0)
        ok = scored
        res = {"count": int(ok.sum()), "count_occ_correct": int((ok & (pv == gv)).sum()), "count_gt_visible": int((ok & gv).sum())}
        res["occlusion_accuracy"] = _ratio(res["count_occ_correct"], res["count"])
        pts, jac = [], []
        for thr in TAP_THRESHOLDS:
            within = d < (F(thr) * u).astype(F)
            res[f"count_within_{thr}"] = int((ok & within & gv).sum())
            res[f"count_tp_{thr}"] = int((ok & within & pv & gv).sum())
            res[f"count_fp_{thr}"] = int((ok & pv & ~(gv & within)).sum())
            res[f"pts_within_{thr}"] = _ratio(res[f"count_within_{thr}"], res["count_gt_visible"])
            res[f"jaccard_{thr}"] = _ratio(res[f"count_tp_{thr}"], res["count_gt_visible"] + res[f"count_fp_{thr}"])
            pts.append(res[f"pts_within_{thr}"])
            jac.append(res[f"jaccard_{thr}"])
    res["average_pts_within_thresh"] = float(np.sum(pts)) / 5.0
    res["average_jaccard"] = float(np.sum(jac)) / 5.0
    res["scale"] = out31
    res["track_scales"] = s
    res["eligible_per_track"] = eligible.sum(1)
    res["ratios"], res["eligible"] = r, eligible
    return res


# ------------------------------------------------------------------------------------------------- depth
def depth_full_align(est, gt, valid, mode, dmin=1e-3, dmax=80.0):
    """(s, t) as np.float32 of one clip for every alignment of l4p_metric_depth_full."""
    if mode != "lstsq_inv":
        return depth_align(est, gt, valid, mode, dmin, dmax)
    ok = depth_valid(est, gt, valid, dmin, dmax)
    e, g = np.asarray(est, F).reshape(-1)[ok], np.asarray(gt, F).reshape(-1)[ok]
    with np.errstate(all="ignore"):
        x, y = (F(1) / e).astype(F).astype(np.float64), (F(1) / g).astype(F).astype(np.float64)
    c = x.size
    if c < 2 or not (c * np.sum(x * x) - np.sum(x) ** 2 > 0):
        return F(NAN), F(NAN)
    sol = np.linalg.lstsq(np.stack([x, np.ones_like(x)], 1), y, rcond=None)[0]
    return F(sol[0]), F(sol[1])


def depth_full_aligned(e, s, t, inv, dmin, dmax):
    """the aligned value a of the valid estimates e (f32) under (s, t)"""
    s, t = F(s), F(t)
    if not inv:
        m = (s * e).astype(F)
        return np.minimum(np.maximum((m + t).astype(F), F(dmin)), F(dmax)).astype(F), None
    x = (F(1) / e).astype(F)
    p = ((s * x).astype(F) + t).astype(F)
    lo, hi = F(1) / F(dmax), F(1) / F(dmin)
    pc = np.minimum(np.maximum(p, lo), hi).astype(F)
    return np.minimum(np.maximum((F(1) / pc).astype(F), F(dmin)), F(dmax)).astype(F), int(np.sum(pc != p))


def depth_full_errors(est, gt, valid, s, t, inv=False, dmin=1e-3, dmax=80.0):
    """Counts, sums and metrics of one clip under the alignment (s, t): the names of metrics_restate.depth_errors, then the
    log-space sums and metrics; "clamped_inv" counts the elements clamped in disparity."""
    s, t = F(s), F(t)
    ok = depth_valid(est, gt, valid, dmin, dmax)
    if np.isnan(s) or np.isnan(t):
        ok = np.zeros_like(ok)
    e, g = np.asarray(est, F).reshape(-1)[ok], np.asarray(gt, F).reshape(-1)[ok]
    c = e.size
    with np.errstate(all="ignore"):
        a, clamped = depth_full_aligned(e, s, t, inv, dmin, dmax)
        d = (a - g).astype(F)
        abs_rel = (np.abs(d) / g).astype(F)
        sq = (d * d).astype(F)
        sq_rel = (sq / g).astype(F)
        r = np.maximum((a / g).astype(F), (g / a).astype(F))
        l = np.log(a.astype(np.float64)) - np.log(g.astype(np.float64))
    res = {"count": c, "sum_abs_rel": float(np.sum(abs_rel.astype(np.float64))), "sum_sq": float(np.sum(sq.astype(np.float64))),
           "sum_sq_rel": float(np.sum(sq_rel.astype(np.float64))), "sum_log": float(np.sum(l)), "sum_log_sq": float(np.sum(l * l)),
           "sum_abs_log": float(np.sum(np.abs(l))), "clamped_inv": clamped}
    for k, thr in enumerate((F(1.25), F(1.5625), F(1.953125))):
        res[f"count_delta{k + 1}"] = int(np.sum(r < thr))
        res[f"delta{k + 1}"] = _ratio(res[f"count_delta{k + 1}"], c)
    res["abs_rel"] = res["sum_abs_rel"] / c if c else NAN
    res["rmse"] = float(np.sqrt(res["sum_sq"] / c)) if c else NAN
    res["sq_rel"] = res["sum_sq_rel"] / c if c else NAN
    res["rmse_log"] = float(np.sqrt(res["sum_log_sq"] / c)) if c else NAN
    res["log10"] = (res["sum_abs_log"] / c) / LN10 if c else NAN
    res["log_var"] = res["sum_log_sq"] / c - (res["sum_log"] / c) ** 2 if c else NAN
    res["silog"] = 100.0 * float(np.sqrt(max(res["log_var"], 0.0))) if c else NAN
    res["align_scale"], res["align_shift"] = float(s), float(t)
    return res


def depth_full(est, gt, valid=None, mode="median", dmin=1e-3, dmax=80.0):
    s, t = depth_full_align(est, gt, valid, mode, dmin, dmax)
    return depth_full_errors(est, gt, valid, s, t, mode == "lstsq_inv", dmin, dmax)


# ------------------------------------------------------------------------------------------------- seeded inputs of the tests
K_STEPS = np.asarray([0.0, 0.5, 0.999, 1.001, 1.999, 2.001, 3.999, 4.001, 7.999, 8.001, 15.999, 16.001, 40.0])


def make_track3d_case(B, N, T, seed, hw=(224, 224), per_track=False):
    """make_track_case plus intrinsics that vary per frame, gt depths in [1, 8] and an estimate whose 3D point is the gt point moved
    by k * zg / f256 (k on both sides of every threshold) along a random direction, divided by a hidden scale (1.7 for the clip, or
    one per track in [0.5, 2.5]) and projected back to (x, y, z).  Planted: non-finite / non-positive depths on both sides; the last
    track with gt visibility all clear (no eligible frame); track 1 (N > 1) with a NaN estimate depth in its query frame (no "query"
    scale); frame 1 of track 0 copied into frame 3 together with its intrinsics (two bit-equal ratios: the tie rule).  T >= 5."""
    c = make_track_case(B, N, T, seed, hw)
    rng = np.random.default_rng(seed + 5000)
    H, W = hw
    fx0 = W * rng.uniform(0.8, 1.6, (B, 1))
    fx = fx0 * (1.0 + rng.uniform(-0.05, 0.05, (B, T)))
    K = np.zeros((B, 4, 4, T))
    K[:, 0, 0], K[:, 1, 1] = fx, 1.1 * fx
    K[:, 0, 2], K[:, 1, 2] = W / 2 + rng.uniform(-3, 3, (B, T)), H / 2 + rng.uniform(-3, 3, (B, T))
    K[:, 2, 2] = K[:, 3, 3] = 1.0
    K[:, :, :, 3] = K[:, :, :, 1]
    K = K.astype(F)
    k64 = K.astype(np.float64)
    kfx, kfy, kcx, kcy = k64[:, 0, 0][:, None], k64[:, 1, 1][:, None], k64[:, 0, 2][:, None], k64[:, 1, 2][:, None]  # [B, 1, T]
    zg = rng.uniform(1.0, 8.0, (B, N, T)).astype(F)
    tg = c["traj_gt"].astype(np.float64)
    G = np.stack([(tg[:, :, 0] - kcx) * zg / kfx, (tg[:, :, 1] - kcy) * zg / kfy, zg.astype(np.float64)], -1)  # [B, N, T, 3]
    f256 = np.sqrt(kfx * (256.0 / W) * kfy * (256.0 / H))
    step = K_STEPS[rng.integers(0, K_STEPS.size, (B, N, T))] * zg / f256
    direction = rng.standard_normal((B, N, T, 3))
    direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
    hidden = rng.uniform(0.5, 2.5, (B, N, 1, 1)) if per_track else np.full((B, N, 1, 1), 1.7)
    E = (G + step[..., None] * direction) / hidden
    ze = E[..., 2]
    te = np.stack([E[..., 0] * kfx / ze + kcx, E[..., 1] * kfy / ze + kcy], 2).astype(F)  # [B, N, 2, T]
    ze = ze.astype(F)
    for arr, vals, share in ((ze, (np.nan, np.inf, 0.0, -1.0), 0.04), (zg, (np.nan, 0.0, -2.0), 0.025)):
        idx = rng.choice(B * N * T, size=max(len(vals), int(share * B * N * T)), replace=False)
        arr.reshape(-1)[idx] = np.resize(np.asarray(vals, F), idx.size)
    vis_gt, valid, logit = c["vis_gt"].copy(), c["valid"].copy(), c["vis_logit"]
    vis_gt[:, N - 1] = False
    if N > 1:
        ze[:, 1, T // 2] = np.nan  # track 1 is queried in frame T // 2
    # track 0 (queried in frame 0): frames 1 and 3 are one and the same eligible sample
    zg[:, 0, 1], ze[:, 0, 1] = np.maximum(np.nan_to_num(zg[:, 0, 1], nan=2.0, posinf=2.0), 1.0), np.maximum(
        np.nan_to_num(ze[:, 0, 1], nan=1.0, posinf=1.0), 0.25)
    vis_gt[:, 0, 0, 1] = valid[:, 0, 0, 1] = True
    for a in (zg, ze):
        a[:, 0, 3] = a[:, 0, 1]
    for a in (te, c["traj_gt"]):
        a[:, 0, :, 3] = a[:, 0, :, 1]
    vis_gt[:, 0, 0, 3] = valid[:, 0, 0, 3] = True
    return {"traj_est": te, "depth_est": ze[:, :, None], "traj_gt": c["traj_gt"], "depth_gt": zg[:, :, None], "vis_logit": logit,
            "vis_gt": vis_gt, "valid": valid, "queries": c["queries"], "intrinsics": K, "hw": hw, "hidden": hidden.reshape(B, N)}


def tracks3d_of_case(c, b, scale, valid="case"):
    return tracks3d(c["traj_est"][b], c["depth_est"][b], c["traj_gt"][b], c["depth_gt"][b], c["vis_logit"][b], c["vis_gt"][b],
                    c["valid"][b] if valid == "case" else valid, c["queries"][b], c["intrinsics"][b], c["hw"], scale)
