"""numpy restatement of the evaluation metrics (csrc/metrics.hip, l4p_amd/metrics.py), written from the definitions at the
``l4p_metric_*`` entries of include/l4p_hip.h.  Per-element terms are np.float32, one operation at a time; sums are np.float64;
the median is np.partition at (c - 1) // 2; cameras are float64 with np.linalg.svd.  One clip per call.  Not a test module.
"""
import numpy as np

F = np.float32
NAN = float("nan")
TAP_THRESHOLDS = (1, 2, 4, 8, 16)


def _ratio(num, den):
    return float(num) / float(den) if den else NAN


def depth_valid(est, gt, valid, dmin, dmax):
    est, gt = np.asarray(est, F).reshape(-1), np.asarray(gt, F).reshape(-1)
    v = np.ones(est.shape, bool) if valid is None else np.asarray(valid, F).reshape(-1) > F(0.5)
    with np.errstate(invalid="ignore"):
        return v & np.isfinite(gt) & (gt > F(dmin)) & (gt < F(dmax)) & np.isfinite(est) & (est > F(0))


def depth_align(est, gt, valid, mode, dmin=1e-3, dmax=80.0):
    """(s, t) as np.float32 for one clip; the lstsq solve is float64 (np.linalg.lstsq), rounded to f32."""
    ok = depth_valid(est, gt, valid, dmin, dmax)
    e, g = np.asarray(est, F).reshape(-1)[ok], np.asarray(gt, F).reshape(-1)[ok]
    c = e.size
    if mode == "none":
        return F(1), F(0)
    if mode == "median":
        if c == 0:
            return F(NAN), F(0)
        q = g / e  # float32 quotients
        return np.partition(q, (c - 1) // 2)[(c - 1) // 2], F(0)
    if mode == "lstsq":
        e64, g64 = e.astype(np.float64), g.astype(np.float64)
        if c < 2 or not (c * np.sum(e64 * e64) - np.sum(e64) ** 2 > 0):
            return F(NAN), F(NAN)
        sol = np.linalg.lstsq(np.stack([e64, np.ones_like(e64)], 1), g64, rcond=None)[0]
        return F(sol[0]), F(sol[1])
    raise ValueError(mode)


def depth_errors(est, gt, valid, s, t, dmin=1e-3, dmax=80.0):
    """Counts, sums and metrics of one clip under the alignment (s, t)."""
    s, t = F(s), F(t)
    ok = depth_valid(est, gt, valid, dmin, dmax)
    if np.isnan(s) or np.isnan(t):
        ok = np.zeros_like(ok)
    e, g = np.asarray(est, F).reshape(-1)[ok], np.asarray(gt, F).reshape(-1)[ok]
    c = e.size
    m = (s * e).astype(F)
    a = np.minimum(np.maximum((m + t).astype(F), F(dmin)), F(dmax)).astype(F)
    d = (a - g).astype(F)
    abs_rel = (np.abs(d) / g).astype(F)
    sq = (d * d).astype(F)
    r = np.maximum((a / g).astype(F), (g / a).astype(F))
    res = {"count": c, "sum_abs_rel": float(np.sum(abs_rel.astype(np.float64))), "sum_sq": float(np.sum(sq.astype(np.float64)))}
    for k, thr in enumerate((F(1.25), F(1.5625), F(1.953125))):
        res[f"count_delta{k + 1}"] = int(np.sum(r < thr))
        res[f"delta{k + 1}"] = _ratio(res[f"count_delta{k + 1}"], c)
    res["abs_rel"] = res["sum_abs_rel"] / c if c else NAN
    res["rmse"] = float(np.sqrt(res["sum_sq"] / c)) if c else NAN
    res["align_scale"], res["align_shift"] = float(s), float(t)
    return res


def depth(est, gt, valid=None, mode="median", dmin=1e-3, dmax=80.0):
    s, t = depth_align(est, gt, valid, mode, dmin, dmax)
    return depth_errors(est, gt, valid, s, t, dmin, dmax)


def flow(est, gt, valid=None):
    """est, gt, valid [2, ...] of one clip."""
    est, gt = np.asarray(est, F).reshape(2, -1), np.asarray(gt, F).reshape(2, -1)
    v = np.ones(est.shape, F) if valid is None else np.asarray(valid, F).reshape(2, -1)
    ok = (v[0] > F(0.5)) & (v[1] > F(0.5)) & np.isfinite(gt[0]) & np.isfinite(gt[1])
    du, dv = (est[0][ok] - gt[0][ok]).astype(F), (est[1][ok] - gt[1][ok]).astype(F)
    uu, vv = (du * du).astype(F), (dv * dv).astype(F)
    epe = np.sqrt((uu + vv).astype(F)).astype(F)
    c = epe.size
    res = {"count": c, "sum_epe": float(np.sum(epe.astype(np.float64)))}
    res["epe"] = res["sum_epe"] / c if c else NAN
    for px in (1, 3, 5):
        res[f"count_{px}px"] = int(np.sum(epe < F(px)))
        res[f"{px}px"] = _ratio(res[f"count_{px}px"], c)
    return res


def mask(logit, gt, valid=None):
    logit, gt = np.asarray(logit, F).reshape(-1), np.asarray(gt, F).reshape(-1)
    v = np.ones(logit.shape, bool) if valid is None else np.asarray(valid, F).reshape(-1) > F(0.5)
    pp, gp = logit > F(0), gt > F(0.5)
    tp, fp = int(np.sum(v & pp & gp)), int(np.sum(v & pp & ~gp))
    fn, tn = int(np.sum(v & ~pp & gp)), int(np.sum(v & ~pp & ~gp))
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "iou": _ratio(tp, tp + fp + fn), "precision": _ratio(tp, tp + fp),
            "recall": _ratio(tp, tp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn), "accuracy": _ratio(tp + tn, tp + fp + fn + tn)}


def tracks(traj_est, traj_gt, vis_logit, vis_gt, valid, queries, hw):
    """traj [N, 2, T], vis_logit / vis_gt / valid [N, T], queries [N, 3] of one clip; hw = (H, W)."""
    te, tg = np.asarray(traj_est, F), np.asarray(traj_gt, F)
    N, _, T = te.shape
    logit = np.asarray(vis_logit, F).reshape(N, T)
    gv = np.asarray(vis_gt).reshape(N, T) != 0
    ok = np.ones((N, T), bool) if valid is None else np.asarray(valid).reshape(N, T) != 0
    qt = np.floor(np.asarray(queries, F)[:, 0]).astype(np.int64)
    ok = ok & (np.arange(T)[None, :] != qt[:, None])
    sx, sy = F(256) / F(hw[1]), F(256) / F(hw[0])
    dx = ((te[:, 0] - tg[:, 0]).astype(F) * sx).astype(F)
    dy = ((te[:, 1] - tg[:, 1]).astype(F) * sy).astype(F)
    d2 = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
    pv = logit > F(0)
    res = {"count": int(ok.sum()), "count_occ_correct": int((ok & (pv == gv)).sum()), "count_gt_visible": int((ok & gv).sum())}
    res["occlusion_accuracy"] = _ratio(res["count_occ_correct"], res["count"])
    pts, jac = [], []
    for thr in TAP_THRESHOLDS:
        within = d2 < F(thr) * F(thr)
        res[f"count_within_{thr}"] = int((ok & within & gv).sum())
        res[f"count_tp_{thr}"] = int((ok & within & pv & gv).sum())
        res[f"count_fp_{thr}"] = int((ok & pv & ~(gv & within)).sum())
        res[f"pts_within_{thr}"] = _ratio(res[f"count_within_{thr}"], res["count_gt_visible"])
        res[f"jaccard_{thr}"] = _ratio(res[f"count_tp_{thr}"], res["count_gt_visible"] + res[f"count_fp_{thr}"])
        pts.append(res[f"pts_within_{thr}"])
        jac.append(res[f"jaccard_{thr}"])
    res["average_pts_within_thresh"] = float(np.sum(pts)) / 5.0
    res["average_jaccard"] = float(np.sum(jac)) / 5.0
    return res


def umeyama(src, dst):
    """Closed-form similarity dst ~ s R src + t (Umeyama 1991) in float64 with np.linalg.svd; src, dst [T, 3].  The reflection is
    fixed on the last singular value (det(U) det(Vt) < 0 -> -sigma3), so R is a proper rotation at every rank of cov; where it is
    not unique (rank < 2) it is whichever the SVD returns.  The degenerate contracts of include/l4p_hip.h (l4p_metric_cameras):
    cov = 0 -> R = I (and s = 0 when var > 0); var = 0 (a static src, hence cov = 0) -> s = 1, R = I, t = md - ms."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    cov = xd.T @ xs / src.shape[0]
    var = (xs ** 2).sum() / src.shape[0]
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt if D[0] > 0 else np.eye(3)
    s = float(np.trace(np.diag(D) @ S) / var) if var > 0 else 1.0
    return s, R, md - s * R @ ms, cov


def cameras(pose_est, extr_gt, in_dtype=F):
    """pose_est [16, T] row-major world_T_cam, extr_gt [4, 4, T] cam_T_world of one clip, taken as in_dtype values (the kernel reads
    float32), then float64 throughout."""
    P = np.asarray(pose_est, in_dtype).astype(np.float64).reshape(4, 4, -1).transpose(2, 0, 1)
    G = np.linalg.inv(np.asarray(extr_gt, in_dtype).astype(np.float64).transpose(2, 0, 1))
    T = P.shape[0]
    s, R, t, _ = umeyama(P[:, :3, 3], G[:, :3, 3])
    err = (s * (R @ P[:, :3, 3].T).T + t) - G[:, :3, 3]
    sum_ate = float((err ** 2).sum())
    Ps = P.copy()
    Ps[:, :3, 3] *= s
    sum_tr = sum_rot = 0.0
    for i in range(T - 1):
        relP = np.linalg.inv(Ps[i]) @ Ps[i + 1]
        relG = np.linalg.inv(G[i]) @ G[i + 1]
        E = np.linalg.inv(relG) @ relP
        sum_tr += float((E[:3, 3] ** 2).sum())
        ax = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        ang = np.degrees(np.arctan2(0.5 * np.sqrt((ax ** 2).sum()), 0.5 * (np.trace(E[:3, :3]) - 1.0)))
        sum_rot += float(ang ** 2)
    return {"ate": float(np.sqrt(sum_ate / T)), "rpe_trans": float(np.sqrt(sum_tr / (T - 1))),
            "rpe_rot": float(np.sqrt(sum_rot / (T - 1))), "align_scale": s, "sum_sq_ate": sum_ate, "sum_sq_rpe_trans": sum_tr,
            "sum_sq_rpe_rot": sum_rot, "frames": T}


# ------------------------------------------------------------------------------------------------- seeded inputs of the tests
def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_poses(T, seed, extent=2.0):
    """world_T_cam float64 [T, 4, 4]: a smooth path with spread in all three axes and turning cameras."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, T)
    c = np.stack([extent * np.cos(2.5 * u), 0.7 * extent * np.sin(3.1 * u + 0.3), 0.5 * extent * u * u + 0.2 * np.sin(5 * u)], 1)
    c = c + 0.05 * extent * rng.standard_normal((T, 3))
    W = np.tile(np.eye(4), (T, 1, 1))
    for i in range(T):
        W[i, :3, :3] = rot([0.3, 1.0, 0.2], 0.8 * u[i]) @ rot([1.0, 0.1, -0.4], 0.3 * np.sin(4 * u[i]))
        W[i, :3, 3] = c[i]
    return W


def make_camera_case(T, seed, reflect=False, noise=1e-2):
    """(pose_est [16, T] f32, extr_gt [4, 4, T] f32): the estimate is a similarity transform of the gt plus noise of `noise` times the
    extent; reflect=True mirrors the estimated centres, so the cross-covariance of the centres has a negative determinant."""
    rng = np.random.default_rng(seed + 1000)
    Wg = make_poses(T, seed)
    extent = float(np.ptp(Wg[:, :3, 3], axis=0).max())
    s, R, t = 1.7, rot([0.2, -0.5, 1.0], 0.9), np.array([0.5, -1.0, 2.0])
    We = Wg.copy()
    for i in range(T):
        c = Wg[i, :3, 3] * (np.array([1.0, 1.0, -1.0]) if reflect else 1.0)
        We[i, :3, 3] = s * R @ c + t + noise * extent * s * rng.standard_normal(3)
        We[i, :3, :3] = R @ Wg[i, :3, :3] @ rot(rng.standard_normal(3), noise * rng.standard_normal())
    pose = We.transpose(1, 2, 0).reshape(16, T).astype(F)
    extr = np.linalg.inv(Wg).transpose(1, 2, 0).astype(F)
    return pose, extr


def make_dense_case(B, n, seed, lo=0.5, hi=10.0):
    """Seeded depth / flow / mask inputs of B clips with n elements: about 30 % invalid, with non-finite and non-positive values
    planted among the depth estimates and the ground truth.  Depths lie in [lo, hi]."""
    rng = np.random.default_rng(seed)
    d = {}
    gt = rng.uniform(lo, hi, (B, n)).astype(F)
    est = (gt * rng.uniform(0.6, 1.9, (B, n)) * 1.3 + rng.uniform(-0.05, 0.05, (B, n))).astype(F)
    valid = (rng.uniform(size=(B, n)) > 0.2).astype(F)
    for arr, vals in ((est, (np.nan, np.inf, -np.inf, 0.0, -1.0)), (gt, (np.nan, np.inf, 0.0, -2.0, 100.0, 5e-4))):
        idx = rng.choice(B * n, size=max(len(vals), (B * n) // 20), replace=False)
        arr.reshape(-1)[idx] = np.resize(np.asarray(vals, F), idx.size)
    d["depth_est"], d["depth_gt"], d["depth_valid"] = est, gt, valid
    fgt = rng.uniform(-20, 20, (B, 2, n)).astype(F)
    scale = rng.choice(np.asarray([0.3, 1.5, 3.0, 8.0]), (B, 1, n))
    fest = (fgt + scale * rng.standard_normal((B, 2, n))).astype(F)
    fvalid = (rng.uniform(size=(B, 2, n)) > 0.15).astype(F)
    idx = rng.choice(B * 2 * n, size=max(3, (B * n) // 20), replace=False)
    fgt.reshape(-1)[idx] = np.resize(np.asarray([np.nan, np.inf, -np.inf], F), idx.size)
    d["flow_est"], d["flow_gt"], d["flow_valid"] = fest, fgt, fvalid
    d["mask_logit"] = rng.standard_normal((B, n)).astype(F)
    d["mask_logit"].reshape(-1)[:: 7] = 0.0  # a logit of exactly 0 is negative
    d["mask_gt"] = (rng.uniform(size=(B, n)) > 0.6).astype(F)
    d["mask_valid"] = (rng.uniform(size=(B, n)) > 0.3).astype(F)
    return d


def make_track_case(B, N, T, seed, hw=(224, 224)):
    """Seeded track inputs: queries in the first, a middle and the last frame (a last-frame track with everything before it
    invalid scores nothing), distances planted on both sides of every threshold of the 256 x 256 frame."""
    rng = np.random.default_rng(seed)
    H, W = hw
    tg = np.stack([rng.uniform(0, W, (B, N, T)), rng.uniform(0, H, (B, N, T))], 2).astype(F)
    # distance (in the 256 frame) just below / above each threshold, along x or y
    thr = np.asarray([0.0, 0.5, 0.999, 1.001, 1.999, 2.001, 3.999, 4.001, 7.999, 8.001, 15.999, 16.001, 40.0])
    dist = thr[rng.integers(0, thr.size, (B, N, T))]
    along_x = rng.uniform(size=(B, N, T)) > 0.5
    te = tg.copy()
    te[:, :, 0] += np.where(along_x, dist * W / 256.0, 0.0).astype(F)
    te[:, :, 1] += np.where(along_x, 0.0, dist * H / 256.0).astype(F)
    vis_gt = rng.uniform(size=(B, N, 1, T)) > 0.3
    logit = np.where(vis_gt, 1.0, -1.0) * np.where(rng.uniform(size=(B, N, 1, T)) > 0.2, 1.0, -1.0) * rng.uniform(0.1, 3, (B, N, 1, T))
    logit.reshape(-1)[:: 11] = 0.0
    qt = np.resize(np.asarray([0, T // 2, T - 1]), N)[None, :].repeat(B, 0)
    valid = np.arange(T)[None, None, None, :] >= qt[:, :, None, None]  # cleared before the query frame
    valid = valid & (rng.uniform(size=(B, N, 1, T)) > 0.1)
    q = np.stack([qt + 0.5, rng.uniform(0, W, (B, N)), rng.uniform(0, H, (B, N))], 2).astype(F)
    return {"traj_est": te.astype(F), "traj_gt": tg, "vis_logit": logit.astype(F), "vis_gt": vis_gt, "valid": valid, "queries": q, "hw": hw}
