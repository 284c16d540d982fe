"""numpy restatement of the object-motion stage (include/l4p_hip.h "Object motion and models", csrc/object_motion.hip) and the
clips of its tests.  int64 and float64 (and float32 where the header says f32), no torch device.

``restate`` follows the header's rule: the pairs (the labelling's temporal edge, the same-object test, the tables' fixed-point
rule), the centre pass, the fit and refit passes as int64 sums, the solve in float64, the composition and the canonical points.
The integer part (pairs, centres, far pairs, inlier sets, moments) is exact, so the GPU tests compare bytes.  The rotation is NOT
the header's closed form: it is Kabsch through ``np.linalg.svd`` with the determinant sign, so the models agree with the GPU's
within rounding, not bit for bit, and an inlier set could differ if a residual sat on the threshold - ``margins`` reports how far
from it the nearest one is, and the CPU tests assert that the cases stay clear."""
import numpy as np

from tests import moving_objects_restate as RS

F32 = np.float32
FAR = 1 << 21
EYE12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
INT_FIELDS = ("n_pairs", "n_inliers", "n_far", "valid", "moments")
DTYPES = dict(n_pairs=np.int32, n_inliers=np.int32, n_far=np.int32, valid=np.uint8, moments=np.int64, pose_valid=np.uint8)


def fixed(p, grid):
    """(ok [N] bool, s [N, 3] int64) of f32 points [N, 3]: the rule of l4p_objects_tables."""
    p = np.ascontiguousarray(p, dtype=F32)
    g = np.asarray(grid, dtype=F32).reshape(4)
    v = g[3]
    ok = np.isfinite(p).all(axis=1)
    if not (v > 0 and np.isfinite(v)):
        return np.zeros(len(p), dtype=bool), np.zeros(p.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        q = (p - g[None, :3]) / v
        s = np.floor(q * F32(256.0))
        assert q.dtype == F32 and s.dtype == F32
        ok &= ((s >= F32(-(1 << 28))) & (s < F32(1 << 28))).all(axis=1)  # NaN fails
    return ok, np.where(ok[:, None], s, 0).astype(np.int64)


def pairs(object_id, K, points, grid, flow=None):
    """The pairs in ascending order of the later pixel: dict(m, mp [P] int64, row [P] = k T + t, a, b [P, 3] int64, pa, pb [P, 3] f32)."""
    ids = np.asarray(object_id)
    T, H, W = ids.shape
    pts = np.ascontiguousarray(points, dtype=F32).reshape(T * H * W, 3)
    idx = np.arange(T * H * W, dtype=np.int64).reshape(T, H, W)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ms, mps = [], []
    for t in range(1, T):
        on = (ids[t] >= 0) & (ids[t] < K)
        yq, xq = yy, xx
        if flow is not None:
            u, v = np.asarray(flow[0][t], dtype=F32), np.asarray(flow[1][t], dtype=F32)
            with np.errstate(invalid="ignore", over="ignore"):
                gx = np.floor((xx.astype(F32) + u) + F32(0.5))
                gy = np.floor((yy.astype(F32) + v) + F32(0.5))
                assert gx.dtype == F32 and gy.dtype == F32
                inside = (gx >= 0) & (gx < F32(W)) & (gy >= 0) & (gy < F32(H))
            on = on & np.isfinite(u) & np.isfinite(v) & inside
            xq, yq = np.where(on, gx, 0).astype(np.int64), np.where(on, gy, 0).astype(np.int64)
        on = on & (ids[t - 1][yq, xq] == ids[t])
        ms.append(idx[t][on]), mps.append(idx[t - 1][yq, xq][on])
    m = np.concatenate(ms) if ms else np.zeros(0, dtype=np.int64)
    mp = np.concatenate(mps) if mps else np.zeros(0, dtype=np.int64)
    oka, a = fixed(pts[mp], grid)
    okb, b = fixed(pts[m], grid)
    ok = oka & okb
    m, mp = m[ok], mp[ok]
    row = ids.reshape(-1)[m].astype(np.int64) * T + m // (H * W)
    return dict(m=m, mp=mp, row=row, a=a[ok], b=b[ok], pa=pts[mp], pb=pts[m])


def _floor_div(s, n):
    return np.where(n > 0, s // np.maximum(n, 1), 0)  # numpy's // on int64 is the floor


def kabsch(cov):
    """The rotation that maximises tr(R^T cov): float64 SVD with the determinant sign.  Also returns the singular values."""
    U, D, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    return U @ S @ Vt, D


def solve(mom, cen, grid, min_pairs):
    """float64 models [R, 12], rms [R], valid [R], sigma2 / sigma1 [R] (nan on rows without a rotation fit) and the centroids A, B."""
    rows = len(mom)
    g = np.asarray(grid, dtype=F32).reshape(4).astype(np.float64)
    q = g[3] / 256.0
    model, rms, ratio = np.tile(EYE12, (rows, 1)), np.zeros(rows), np.full(rows, np.nan)
    AB = np.zeros((rows, 2, 3))
    valid = (mom[:, 0] >= min_pairs).astype(np.uint8)
    for r in range(rows):
        S = mom[r].astype(np.float64)
        S[16:18] = mom[r, 16:18].astype(np.uint64).astype(np.float64)  # the sums of squares are unsigned: up to 3 * 2^62
        n = S[0]
        if n < 1:
            continue
        sa, sb = S[1:4], S[4:7]
        C = S[7:16].reshape(3, 3) - np.outer(sb, sa) / n
        Saa = S[16] - ((sa[0] * sa[0] + sa[1] * sa[1]) + sa[2] * sa[2]) / n
        Sbb = S[17] - ((sb[0] * sb[0] + sb[1] * sb[1]) + sb[2] * sb[2]) / n
        R = np.eye(3)
        if valid[r]:
            R, D = kabsch(C / n)
            ratio[r] = D[1] / D[0] if D[0] > 0 else 0.0
        A = g[:3] + ((cen[r, :3].astype(np.float64) + sa / n) + 0.5) * q
        B = g[:3] + ((cen[r, 3:].astype(np.float64) + sb / n) + 0.5) * q
        t = B - R @ A
        rms[r] = q * np.sqrt(max(0.0, ((Sbb + Saa) - 2.0 * float((R * C).sum())) / n))
        model[r, :9], model[r, 9:] = R.reshape(-1), t
        AB[r, 0], AB[r, 1] = A, B
    return model, rms, valid, ratio, AB


def restate(object_id, K, points, grid, flow=None, n_refits=1, inlier_voxels=2.0, min_pairs=16):
    """Every output of ``rigid_motion`` as host arrays, plus ``ratio`` [K, T] (sigma2 / sigma1 of the last round's covariance on valid
    rows, nan elsewhere), ``margin`` (the smallest |residual - tau| / tau over every inlier test made, inf when none was), ``AB``
    [K, T, 2, 3] (the float64 centroids t = B - R A is formed from), ``extent_d`` [K, T] (the largest |d| of a counted pair, in
    fixed-point steps) and ``pairs``."""
    ids = np.asarray(object_id)
    T, H, W = ids.shape
    rows = K * T
    g = np.asarray(grid, dtype=F32).reshape(4)
    pr = pairs(ids, K, points, g, flow)
    row = pr["row"]
    n = np.bincount(row, minlength=rows).astype(np.int64)
    sa, sb = np.zeros((rows, 3), dtype=np.int64), np.zeros((rows, 3), dtype=np.int64)
    np.add.at(sa, row, pr["a"]), np.add.at(sb, row, pr["b"])
    cen = np.concatenate([_floor_div(sa, n[:, None]), _floor_div(sb, n[:, None])], axis=1)
    da, db = pr["a"] - cen[row, :3], pr["b"] - cen[row, 3:]
    far = (np.abs(da) >= FAR).any(axis=1) | (np.abs(db) >= FAR).any(axis=1)
    n_far = np.bincount(row[far], minlength=rows).astype(np.int64)
    tau = F32(inlier_voxels) * g[3]
    assert tau.dtype == F32
    margin, model32 = np.inf, None
    for rnd in range(n_refits + 1):
        sel = ~far
        if rnd > 0:
            mo = model32[row]  # [P, 12] f32, the round before
            pa, pb = pr["pa"], pr["pb"]
            with np.errstate(all="ignore"):
                d = [((mo[:, 3 * i] * pa[:, 0] + mo[:, 3 * i + 1] * pa[:, 1]) + mo[:, 3 * i + 2] * pa[:, 2]) + mo[:, 9 + i] - pb[:, i]
                     for i in range(3)]
                r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                assert r2.dtype == F32
                inl = r2 <= tau * tau  # NaN fails
            if sel.any():
                res = np.sqrt(r2[sel].astype(np.float64))
                margin = min(margin, float(np.min(np.abs(res - float(tau)) / float(tau))))
            sel = sel & inl
        mom = np.zeros((rows, 18), dtype=np.int64)
        r_, a_, b_ = row[sel], da[sel], db[sel]
        np.add.at(mom[:, 0], r_, 1)
        np.add.at(mom[:, 1:4], r_, a_), np.add.at(mom[:, 4:7], r_, b_)
        np.add.at(mom[:, 7:16], r_, (b_[:, :, None] * a_[:, None, :]).reshape(-1, 9))
        np.add.at(mom[:, 16], r_, (a_ * a_).sum(axis=1)), np.add.at(mom[:, 17], r_, (b_ * b_).sum(axis=1))
        model, rms, valid, ratio, AB = solve(mom, cen, g, min_pairs)
        model32 = model.astype(F32)
    ext = np.zeros(rows, dtype=np.int64)
    np.maximum.at(ext, row[sel], np.maximum(np.abs(da[sel]).max(axis=1), np.abs(db[sel]).max(axis=1)) if sel.any() else 0)
    # composition over the emitted f32 motions, float64
    present = np.zeros((K, T), dtype=bool)
    on = (ids >= 0) & (ids < K)
    tt = np.broadcast_to(np.arange(T)[:, None, None], ids.shape)
    present[ids[on], tt[on]] = True
    M32 = model32.reshape(K, T, 12)
    pose, pose_valid, inv = np.tile(EYE12, (K, T, 1)), np.ones((K, T), dtype=np.uint8), np.zeros((K, T, 12))
    v2 = valid.reshape(K, T)
    for k in range(K):
        first = int(np.argmax(present[k])) if present[k].any() else T
        G, ok = np.eye(4), True
        for t in range(T):
            if t > first:
                Mo = np.eye(4)
                Mo[:3, :3], Mo[:3, 3] = M32[k, t, :9].astype(np.float64).reshape(3, 3), M32[k, t, 9:].astype(np.float64)
                G = Mo @ G
                ok = ok and bool(v2[k, t])
            pose[k, t, :9], pose[k, t, 9:] = G[:3, :3].reshape(-1), G[:3, 3]
            pose_valid[k, t] = ok
            inv[k, t, :9], inv[k, t, 9:] = G[:3, :3].T.reshape(-1), -(G[:3, :3].T @ G[:3, 3])
    pts = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3).astype(np.float64)
    canonical = np.full((T * H * W, 3), np.nan, dtype=F32)
    mm = np.nonzero(on.reshape(-1))[0]
    gi = inv[ids.reshape(-1)[mm], mm // (H * W)]
    with np.errstate(all="ignore"):
        canonical[mm] = (np.einsum("nij,nj->ni", gi[:, :9].reshape(-1, 3, 3), pts[mm]) + gi[:, 9:]).astype(F32)
    sh = (K, T)
    return dict(motion=model32.reshape(K, T, 12), motion64=model.reshape(K, T, 12), n_pairs=n.astype(np.int32).reshape(sh),
                n_inliers=mom[:, 0].astype(np.int32).reshape(sh), n_far=n_far.astype(np.int32).reshape(sh), rms=rms.reshape(sh),
                valid=v2, moments=mom.reshape(K, T, 18), pose=pose, pose_valid=pose_valid, canonical=canonical,
                ratio=ratio.reshape(sh), margin=margin, AB=AB.reshape(K, T, 2, 3), extent_d=ext.reshape(sh), pairs=pr, cen=cen)


# ------------------------------------------------------------------------------------------------------------------------------
# Clips.  Every builder returns dict(object_id [T, H, W] int32, K, points [T H W, 3] f32, grid [4] f32, flow [2, T, H, W] f32 or None).
# ------------------------------------------------------------------------------------------------------------------------------
GRID = np.array([0.1, -0.2, 0.3, 0.05], dtype=F32)


def random_case(seed, T, H, W, bad=True):
    """A ``random_case`` clip of the moving-objects restatement, labelled by that restatement, with random points (N(0, 2)); with
    ``bad`` a few NaN / Inf points (the flow of that clip carries NaN already)."""
    c = RS.random_case(seed, T, H, W)
    lab = RS.label(c["mask"], None, c["flow"], None)
    g = np.random.default_rng(1000 + seed)
    pts = g.normal(0, 2, (T * H * W, 3)).astype(F32)
    if bad:
        hit = g.random(len(pts)) < 0.06
        pts[hit, g.integers(0, 3, int(hit.sum()))] = g.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), int(hit.sum()))
    return dict(object_id=lab["object_id"], K=lab["K"], points=pts, grid=GRID.copy(), flow=c["flow"])


def _near_rigid_points(g, T, H, W, outliers=0.15):
    """A curved sheet over the pixel grid, turned and shifted a little per frame, plus noise of a tenth of a voxel; the share
    ``outliers`` of the points is thrown 0.4 .. 0.8 off (8 to 16 voxels of GRID) in a random direction, so that the refit has pairs
    to reject and none of them near its threshold of two voxels."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([0.03 * xx, 0.03 * yy, 2.0 + 0.4 * np.sin(0.09 * xx) * np.cos(0.13 * yy)], axis=-1).reshape(-1, 3)
    pts = np.stack([(base @ rot([0.2, 1.0, -0.3], 0.04 * t).T + np.array([0.05, -0.02, 0.03]) * t) for t in range(T)])
    pts = pts + g.normal(0, 0.005, pts.shape)
    d = g.normal(0, 1, pts.shape)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * g.uniform(0.4, 0.8, pts.shape[:-1] + (1,))
    return np.where(g.random(pts.shape[:-1] + (1,)) < outliers, pts + d, pts).reshape(-1, 3).astype(F32)


def serpentine_case(T=3, H=41, W=150, seed=5):
    """The serpentine of the moving-objects restatement (one object through the whole frame, every frame) on near-rigid points."""
    c = RS.serpentine(T, H, W)
    lab = RS.label(c["mask"])
    pts = _near_rigid_points(np.random.default_rng(seed), T, H, W)
    return dict(object_id=lab["object_id"], K=lab["K"], points=pts, grid=GRID.copy(), flow=None)


def straddle_case(T=3, H=5, W=200, seed=9):
    """Two objects whose runs of pixels cross the 64-lane and the 256-thread boundaries of the pixel launches (W is no multiple of
    64): object 0 on columns 50 .. 139 of every row, object 1 on columns 140 .. 179 and, in stripes of three pixels, inside
    object 0's columns on the odd rows - runs of one (object, frame) of length 3 to 90 that start and end at every phase.  Near-rigid
    points."""
    ids = np.full((T, H, W), -1, dtype=np.int32)
    ids[:, :, 50:140] = 0
    ids[:, :, 140:180] = 1
    stripes = (np.arange(W) // 3) % 2 == 1
    ids[:, 1::2, :] = np.where(stripes[None, None, :] & (ids[:, 1::2, :] == 0), 1, ids[:, 1::2, :])
    pts = _near_rigid_points(np.random.default_rng(seed), T, H, W)
    return dict(object_id=ids, K=2, points=pts, grid=GRID.copy(), flow=None)


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


RIGID = dict(T=4, H=40, W=64, h=20, w=24, start=(3, 2), step=(9, 5), spacing=0.03)
RIGID_ANGLES = (0.0, 0.06, 0.35, 0.6)  # radians from frame 0: steps of 3.4, 16.6 and 14.3 degrees
RIGID_AXES = ([0.3, -1.0, 0.45], [1.0, 0.2, -0.1], [0.0, 0.3, 1.0])
RIGID_SHIFT = np.array([0.31, -0.12, 0.23])


def rigid_poses():
    """G_t [T, 4, 4] float64 of ``rigid_scene``: G_0 = I, then a turn about a different axis and a shift per frame."""
    G = [np.eye(4)]
    for t in range(1, RIGID["T"]):
        S = np.eye(4)
        S[:3, :3] = rot(RIGID_AXES[t - 1], RIGID_ANGLES[t] - RIGID_ANGLES[t - 1])
        S[:3, 3] = RIGID_SHIFT * (1 + 0.25 * t) - S[:3, :3] @ np.array([0.3, 0.25, 2.0]) + np.array([0.3, 0.25, 2.0])  # turn about the body
        G.append(S @ G[-1])
    return np.stack(G)


def rigid_scene(corrupt=0.0, seed=3):
    """A h x w rectangle of object pixels that moves by ``step`` pixels per frame, with integer flow -step on it.  Local pixel
    (u, v) owns the canonical point c(u, v) on a curved, non-planar sheet; its world point in frame t is G_t c(u, v), so the pairs
    are exact correspondences and the true motion of row (0, t) is G_t G_(t-1)^-1.  The background is a far plane.  With
    ``corrupt`` that share of the object's pixels of every frame t >= 1 (seeded) has its flow redirected by half the rectangle's
    width, to another pixel of the same object: a wrong correspondence 12 pixels = 0.36 world units = 7.2 voxels off.  Also
    returns ``G`` [T, 4, 4] and ``true`` [T, 12] (row 0 = identity)."""
    T, H, W, h, w = (RIGID[k] for k in ("T", "H", "W", "h", "w"))
    sp, G = RIGID["spacing"], rigid_poses()
    uu, vv = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")  # [h, w]
    canon = np.stack([sp * uu, sp * vv, 2.0 + 0.25 * np.sin(0.31 * uu) * np.cos(0.23 * vv) + 0.004 * uu * vv / 4], axis=-1)  # [h, w, 3]
    ids = np.full((T, H, W), -1, dtype=np.int32)
    flow = np.zeros((2, T, H, W), dtype=F32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pts = np.broadcast_to(np.stack([0.05 * xx, 0.05 * yy, np.full(xx.shape, 9.0)], axis=-1), (T, H, W, 3)).copy()
    g = np.random.default_rng(seed)
    for t in range(T):
        x0, y0 = RIGID["start"][0] + t * RIGID["step"][0], RIGID["start"][1] + t * RIGID["step"][1]
        ids[t, y0:y0 + h, x0:x0 + w] = 0
        pts[t, y0:y0 + h, x0:x0 + w] = canon @ G[t, :3, :3].T + G[t, :3, 3]
        fx = np.full((h, w), -float(RIGID["step"][0]))
        if corrupt > 0 and t >= 1:
            hit = g.random((h, w)) < corrupt
            fx = np.where(hit, fx + np.where(uu < w // 2, w // 2, -(w // 2)), fx)
        flow[0, t, y0:y0 + h, x0:x0 + w], flow[1, t, y0:y0 + h, x0:x0 + w] = fx, -float(RIGID["step"][1])
    true = np.tile(EYE12, (T, 1))
    for t in range(1, T):
        S = G[t] @ np.linalg.inv(G[t - 1])
        true[t, :9], true[t, 9:] = S[:3, :3].reshape(-1), S[:3, 3]
    return dict(object_id=ids, K=1, points=pts.reshape(-1, 3).astype(F32), grid=np.array([0, 0, 0, 0.05], dtype=F32), flow=flow, G=G,
                true=true, colors=g.integers(0, 256, (T * H * W, 3)).astype(np.uint8))


def motion_error(model, true):
    """(largest entrywise error of R, largest error of t) of models [..., 12] against ``true``."""
    d = np.abs(np.asarray(model, dtype=np.float64) - true)
    return float(d[..., :9].max()), float(d[..., 9:].max())


EDGE_OBJECTS = dict(full=0, few=1, late=2, far=3)


def edge_case(seed=21):
    """(5, 12, 40), four still objects on near-rigid points without outliers: ``full`` a 6 x 6 square in every frame (36 pairs);
    ``few`` 2 x 3 pixels (6 pairs: below min_pairs); ``late`` a 5 x 5 square first seen in frame 2; ``far`` a 5 x 5 square two of
    whose points lie 1000 units off along x in every frame (4.7e6 fixed-point steps from the centre they drag along by 4.1e5)."""
    T, H, W = 5, 12, 40
    ids = np.full((T, H, W), -1, dtype=np.int32)
    ids[:, 1:7, 1:7] = EDGE_OBJECTS["full"]
    ids[:, 1:3, 10:13] = EDGE_OBJECTS["few"]
    ids[2:, 5:10, 15:20] = EDGE_OBJECTS["late"]
    ids[:, 2:7, 30:35] = EDGE_OBJECTS["far"]
    pts = _near_rigid_points(np.random.default_rng(seed), T, H, W, outliers=0.0).reshape(T, H, W, 3)
    pts[:, 3, 31, 0] += 1000.0
    pts[:, 5, 33, 0] += 1000.0
    return dict(object_id=ids, K=4, points=pts.reshape(-1, 3), grid=GRID.copy(), flow=None)


def gpu_cases():
    """name -> (clip, keyword arguments of ``rigid_motion``): every clip the GPU tests run, so that the CPU tests can assert of each
    one that its valid rows are well conditioned and that no residual sits near the inlier threshold."""
    c = {}
    for name, clip in (("ragged_3x5x7", random_case(1, 3, 5, 7)), ("ragged_4x13x17", random_case(2, 4, 13, 17))):
        for flow in (True, False):
            for n_refits in (0, 1):
                c[f"{name}_{'flow' if flow else 'noflow'}_refits{n_refits}"] = (
                    dict(clip, flow=clip["flow"] if flow else None), dict(min_pairs=3, n_refits=n_refits))
    snake = serpentine_case()
    g = np.random.default_rng(77)
    T, H, W = snake["object_id"].shape
    jitter = g.integers(-1, 2, (2, T, H, W)).astype(F32)
    jitter[:, g.random((T, H, W)) < 0.03] = np.nan
    bad = snake["points"].copy()
    bad[g.random(len(bad)) < 0.03] = np.nan
    bad[g.random(len(bad)) < 0.01] = np.inf
    c["serpentine_noflow"] = (snake, {})
    c["serpentine_flow_bad_points"] = (dict(snake, flow=jitter, points=bad), {})
    c["straddle"] = (straddle_case(), {})
    c["straddle_two_refits"] = (straddle_case(), dict(n_refits=2, inlier_voxels=1.5))
    c["one_frame"] = (random_case(3, 1, 9, 11), dict(min_pairs=3))
    c["edge"] = (edge_case(), {})
    c["rigid"] = (rigid_scene(), {})
    c["rigid_corrupted"] = (rigid_scene(corrupt=CORRUPT_SHARE), {})
    return c


CORRUPT_SHARE = 0.1


def big_sums_case(seed=8):
    """(2, 1024, 1024), one still object on every pixel, no flow: 2^20 pairs, the most a row may hold, a quarter each at four
    corners (+, +, +), (+, -, -), (-, +, -), (-, -, +) of a cube of half side 2^21 - 4 fixed-point steps about the origin (grid
    (0, 0, 0, 256): one step is one unit and a point s + 0.5 is exact in f32), frame 1 = frame 0 turned a quarter about z and moved by
    -1, 0 or 1 steps per axis (seeded).  Centres 0 or -1, no pair far, and each sum of squares is 3 * 2^20 * (2^21 - 4)^2 or so: past
    2^63.  The singular values of the covariance are equal; it is a multiple of a rotation, so R is still unique."""
    H = W = 1024
    g = np.random.default_rng(seed)
    c = float((1 << 21) - 4)
    corners = np.array([[c, c, c], [c, -c, -c], [-c, c, -c], [-c, -c, c]])
    a = corners[np.arange(H * W) % 4]
    b = np.stack([-a[:, 1], a[:, 0], a[:, 2]], axis=1) + g.integers(-1, 2, a.shape)
    pts = (np.concatenate([a, b]) + 0.5).astype(F32)
    assert np.array_equal(pts.astype(np.float64), np.concatenate([a, b]) + 0.5)
    return dict(object_id=np.zeros((2, H, W), dtype=np.int32), K=1, points=pts, grid=np.array([0, 0, 0, 256], dtype=F32), flow=None)
