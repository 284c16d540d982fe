"""numpy restatement of the moving-object stage (include/l4p_hip.h "Moving objects", csrc/objects.hip) and the clips of its tests.

``label`` follows the header's rule operation by operation: the foreground, the edge list (spatial edges with the depth gate in f32,
temporal edges through the flow rounded in f32), a plain union-find over that list, labels = the smallest member, numbering by
ascending label.  ``tables``, ``tracks`` and ``overlay`` restate the rest: integer sums, f64 centroids with one rounding per
operation, f32 steps.  Nothing here is approximate, so the GPU tests compare bits."""
import numpy as np

F32 = np.float32
COUNTERS = ("n_pixels", "n_foreground", "n_components", "n_kept", "n_kept_pixels", "n_guard")
LABEL_FIELDS = ("object_id", "label", "root", "n_pixels", "first_frame", "last_frame")
TABLES_2D = ("count", "bbox", "centroid_px")
TABLES_3D = ("count3d", "centroid_xyz", "box3d", "step", "speed")
TRACK_FIELDS = ("track_object_nt", "track_object", "votes")
DTYPES = dict(object_id=np.int32, label=np.int32, root=np.int32, n_pixels=np.int32, first_frame=np.int32, last_frame=np.int32,
              count=np.int32, bbox=np.int32, centroid_px=F32, count3d=np.int32, centroid_xyz=F32, box3d=F32, step=F32, speed=F32,
              track_object_nt=np.int32, track_object=np.int32, votes=np.int32)


def foreground(mask, depth=None, keep=None):
    with np.errstate(invalid="ignore"):
        fg = np.asarray(mask, dtype=F32) > 0  # NaN > 0 is False
        if keep is not None:
            fg &= np.asarray(keep) != 0
        if depth is not None:
            d = np.asarray(depth, dtype=F32)
            fg &= np.isfinite(d) & (d > 0)
    return fg


def edges(fg, depth=None, flow=None, connectivity=8, max_depth_ratio=0.0):
    """(a, b) int64 arrays: the linear indices of the two ends of every edge."""
    T, H, W = fg.shape
    idx = np.arange(T * H * W, dtype=np.int64).reshape(T, H, W)
    ratio = F32(max_depth_ratio)
    d = None if depth is None else np.asarray(depth, dtype=F32)
    ea, eb = [], []
    offsets = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for dy, dx in offsets:
        ys = slice(1, H) if dy else slice(0, H)  # the pixel
        yn = slice(0, H - 1) if dy else slice(0, H)  # its neighbour
        xs, xn = {-1: (slice(1, W), slice(0, W - 1)), 0: (slice(0, W), slice(0, W)), 1: (slice(0, W - 1), slice(1, W))}[dx]
        on = fg[:, ys, xs] & fg[:, yn, xn]
        if d is not None and not ratio <= 0:
            da, db = d[:, ys, xs], d[:, yn, xn]
            with np.errstate(invalid="ignore"):
                gate = np.maximum(da, db) <= ratio * np.minimum(da, db)  # f32 product; both depths are finite where `on`
            on = on & gate
        ea.append(idx[:, ys, xs][on]), eb.append(idx[:, yn, xn][on])
    if T > 1:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        for t in range(1, T):
            on = fg[t].copy()
            yq, xq = yy, xx
            if flow is not None:
                u, v = np.asarray(flow[0][t], dtype=F32), np.asarray(flow[1][t], dtype=F32)
                with np.errstate(invalid="ignore", over="ignore"):
                    gx = np.floor((xx.astype(F32) + u) + F32(0.5))
                    gy = np.floor((yy.astype(F32) + v) + F32(0.5))
                    assert gx.dtype == F32 and gy.dtype == F32
                    inside = (gx >= 0) & (gx < F32(W)) & (gy >= 0) & (gy < F32(H))
                on &= np.isfinite(u) & np.isfinite(v) & inside
                xq = np.where(on, gx, 0).astype(np.int64)
                yq = np.where(on, gy, 0).astype(np.int64)
            on = on & fg[t - 1][yq, xq]
            ea.append(idx[t][on]), eb.append(idx[t - 1][yq, xq][on])
    return np.concatenate(ea), np.concatenate(eb)


def components(n, a, b, members):
    """Plain union-find over the edge list; returns root [n] = the smallest index of the component of every index in ``members``
    (-1 elsewhere)."""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in zip(a.tolist(), b.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    root = np.full(n, -1, dtype=np.int64)
    for i in members.tolist():
        root[i] = find(i)
    return root


def label(mask, depth=None, flow=None, keep=None, connectivity=8, max_depth_ratio=0.0, min_pixels=1, min_frames=1):
    """The result of ``label_components`` as host arrays: LABEL_FIELDS, ``counters`` and, for all components before filtering,
    ``all`` = dict(root, n_pixels, first_frame, last_frame, kept)."""
    mask = np.asarray(mask, dtype=F32)
    T, H, W = mask.shape
    M, HW = T * H * W, H * W
    fg = foreground(mask, depth, keep)
    a, b = edges(fg, depth, flow, connectivity, max_depth_ratio)
    members = np.nonzero(fg.reshape(-1))[0]
    lab = components(M, a, b, members)
    roots, inv, npix = np.unique(lab[members], return_inverse=True, return_counts=True)  # ascending label
    inv = inv.reshape(-1)
    first = roots // HW
    last = np.zeros(len(roots), dtype=np.int64)
    np.maximum.at(last, inv, members // HW)
    kept = (npix >= min_pixels) & (last - first + 1 >= min_frames)
    number = np.where(kept, np.cumsum(kept) - 1, -1)
    object_id = np.full(M, -1, dtype=np.int64)
    object_id[members] = number[inv]
    k = np.nonzero(kept)[0]
    counters = dict(n_pixels=M, n_foreground=int(len(members)), n_components=int(len(roots)), n_kept=int(len(k)),
                    n_kept_pixels=int(npix[k].sum()), n_guard=0)
    i32 = np.int32
    return dict(object_id=object_id.astype(i32).reshape(T, H, W), label=lab.astype(i32).reshape(T, H, W), root=roots[k].astype(i32),
                n_pixels=npix[k].astype(i32), first_frame=first[k].astype(i32), last_frame=last[k].astype(i32), counters=counters,
                K=int(len(k)), all=dict(root=roots, n_pixels=npix, first_frame=first, last_frame=last, kept=kept))


def _fkey(x):
    """The integer whose order is the floats' order, -0 below +0."""
    i = np.ascontiguousarray(x, dtype=F32).view(np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF))


def tables(object_id, K, points=None, grid=None):
    ids = np.asarray(object_id)
    T, H, W = ids.shape
    tt, yy, xx = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    on = (ids >= 0) & (ids < K)
    row = (ids[on].astype(np.int64) * T + tt[on])
    R = K * T
    count = np.bincount(row, minlength=R).astype(np.int64)
    sx = np.zeros(R, dtype=np.int64)
    sy = np.zeros(R, dtype=np.int64)
    np.add.at(sx, row, xx[on]), np.add.at(sy, row, yy[on])
    big = np.iinfo(np.int64).max
    x0, y0 = np.full(R, big), np.full(R, big)
    x1, y1 = np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
    np.minimum.at(x0, row, xx[on]), np.minimum.at(y0, row, yy[on]), np.maximum.at(x1, row, xx[on]), np.maximum.at(y1, row, yy[on])
    any_ = count > 0
    bbox = np.stack([np.where(any_, x0, 0), np.where(any_, y0, 0), x1, y1], axis=1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        cpx = np.stack([sx.astype(np.float64) / count.astype(np.float64), sy.astype(np.float64) / count.astype(np.float64)], axis=1)
    cpx = np.where(any_[:, None], cpx, 0.0).astype(F32)
    res = dict(count=count.astype(np.int32).reshape(K, T), bbox=bbox.reshape(K, T, 4), centroid_px=cpx.reshape(K, T, 2))
    if points is None:
        return res
    p = np.ascontiguousarray(points, dtype=F32).reshape(T, H, W, 3)[on]
    g = np.asarray(grid, dtype=F32).reshape(4)
    v = g[3]
    ok = np.isfinite(p).all(axis=1)
    s = np.zeros(p.shape, dtype=F32)
    if v > 0 and np.isfinite(v):
        with np.errstate(all="ignore"):
            q = (p - g[None, :3]) / v
            s = np.floor(q * F32(256.0))
            assert q.dtype == F32 and s.dtype == F32
            ok &= ((s >= F32(-(1 << 28))) & (s < F32(1 << 28))).all(axis=1)  # NaN fails
    else:
        ok[:] = False
    r3 = row[ok]
    n = np.bincount(r3, minlength=R).astype(np.int64)
    s3 = np.zeros((R, 3), dtype=np.int64)
    np.add.at(s3, r3, s[ok].astype(np.int64))
    lo = np.full((R, 3), np.iinfo(np.int32).max, dtype=np.int32)
    hi = np.full((R, 3), np.iinfo(np.int32).min, dtype=np.int32)
    key = _fkey(p[ok])
    np.minimum.at(lo, r3, key), np.maximum.at(hi, r3, key)
    unkey = lambda k: np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(F32)  # noqa: E731
    has = n > 0
    nd = n.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (s3.astype(np.float64) + 0.5 * nd) / (nd * 256.0)
        cen = (g[None, :3].astype(np.float64) + f * np.float64(v)).astype(F32)
    cen = np.where(has[:, None], cen, F32(0)).astype(F32).reshape(K, T, 3)
    box = np.where(has[:, None], np.concatenate([unkey(lo), unkey(hi)], axis=1), F32(0)).astype(F32)
    has = has.reshape(K, T)
    step = np.zeros((K, T, 3), dtype=F32)
    both = has[:, 1:] & has[:, :-1]
    with np.errstate(all="ignore"):
        step[:, 1:] = np.where(both[:, :, None], cen[:, 1:] - cen[:, :-1], F32(0))
        speed = np.sqrt((step[..., 0] * step[..., 0] + step[..., 1] * step[..., 1]) + step[..., 2] * step[..., 2])
    assert step.dtype == F32 and speed.dtype == F32
    res.update(count3d=n.astype(np.int32).reshape(K, T), centroid_xyz=cen, box3d=box.reshape(K, T, 6), step=step, speed=speed)
    return res


def tracks(object_id, traj, vis):
    ids = np.asarray(object_id)
    T, H, W = ids.shape
    traj, vis = np.asarray(traj, dtype=F32), np.asarray(vis, dtype=F32)
    N = traj.shape[0]
    x, y = traj[:, 0], traj[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        gx, gy = np.floor(x + F32(0.5)), np.floor(y + F32(0.5))
        on = (vis > 0) & np.isfinite(x) & np.isfinite(y) & (gx >= 0) & (gx < F32(W)) & (gy >= 0) & (gy < F32(H))
    xi, yi = np.where(on, gx, 0).astype(np.int64), np.where(on, gy, 0).astype(np.int64)
    tt = np.broadcast_to(np.arange(T)[None], (N, T))
    nt = np.where(on, ids[tt, yi, xi], -1).astype(np.int32)
    best, votes = np.full(N, -1, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for n in range(N):
        got = nt[n][nt[n] >= 0]
        if len(got):
            c = np.bincount(got)
            best[n], votes[n] = int(np.argmax(c)), int(c.max())  # argmax: the first, the smallest id
    return dict(track_object_nt=nt, track_object=best, votes=votes)


def overlay(frames, object_id, lut, alpha):
    f = np.asarray(frames, dtype=np.uint8)
    ids = np.asarray(object_id)
    on = (ids >= 0) & (ids < len(lut))
    out = f.copy()
    col = np.asarray(lut, dtype=np.int64).reshape(-1, 3)[ids[on]]
    out[on] = ((f[on].astype(np.int64) * (256 - alpha) + col * alpha + 128) >> 8).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# Clips.  A mask is logits: +2 foreground, -2 background.
# ------------------------------------------------------------------------------------------------------------------------------
TILE_W, TILE_H = 64, 16  # OB_TW, OB_TH of csrc/objects.hip: what "a little over two tiles" means


def logits(fg):
    return np.where(fg, F32(2), F32(-2)).astype(F32)


def random_case(seed, T, H, W, p=0.45):
    """Random mask, positive depths in [1, 3] with a few bad ones, flow of a few pixels with a few NaN, a keep plane."""
    g = np.random.default_rng(seed)
    mask = g.normal(0.0, 1.0, (T, H, W)).astype(F32) + F32(np.log(p / (1 - p)))
    mask[g.random((T, H, W)) < 0.02] = np.nan
    depth = g.uniform(1.0, 3.0, (T, H, W)).astype(F32)
    bad = g.random((T, H, W)) < 0.04
    depth[bad] = g.choice(np.array([0.0, -1.0, np.nan, np.inf], dtype=F32), int(bad.sum()))
    flow = g.integers(-3, 4, (2, T, H, W)).astype(F32) + g.choice(np.array([0.0, 0.25, 0.5, -0.5], dtype=F32), (2, T, H, W))
    flow[:, g.random((T, H, W)) < 0.03] = np.nan
    keep = (g.random((T, H, W)) > 0.05).astype(np.uint8)
    mask[0, 0, 1], depth[0, 2, 2], keep[0, 1, 1] = np.nan, np.nan, 0  # at least one of each, whatever the seed drew
    flow[:, T - 1, 1, 2] = np.nan
    return dict(mask=mask, depth=depth, flow=flow, keep=keep)


def serpentine(T, H, W, mirrored=False):
    """A one-pixel-wide snake through the whole frame, the same in every frame: every even row in full, and on the odd rows one
    pixel that joins it to the next even row, at the right end after rows 0, 4, 8, ... and at the left end after rows 2, 6, ...
    Its smallest index is pixel (0, 0, 0), one end of the snake; mirrored left to right the snake starts at (0, 0, W - 1) and its
    smallest index is the far end of row 0."""
    fg = np.zeros((H, W), dtype=bool)
    fg[0::2] = True
    for y in range(1, H - 1, 2):
        fg[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    if mirrored:
        fg = fg[:, ::-1]
    return dict(mask=logits(np.broadcast_to(fg, (T, H, W)).copy()))


def checkerboard(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return dict(mask=logits(((yy + xx) % 2 == 0)[None]))


def moving_square(T=4, H=20, W=30, step=(5, 3), size=4, start=(2, 1)):
    """A size x size square at (x, y) = start + t step; ``flow`` = -step on its pixels (the backward flow of that motion), 0 elsewhere."""
    fg = np.zeros((T, H, W), dtype=bool)
    flow = np.zeros((2, T, H, W), dtype=F32)
    for t in range(T):
        x, y = start[0] + t * step[0], start[1] + t * step[1]
        fg[t, y:y + size, x:x + size] = True
        flow[0, t, y:y + size, x:x + size] = -step[0]
        flow[1, t, y:y + size, x:x + size] = -step[1]
    return dict(mask=logits(fg), flow=flow, fg=fg)


def two_rectangles(H=12, W=20):
    """Two overlapping rectangles, the front one at depth 1 and the back one at depth 3, one frame."""
    fg = np.zeros((1, H, W), dtype=bool)
    depth = np.full((1, H, W), 5.0, dtype=F32)
    fg[0, 2:9, 2:12] = True
    depth[0, 2:9, 2:12] = 3.0
    fg[0, 5:11, 8:18] = True
    depth[0, 5:11, 8:18] = 1.0
    return dict(mask=logits(fg), depth=depth, fg=fg)


def blobs():
    """Five blobs on a (6, 24, 40) clip that first appear in frames 0, 0, 1, 2, 4, with 9, 4, 12, 2 and 6 pixels per frame and
    6, 1, 5, 2 and 2 frames."""
    T, H, W = 6, 24, 40
    fg = np.zeros((T, H, W), dtype=bool)
    fg[:, 2:5, 3:6] = True  # 9 pixels, all 6 frames
    fg[0, 10:12, 30:32] = True  # 4 pixels, frame 0 only
    fg[1:, 15:18, 10:14] = True  # 12 pixels, frames 1..5
    fg[2:4, 20, 33:35] = True  # 2 pixels, frames 2, 3
    fg[4:, 8:10, 20:23] = True  # 6 pixels, frames 4, 5
    return dict(mask=logits(fg), fg=fg)


def dyadic_plane(T=4, H=64, W=64):
    """All foreground; point (t, y, x) = (x / 8, y / 8, 2 + t / 4): every number dyadic, grid (0, 0, 0, 0.5)."""
    tt, yy, xx = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    pts = np.stack([xx / 8.0, yy / 8.0, 2.0 + tt / 4.0], axis=-1).astype(F32).reshape(-1, 3)
    return dict(mask=logits(np.ones((T, H, W), dtype=bool)), points=pts, grid=np.array([0, 0, 0, 0.5], dtype=F32))
