"""numpy restatement of the static scene map (include/l4p_hip.h "Static scene map", csrc/static_map.hip) and a seeded scene generator.

``restate`` follows the header's rule operation by operation: f32 for q, i and f; int64 keys and sums; np.unique ordered by first
index for the output order; f64 for the emitted position, one rounding per operation.  Nothing here is approximate, so the GPU
tests compare bits.

``make_scene``: a textured plane and a static box seen by a camera that translates and turns a little per frame, with a sphere that
moves across the view and that the motion mask covers.  It returns the frame-major world points an engine would hand to the map."""
import numpy as np

COUNTERS = ("n_points", "n_used", "n_nonfinite", "n_masked", "n_out_of_range", "n_voxels", "n_kept", "n_overflow")
FIELDS = ("xyz", "colors", "count", "n_frames", "first_frame", "last_frame", "first_point", "key", "voxel_id")
LO, HI = -(1 << 20), (1 << 20) - 1


def keys_of(points, grid, mask=None, keep=None):
    """(status [M] int: 0 used, 1 non-finite, 2 masked, 3 out of range; key [M] int64; f [M, 3] int64), f32 arithmetic."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    g = np.asarray(grid, dtype=np.float32).reshape(4)
    M = p.shape[0]
    status = np.zeros(M, dtype=np.int64)
    finite = np.isfinite(p).all(axis=1)
    status[~finite] = 1
    masked = np.zeros(M, dtype=bool)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            masked |= np.asarray(mask, dtype=np.float32).reshape(M) > 0  # NaN > 0 is False
    if keep is not None:
        masked |= np.asarray(keep).reshape(M) == 0
    status[finite & masked] = 2
    live = status == 0
    v = g[3]
    key = np.zeros(M, dtype=np.int64)
    f = np.zeros((M, 3), dtype=np.int64)
    if not (v > 0 and np.isfinite(v)):
        status[live] = 3
        return status, key, f
    with np.errstate(all="ignore"):
        q = (p - g[None, :3]) / v  # f32 - f32, f32 / f32
        i = np.floor(q)
        assert q.dtype == np.float32 and i.dtype == np.float32
        inside = ((i >= np.float32(LO)) & (i <= np.float32(HI))).all(axis=1)  # NaN fails
        status[live & ~inside] = 3
        ok = status == 0
        fr = np.floor((q[ok] - i[ok]) * np.float32(65536.0))
        assert fr.dtype == np.float32
    f[ok] = fr.astype(np.int64)
    assert f.min() >= 0 and f.max() <= 65535
    ii = i[ok].astype(np.int64) + (1 << 20)
    key[ok] = ii[:, 0] | (ii[:, 1] << 21) | (ii[:, 2] << 42)
    return status, key, f


def restate(points, colors, T, grid, mask=None, keep=None, min_frames=2, min_points=1):
    """The map of ``fuse_points`` as host arrays: the FIELDS, ``counters`` (dict of ints, n_overflow 0: the restatement has no
    table) and, for all voxels before filtering, ``all`` = dict(key, count, n_frames, first_point, kept)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    g = np.asarray(grid, dtype=np.float32).reshape(4)
    M = p.shape[0]
    assert M % T == 0
    HW = M // T
    status, key, f = keys_of(p, g, mask, keep)
    used = np.nonzero(status == 0)[0]
    uk, first, inv, count = np.unique(key[used], return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")  # voxels by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    vox = rank[inv]  # voxel (in output order, before filtering) of every used point
    nv = len(uk)
    vkey, vcount, vfirst = uk[order], count[order].astype(np.int64), used[first[order]]
    sum_f = np.zeros((nv, 3), dtype=np.int64)
    sum_c = np.zeros((nv, 3), dtype=np.int64)
    np.add.at(sum_f, vox, f[used])
    np.add.at(sum_c, vox, c[used].astype(np.int64))
    frame = used // HW
    pairs = np.unique(vox * T + frame)  # distinct (voxel, frame)
    n_frames = np.bincount(pairs // T, minlength=nv).astype(np.int64)
    last = np.full(nv, -1, dtype=np.int64)
    np.maximum.at(last, vox, frame)
    kept = (n_frames >= min_frames) & (vcount >= min_points)
    out_idx = np.where(kept, np.cumsum(kept) - 1, -1)
    voxel_id = np.full(M, -1, dtype=np.int32)
    voxel_id[used] = out_idx[vox]
    k = np.nonzero(kept)[0]
    cnt = vcount[k].astype(np.float64)[:, None]
    idx = np.stack([((vkey[k] >> s) & 0x1FFFFF) - (1 << 20) for s in (0, 21, 42)], axis=1).astype(np.float64)
    fr = (sum_f[k].astype(np.float64) + 0.5 * cnt) / (cnt * 65536.0)
    xyz = (g[None, :3].astype(np.float64) + (idx + fr) * np.float64(g[3])).astype(np.float32)
    rgb = ((2 * sum_c[k] + vcount[k][:, None]) // (2 * vcount[k][:, None])).astype(np.uint8)
    counters = dict(n_points=M, n_used=int(len(used)), n_nonfinite=int((status == 1).sum()), n_masked=int((status == 2).sum()),
                    n_out_of_range=int((status == 3).sum()), n_voxels=int(nv), n_kept=int(len(k)), n_overflow=0)
    i32 = np.int32
    return dict(xyz=xyz.reshape(-1, 3), colors=rgb.reshape(-1, 3), count=vcount[k].astype(i32), n_frames=n_frames[k].astype(i32),
                first_frame=(vfirst[k] // HW).astype(i32), last_frame=last[k].astype(i32), first_point=vfirst[k].astype(i32),
                key=vkey[k].astype(np.int64), voxel_id=voxel_id, counters=counters,
                all=dict(key=vkey, count=vcount, n_frames=n_frames, first_point=vfirst, kept=kept))


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def make_scene(seed, T, H, W):
    """dict(points [T H W, 3] f32, colors [T H W, 3] u8, mask [T H W] f32 logits, mover [T H W] bool, px: the world size of a pixel
    at the plane).  The plane z = 4 behind everything, the box [-0.6, 0.1] x [-0.3, 0.5] x [2.6, 3.2], a sphere of radius 0.35 at
    depth 2.2 that crosses the view; camera t at (0.04 t, 0.01 t, 0) turned by 0.01 t about y.  Colours are a texture of the WORLD
    position (8 levels per channel), so one surface point keeps its colour across frames; the mask logit is +2 on the sphere and -2
    elsewhere, plus seeded noise below 1."""
    rng = np.random.default_rng(seed)
    fx = 1.1 * max(H, W)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays_c = np.stack([(ii - (W - 1) / 2) / fx, (jj - (H - 1) / 2) / fx, np.ones_like(ii)], axis=-1).reshape(-1, 3)
    b0, b1 = np.array([-0.6, -0.3, 2.6]), np.array([0.1, 0.5, 3.2])
    pts, cols, mask, mover = [], [], [], []
    for t in range(T):
        R, o = _rot_y(0.01 * t), np.array([0.04 * t, 0.01 * t, 0.0])
        d = rays_c @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            s_plane = (4.0 - o[2]) / d[:, 2]
            lo, hi = (b0 - o) / d, (b1 - o) / d
            near, far = np.minimum(lo, hi).max(axis=1), np.maximum(lo, hi).min(axis=1)
        s_box = np.where((near <= far) & (near > 0), near, np.inf)
        cs = np.array([-0.9 + 1.8 * t / max(T - 1, 1), -0.1, 2.2])
        oc = o - cs
        bq = d @ oc
        disc = bq * bq - (d * d).sum(axis=1) * (oc @ oc - 0.35 ** 2)
        with np.errstate(invalid="ignore"):
            s_sph = np.where(disc > 0, (-bq - np.sqrt(np.maximum(disc, 0))) / (d * d).sum(axis=1), np.inf)
        s_sph = np.where(s_sph > 0, s_sph, np.inf)
        s = np.minimum(np.minimum(s_plane, s_box), s_sph)
        X = o + s[:, None] * d
        on_sphere = s_sph <= s
        cell = np.floor(X * 7.0).astype(np.int64)
        tex = np.stack([(cell[:, 0] * 3 + cell[:, 1]) % 8, (cell[:, 1] * 5 + cell[:, 2]) % 8, (cell[:, 0] + cell[:, 2] * 3) % 8], axis=1)
        col = np.where(on_sphere[:, None], np.array([224, 32, 32]), 16 + 28 * tex)
        pts.append(X.astype(np.float32))
        cols.append(col.astype(np.uint8))
        mask.append((np.where(on_sphere, 2.0, -2.0) + rng.uniform(-0.9, 0.9, size=H * W)).astype(np.float32))
        mover.append(on_sphere)
    return dict(points=np.concatenate(pts), colors=np.concatenate(cols), mask=np.concatenate(mask), mover=np.concatenate(mover),
                px=4.0 / fx)


# ------------------------------------------------------------------------------------------------------------------------------
# The clouds of the GPU cases (tests/test_static_map_gpu.py); tests/test_static_map_cpu.py checks that each is what its name says.
# Each returns dict(points, colors, T, grid[, mask, keep]).
# ------------------------------------------------------------------------------------------------------------------------------
def scene_case(seed, T, H, W, voxel_px):
    s = make_scene(seed, T, H, W)
    return dict(points=s["points"], colors=s["colors"], T=T, grid=np.array([0, 0, 0, voxel_px * s["px"]], dtype=np.float32), mask=s["mask"])


def one_voxel_case(seed=11, T=4, HW=1024):
    """Every point inside voxel (3, -2, 7) of a grid with v = 0.5 and origin (0.25, -0.5, 1)."""
    rng = np.random.default_rng(seed)
    g = np.array([0.25, -0.5, 1.0, 0.5], dtype=np.float32)
    u = rng.uniform(0.02, 0.98, size=(T * HW, 3))
    p = (g[:3].astype(np.float64) + (np.array([3, -2, 7]) + u) * 0.5).astype(np.float32)
    return dict(points=p, colors=rng.integers(0, 256, size=(T * HW, 3), dtype=np.uint8), T=T, grid=g)


def tight_table_case(seed=12, T=4, HW=13 * 17):
    """884 points uniform over the 16^3 unit voxels of [-8, 8)^3: about 800 distinct voxels for a table of 1024 slots."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-8, 8, size=(T * HW, 3)).astype(np.float32)
    return dict(points=p, colors=rng.integers(0, 256, size=(T * HW, 3), dtype=np.uint8), T=T, grid=np.array([0, 0, 0, 1], dtype=np.float32))


def overflow_case(n=200):
    """n points in n different voxels (T = 2)."""
    p = np.stack([np.arange(n) + 0.5, np.zeros(n) + 0.5, np.ones(n) * 2.5], axis=1).astype(np.float32)
    return dict(points=p, colors=np.full((n, 3), 7, dtype=np.uint8), T=2, grid=np.array([0, 0, 0, 1], dtype=np.float32))


def frames_case(seed=13, T=4):
    """Per frame 24 points: voxels A0..A7 (x index 0..7, y index 0) get a point in every frame, B0..B7 (y index 1) in frames 0 and 2,
    and every other slot holds a voxel of its own (y index 2 + t): voxels with 1, 2 and T frames and counts 1, 2 and T."""
    rng = np.random.default_rng(seed)
    pts = []
    for t in range(T):
        u = rng.uniform(0.05, 0.95, size=(24, 3))
        idx = np.zeros((24, 3))
        idx[:, 0] = np.arange(24) % 8
        idx[:8, 1], idx[16:, 1] = 0, 2 + t
        idx[8:16, 1] = 1 if t in (0, 2) else 2 + T + t
        idx[:, 2] = -3
        pts.append((idx + u) * 0.25)
    p = np.concatenate(pts).astype(np.float32)
    return dict(points=p, colors=rng.integers(0, 256, size=(len(p), 3), dtype=np.uint8), T=T, grid=np.array([0, 0, 0, 0.25], dtype=np.float32))


def edges_case(origin=(0.0, 0.0, 0.0)):
    """Two frames of the same rows (frame 1 moved by v / 8 inside the voxel where that is exact): points on voxel faces, negative
    coordinates, -0.0, the first and last voxel index and one step outside, NaN / +-Inf rows, mask logits 0, > 0 and NaN, keep 0."""
    v = 0.5
    o = np.array(origin, dtype=np.float64)
    nan, inf = float("nan"), float("inf")
    rows = []  # (index-space position or None with a raw point, mask logit, keep)

    def at(i, j, k, logit=-1.0, keep=1):
        rows.append((o + np.array([i, j, k], dtype=np.float64) * v, logit, keep))

    def raw(x, y, z, logit=-1.0, keep=1):
        rows.append((np.array([x, y, z], dtype=np.float64), logit, keep))

    at(0, 0, 0), at(1, 0, 0), at(-1, 0, 0), at(3, -4, 5), at(-7, -7, -7)  # on faces: f = 0 on every axis
    at(0.5, 0.5, 0.5), at(-0.5, -0.25, -0.75), at(-2.125, 1.875, -0.0625)  # negative coordinates: floor, not truncation
    raw(-0.0, -0.0, -0.0), raw(0.0, -0.0, 0.0), raw(-0.0, 1.0, -1.0)
    at(-(1 << 20), 0, 0), at(0, -(1 << 20), 0), at(0, 0, -(1 << 20))  # the first index: kept
    at((1 << 20) - 1, 0, 0), at(0, (1 << 20) - 1, 0), at(0, 0, (1 << 20) - 0.5)  # the last index: kept
    at(-(1 << 20) - 1, 0, 0), at(0, (1 << 20), 0), at(0, 0, (1 << 20) + 3), raw(1e30, 0, 0), raw(0, -3e38, 0)  # out of range
    raw(nan, 0, 0), raw(0, inf, 0), raw(0, 0, -inf), raw(nan, inf, -inf), raw(nan, 0, 0, logit=5.0), raw(inf, 0, 0, keep=0)  # non-finite
    at(2, 2, 2, logit=0.0), at(2, 2, 2, logit=-0.0), at(2, 2, 2, logit=1e-45), at(2, 2, 2, logit=3.0), at(2, 2, 2, logit=inf)
    at(2, 2, 2, logit=nan), at(2, 2, 2, logit=-inf), at(4, 4, 4, keep=0), at(4, 4, 4, logit=2.0, keep=0), at(4, 4, 4)
    p0 = np.array([r[0] for r in rows]).astype(np.float32)
    p1 = p0.copy()
    small = np.abs(p0).max(axis=1) < 64  # v / 8 = 2^-4 is absorbed exactly there (the grid numbers are dyadic)
    p1[small] = p1[small] + np.float32(v / 8)
    logit = np.array([r[1] for r in rows], dtype=np.float32)
    keep = np.array([r[2] for r in rows], dtype=np.uint8)
    n = len(rows)
    rng = np.random.default_rng(14)
    return dict(points=np.concatenate([p0, p1]), colors=rng.integers(0, 256, size=(2 * n, 3), dtype=np.uint8), T=2,
                grid=np.array(list(origin) + [v], dtype=np.float32), mask=np.concatenate([logit, logit]), keep=np.concatenate([keep, keep]))
