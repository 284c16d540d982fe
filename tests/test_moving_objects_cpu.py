"""CPU: the moving-object restatement on closed-form clips, what the clips of the GPU cases are, the demo's plan with --objects and
the wrappers' argument errors, raised before any GPU work (l4p_amd/utils/moving_objects.py, tests/moving_objects_restate.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import moving_objects as MO
from tests import moving_objects_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAKE = (3, 2 * RS.TILE_H + 9, 2 * RS.TILE_W + 22)  # (3, 41, 150): a little over two tiles each way


def test_the_serpentine_is_one_component_rooted_at_its_end():
    T, H, W = SNAKE
    assert H > 2 * RS.TILE_H and W > 2 * RS.TILE_W and H % RS.TILE_H and W % RS.TILE_W
    for mirrored in (False, True):
        c = RS.serpentine(T, H, W, mirrored)
        r = RS.label(c["mask"])
        fg = c["mask"] > 0
        assert r["counters"]["n_components"] == 1 and r["counters"]["n_kept"] == 1
        assert r["n_pixels"][0] == fg.sum() > fg.sum() / 2 and r["counters"]["n_foreground"] == fg.sum()
        assert r["root"].tolist() == [0] and r["first_frame"].tolist() == [0] and r["last_frame"].tolist() == [T - 1]
        assert np.array_equal(r["label"] == 0, fg) and np.array_equal(r["object_id"] == 0, fg)
        # one pixel wide: inside one frame every pixel but the two ends has exactly two 4-neighbours, and the ends have one
        f = np.pad(fg[0], 1).astype(int)
        deg = np.where(fg[0], f[:-2, 1:-1] + f[2:, 1:-1] + f[1:-1, :-2] + f[1:-1, 2:], 0)
        assert sorted(set(deg[fg[0]].tolist())) == [1, 2] and (deg == 1).sum() == 2
        # the free end of row 0: pixel 0 itself, or (mirrored) the far end of row 0 from pixel 0
        assert [0, W - 1 if mirrored else 0] in np.argwhere(deg == 1).tolist()
        # one frame alone is the same snake
        assert RS.label(c["mask"][:1], connectivity=4)["counters"]["n_components"] == 1


def test_checkerboard_connectivity():
    c = RS.checkerboard(9, 11)
    n = int((c["mask"] > 0).sum())
    r8 = RS.label(c["mask"], connectivity=8)
    assert r8["counters"]["n_components"] == 1 and r8["n_pixels"].tolist() == [n]
    r4 = RS.label(c["mask"], connectivity=4)
    assert r4["counters"]["n_components"] == n and (r4["n_pixels"] == 1).all() and r4["K"] == n
    assert np.array_equal(r4["root"], np.nonzero(c["mask"].reshape(-1) > 0)[0])
    none = RS.label(c["mask"], connectivity=4, min_pixels=2)
    assert none["K"] == 0 and (none["object_id"] == -1).all() and none["counters"]["n_components"] == n
    t = RS.tables(none["object_id"], 0)
    assert t["count"].shape == (0, 1) and t["bbox"].shape == (0, 1, 4)


def test_temporal_linking_through_the_flow():
    c = RS.moving_square()
    still = RS.label(c["mask"])
    assert still["counters"]["n_components"] == 4 and still["n_pixels"].tolist() == [16] * 4
    assert RS.label(c["mask"], min_frames=2)["K"] == 0
    moved = RS.label(c["mask"], flow=c["flow"], min_frames=2)
    assert moved["K"] == 1 and moved["n_pixels"].tolist() == [64] and moved["first_frame"].tolist() == [0]
    assert moved["last_frame"].tolist() == [3] and np.array_equal(moved["object_id"] == 0, c["fg"])
    # NaN on all pixels of frame 2: the chain breaks there
    f = c["flow"].copy()
    f[0, 2][c["fg"][2]] = np.nan
    r = RS.label(c["mask"], flow=f)
    assert r["n_pixels"].tolist() == [32, 32] and r["first_frame"].tolist() == [0, 2]
    # NaN on all but one pixel: one edge is enough
    f = c["flow"].copy()
    ys, xs = np.nonzero(c["fg"][2])
    f[1, 2, ys[1:], xs[1:]] = np.nan
    assert RS.label(c["mask"], flow=f)["K"] == 1
    # a flow that points outside the frame links nothing
    f = c["flow"].copy()
    f[0, 1] = -100.0
    assert RS.label(c["mask"], flow=f)["n_pixels"].tolist() == [16, 48]
    # x.5 rounds up: -5.5 lands on x - 5 (still the square, one column in), -4.5 on x - 4; -6.5 on x - 6, outside it for column 0
    for dx, comps in ((-5.5, 1), (-4.5, 1)):
        f = c["flow"].copy()
        f[0][c["fg"]] = dx
        assert RS.label(c["mask"], flow=f)["counters"]["n_components"] == comps, dx
    f = c["flow"].copy()
    f[0][c["fg"]] = -8.5  # x - 8: the square's columns land on x0 - 3 .. x0: only its last column hits the square
    assert RS.label(c["mask"], flow=f)["counters"]["n_components"] == 1
    f[0][c["fg"]] = -9.5  # x0 - 4 .. x0 - 1: none does
    assert RS.label(c["mask"], flow=f)["counters"]["n_components"] == 4


def test_depth_gate_and_bad_depths():
    c = RS.two_rectangles()
    assert RS.label(c["mask"], depth=c["depth"], max_depth_ratio=1.5)["n_pixels"].tolist() == [54, 60]  # the back one less the overlap
    assert RS.label(c["mask"], depth=c["depth"], max_depth_ratio=0.0)["K"] == 1
    assert RS.label(c["mask"])["K"] == 1 and RS.label(c["mask"], depth=c["depth"], max_depth_ratio=3.0)["K"] == 1
    d = c["depth"].copy()
    bad = [(0, 3, 3, 0.0), (0, 3, 4, -1.0), (0, 4, 3, np.nan), (0, 4, 4, np.inf), (0, 6, 6, -np.inf)]
    for t, y, x, v in bad:
        d[t, y, x] = v
    r = RS.label(c["mask"], depth=d)
    assert all(r["label"][t, y, x] == -1 for t, y, x, _ in bad) and r["counters"]["n_foreground"] == c["fg"].sum() - len(bad)


def test_order_and_filters():
    c = RS.blobs()
    r = RS.label(c["mask"])
    assert r["first_frame"].tolist() == [0, 0, 1, 2, 4] and r["last_frame"].tolist() == [5, 0, 5, 3, 5]
    assert r["n_pixels"].tolist() == [54, 4, 60, 4, 12] and np.array_equal(r["root"], np.sort(r["root"]))
    assert RS.label(c["mask"], min_pixels=5)["n_pixels"].tolist() == [54, 60, 12]
    assert RS.label(c["mask"], min_frames=2)["n_pixels"].tolist() == [54, 60, 4, 12]
    both = RS.label(c["mask"], min_pixels=12, min_frames=3)
    assert both["n_pixels"].tolist() == [54, 60]
    k = both["counters"]
    assert (k["n_foreground"], k["n_components"], k["n_kept"], k["n_kept_pixels"], k["n_guard"]) == (134, 5, 2, 114, 0)
    assert sorted(set(both["object_id"].reshape(-1).tolist())) == [-1, 0, 1]
    # tables: object 1 (rows 15..17, columns 10..13) is absent from frame 0
    t = RS.tables(both["object_id"], 2)
    assert t["count"].tolist() == [[9] * 6, [0] + [12] * 5]
    assert t["bbox"][1, 0].tolist() == [0, 0, -1, -1] and t["bbox"][1, 1].tolist() == [10, 15, 13, 17]
    assert t["centroid_px"][1].tolist() == [[0, 0]] + [[11.5, 16.0]] * 5 and t["centroid_px"][0, 0].tolist() == [4.0, 3.0]


def test_the_dyadic_plane_in_closed_form():
    c = RS.dyadic_plane()
    r = RS.label(c["mask"])
    assert r["K"] == 1 and r["n_pixels"].tolist() == [16384]
    t = RS.tables(r["object_id"], 1, c["points"], c["grid"])
    assert t["count"].tolist() == [[4096] * 4] and t["count3d"].tolist() == [[4096] * 4]
    assert (t["bbox"][0] == np.array([0, 0, 63, 63])).all() and (t["centroid_px"] == 31.5).all()
    half = 0.5 / 512  # half a fixed-point step of v / 256
    want = np.stack([np.full(4, 31.5 / 8 + half), np.full(4, 31.5 / 8 + half), 2.0 + np.arange(4) / 4 + half], axis=1)
    assert np.array_equal(t["centroid_xyz"][0], want.astype(np.float32))
    assert np.array_equal(t["box3d"][0], np.stack([np.array([0, 0, 2 + k / 4, 63 / 8, 63 / 8, 2 + k / 4], dtype=np.float32) for k in range(4)]))
    assert t["step"][0].tolist() == [[0, 0, 0]] + [[0, 0, 0.25]] * 3 and t["speed"][0].tolist() == [0, 0.25, 0.25, 0.25]
    # invalid points do not count: NaN, outside the fixed-point range, and no grid at all
    p = c["points"].copy()
    p[0, 0], p[1, 1], p[2, 2] = np.nan, 1e9, -1e9
    t2 = RS.tables(r["object_id"], 1, p, c["grid"])
    assert t2["count3d"].tolist() == [[4093, 4096, 4096, 4096]] and t2["count"].tolist() == [[4096] * 4]
    for v in (0.0, -1.0, np.nan, np.inf):
        t3 = RS.tables(r["object_id"], 1, c["points"], np.array([0, 0, 0, v], dtype=np.float32))
        assert (t3["count3d"] == 0).all() and (t3["centroid_xyz"] == 0).all() and (t3["speed"] == 0).all() and (t3["box3d"] == 0).all()
    # an object absent in 3D from frame 1: zeros, and step 0 on both sides of the gap
    p = c["points"].copy().reshape(4, -1, 3)
    p[1] = np.nan
    t4 = RS.tables(r["object_id"], 1, p.reshape(-1, 3), c["grid"])
    assert t4["count3d"].tolist() == [[4096, 0, 4096, 4096]] and t4["centroid_xyz"][0, 1].tolist() == [0, 0, 0]
    assert t4["speed"][0].tolist() == [0, 0, 0, 0.25]


def test_tracks_and_overlay_restatements():
    ids = np.full((4, 6, 8), -1, dtype=np.int32)
    ids[:, 1, 1], ids[:, 2, 2], ids[:2, 4, 4] = 1, 0, 2
    traj = np.zeros((5, 2, 4), dtype=np.float32)
    vis = np.ones((5, 4), dtype=np.float32)
    traj[0, :, :2], traj[0, :, 2:] = 1, 2  # two frames on object 1, two on object 0: the tie goes to 0
    traj[1] = 4  # on object 2 in frames 0, 1, on nothing later
    traj[2] = 1
    vis[2, 1:] = -1  # invisible after frame 0
    traj[3, 0], traj[3, 1] = [0.5, 1.49, -0.6, 7.5], [0.5, 0.5, 1, 1]  # x.5 rounds up: (1, 1), (1, 1), outside, outside
    traj[4] = 5  # never on an object
    r = RS.tracks(ids, traj, vis)
    assert r["track_object_nt"].tolist() == [[1, 1, 0, 0], [2, 2, -1, -1], [1, -1, -1, -1], [1, 1, -1, -1], [-1] * 4]
    assert r["track_object"].tolist() == [0, 2, 1, 1, -1] and r["votes"].tolist() == [2, 2, 1, 2, 0]
    frames = np.arange(4 * 6 * 8 * 3, dtype=np.int64).reshape(4, 6, 8, 3).astype(np.uint8)
    lut = MO.object_colours(3)
    assert lut.shape == (3, 3) and lut.dtype == np.uint8 and lut[0].tolist() == [255, 0, 0]
    assert np.array_equal(RS.overlay(frames, ids, lut, 0), frames)
    full = RS.overlay(frames, ids, lut, 256)
    assert np.array_equal(full[ids >= 0], lut[ids[ids >= 0]]) and np.array_equal(full[ids < 0], frames[ids < 0])
    half = RS.overlay(frames, ids, lut, 128)
    assert half[0, 1, 1].tolist() == [(int(a) + int(b) + 1) >> 1 for a, b in zip(frames[0, 1, 1], lut[1])]


def test_the_random_clips_of_the_gpu_cases_exercise_every_rule():
    for seed, shape in ((1, (3, 5, 7)), (2, (4, 13, 17))):
        c = RS.random_case(seed, *shape)
        r = RS.label(c["mask"], c["depth"], c["flow"], c["keep"], max_depth_ratio=1.5)
        k = r["counters"]
        assert 1 < k["n_components"] < k["n_foreground"] < k["n_pixels"] and (r["last_frame"] > r["first_frame"]).any()
        assert np.isnan(c["mask"]).any() and np.isnan(c["flow"]).any() and (c["keep"] == 0).any() and not np.isfinite(c["depth"]).all()


def _load_demo():
    spec = importlib.util.spec_from_file_location("demo_objects_args", os.path.join(ROOT, "demo", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_plan_with_and_without_objects():
    demo = _load_demo()
    base = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]
    kw = dict(crop_size=(64, 224, 224), estimation_directions=[1], track_2d_querry_sampling_spacing=0.04)
    a = demo.parse_args(["--synthetic", "--objects", "out"])
    assert a.objects == "out" and demo.plan(a) == (base + ["camray"], kw)
    a = demo.parse_args(["--synthetic", "--objects", "out", "--static-map", "m", "--frames", "16"])
    assert demo.plan(a) == (base + ["camray"], dict(kw, crop_size=(16, 224, 224)))
    for argv, want in ((["--synthetic"], (base, kw)), (["--synthetic", "--vis", "o"], (base, kw)),
                       (["--synthetic", "--static-map", "o"], (base + ["camray"], kw))):
        a = demo.parse_args(argv)
        assert a.objects is None and demo.plan(a) == want, argv


def test_argument_errors_are_raised_before_any_gpu_work():
    T, H, W = 3, 4, 5
    m = torch.zeros(T, H, W)
    for kw, name in ((dict(mask_thw=m[0]), "mask_thw"), (dict(mask_thw=m.to(torch.int32)), "mask_thw"), (dict(mask_thw=m[:0]), "mask_thw"),
                     (dict(depth_thw=m[:2]), "depth_thw"), (dict(depth_thw=m.long()), "depth_thw"), (dict(flow_2thw=m), "flow_2thw"),
                     (dict(flow_2thw=torch.zeros(3, T, H, W)), "flow_2thw"), (dict(keep_thw=m), "keep_thw"),
                     (dict(keep_thw=torch.ones(T, H, W + 1, dtype=torch.uint8)), "keep_thw"), (dict(connectivity=6), "connectivity"),
                     (dict(max_depth_ratio=float("nan")), "max_depth_ratio"), (dict(max_depth_ratio=0.5), "max_depth_ratio"),
                     (dict(min_pixels=0), "min_pixels"), (dict(min_frames=0), "min_frames")):
        args = dict(mask_thw=m)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            MO.label_components(**args)
    with pytest.raises(AssertionError, match="GPU"):  # valid arguments, host tensors: the device check comes after the argument checks
        MO.label_components(m)
    ids = torch.zeros(T, H, W, dtype=torch.int32)
    pts, grid = torch.zeros(T * H * W, 3), torch.tensor([0.0, 0.0, 0.0, 1.0])
    for kw, name in ((dict(object_id=ids.long()), "object_id"), (dict(object_id=ids[0]), "object_id"), (dict(K=-1), "K must"),
                     (dict(K=(1 << 27)), "K must"), (dict(points=pts), "go together"), (dict(grid=grid), "go together"),
                     (dict(points=pts[:-1], grid=grid), "points"), (dict(points=pts.long(), grid=grid), "points"),
                     (dict(points=pts, grid=grid[:3]), "grid")):
        args = dict(object_id=ids, K=1)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            MO.object_tracks(**args)
    with pytest.raises(AssertionError, match="GPU"):
        MO.object_tracks(ids, 1)
    traj, vis = torch.zeros(2, 2, T), torch.zeros(2, T)
    for a, name in (((ids.float(), traj, vis), "object_id"), ((ids, traj[:, :1], vis), "traj_n2t"), ((ids, traj[..., :2], vis), "traj_n2t"),
                    ((ids, traj, vis[:1]), "vis_nt"), ((ids, traj, vis.long()), "vis_nt")):
        with pytest.raises(ValueError, match=name):
            MO.assign_tracks(*a)
    fr = torch.zeros(T, H, W, 3, dtype=torch.uint8)
    for a, kw, name in (((fr.float(), ids, 1), {}, "frames_u8"), ((fr[:, :, :, :2], ids, 1), {}, "frames_u8"), ((fr, ids, -1), {}, "K must"),
                        ((fr, ids, 1), dict(alpha=257), "alpha"), ((fr, ids, 1), dict(alpha=-1), "alpha"), ((fr, ids, 1), dict(alpha=0.5), "alpha")):
        with pytest.raises(ValueError, match=name):
            MO.overlay(*a, **kw)
    with pytest.raises(ValueError, match="dyn_mask"):
        MO.moving_objects_from_outputs({}, {}, ["depth"])
    with pytest.raises(ValueError, match="dyn_mask"):
        MO.moving_objects_from_outputs({}, {"depth_est_b1thw": m}, ["dyn_mask"])
    with pytest.raises(AssertionError, match="batch size 1"):
        MO.moving_objects_from_outputs({}, {"dyn_mask_est_b1thw": torch.zeros(2, 1, T, H, W)}, ["dyn_mask"])


def test_native_entries_refuse_bad_sizes_and_null_pointers():
    """The argument checks come before anything touches a device: L4P_E_INVALID and a text that names the entry."""
    from l4p_amd import _lib

    lib = _lib.load()
    p = 256  # never dereferenced: every call below is refused
    assert lib.l4p_objects_ws_bytes(3, 5, 7) >= 3 * 105 * 4 and lib.l4p_objects_tables_ws_bytes(2, 3) > 0
    for shape in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (-1, 5, 7), (1 << 10, 1 << 10, (1 << 10) + 1), (1 << 16, 1 << 16, 1 << 16)):
        assert lib.l4p_objects_ws_bytes(*shape) == 0, shape
    assert lib.l4p_objects_ws_bytes(1 << 10, 1 << 10, 1 << 10) > 0
    for kt in ((0, 3), (2, 0), (-1, 3), (1 << 14, (1 << 13) + 1)):
        assert lib.l4p_objects_tables_ws_bytes(*kt) == 0, kt
    good = {"l4p_objects_label": [None, p, None, None, None, 2, 3, 4, 8, 0.0, 1, 1, p, p, p, p],
            "l4p_objects_roots": [None, p, p, p, 2, 3, 4, 1, p, p, p, p],
            "l4p_objects_tables": [None, p, p, p, 2, 3, 4, 1, p, p, p, p, p, p, p, p, p],
            "l4p_objects_tracks": [None, p, p, p, 1, 2, 3, 4, p, p, p],
            "l4p_objects_overlay": [None, p, p, p, 2, 3, 4, 1, 128, p]}
    skip = {("l4p_objects_label", 9), ("l4p_objects_tables", 2)}  # a float; points is optional
    for name, args in good.items():
        fn = getattr(lib, name)
        for k, v in enumerate(args):
            if v is None or (name, k) in skip:
                continue
            bad = list(args)
            bad[k] = None if v == p else -1
            assert fn(*bad) == -1, (name, k)
            assert name + ":" in lib.l4p_last_error().decode(), (name, k)
    assert lib.l4p_objects_label(None, p, None, None, None, 2, 3, 4, 6, 0.0, 1, 1, p, p, p, p) == -1  # connectivity
    assert lib.l4p_objects_label(None, p, None, None, None, 1 << 11, 1 << 10, 1 << 10, 8, 0.0, 1, 1, p, p, p, p) == -1  # T H W > 2^30
    assert lib.l4p_objects_roots(None, p, p, p, 2, 3, 4, 25, p, p, p, p) == -1  # n_kept > T H W
    assert lib.l4p_objects_overlay(None, p, p, p, 2, 3, 4, 1, 257, p) == -1
    # K = 0 and N = 0 are accepted and launch nothing
    assert lib.l4p_objects_roots(None, p, p, p, 2, 3, 4, 0, None, None, None, None) == 0
    assert lib.l4p_objects_tables(None, p, None, None, 2, 3, 4, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.l4p_objects_tracks(None, p, None, None, 0, 2, 3, 4, None, None, None) == 0
