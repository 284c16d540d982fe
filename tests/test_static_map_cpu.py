"""CPU: the static-map restatement on closed-form scenes, what the clouds of the GPU cases are, the demo's plan with --static-map and
the wrappers' argument errors, raised before any GPU work (l4p_amd/utils/static_map.py, tests/static_map_restate.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import static_map as SM
from tests import static_map_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restate(c, **kw):
    return RS.restate(c["points"], c["colors"], c["T"], c["grid"], c.get("mask"), c.get("keep"), **kw)


def test_a_plane_sampled_on_the_voxel_lattice():
    """A fronto-parallel plane z = 2 seen by a camera that does not move, sampled at the quarter points of the voxels (v = 0.25,
    every number dyadic): 8 x 6 voxels, 4 samples per voxel and frame, centres at the voxel's middle plus half a fraction step."""
    T, v = 3, 0.25
    a = (np.arange(-8, 8) + 0.5) * (v / 2)  # two samples per voxel and axis: fractions 0.25 and 0.75
    b = (np.arange(-6, 6) + 0.5) * (v / 2)
    xx, yy = np.meshgrid(a, b, indexing="ij")
    frame = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, 2.0)], axis=1).astype(np.float32)
    pts = np.concatenate([frame] * T)
    col = np.full((len(pts), 3), 100, dtype=np.uint8)
    col[::2] = 101  # mean 100.5 rounds half up
    r = RS.restate(pts, col, T, [0, 0, 0, v])
    assert r["counters"] == dict(n_points=T * 192, n_used=T * 192, n_nonfinite=0, n_masked=0, n_out_of_range=0, n_voxels=48, n_kept=48,
                                 n_overflow=0)
    assert (r["count"] == 4 * T).all() and (r["n_frames"] == T).all() and (r["first_frame"] == 0).all() and (r["last_frame"] == T - 1).all()
    ix = ((r["key"] & 0x1FFFFF) - (1 << 20)).astype(np.float64)
    iy = (((r["key"] >> 21) & 0x1FFFFF) - (1 << 20)).astype(np.float64)
    assert sorted(set(ix)) == list(range(-4, 4)) and sorted(set(iy)) == list(range(-3, 3)) and ((r["key"] >> 42) == (1 << 20) + 8).all()
    half = 0.5 + 2.0 ** -17  # mean fraction (0.25 + 0.75) / 2, plus half a step of 1 / 65536
    want = np.stack([(ix + half) * v, (iy + half) * v, np.full(48, (8 + 2.0 ** -17) * v)], axis=1)
    assert np.array_equal(r["xyz"], want.astype(np.float32))
    assert (r["colors"] == 101).all()
    assert np.array_equal(r["first_point"], np.sort(r["first_point"])) and r["first_point"][0] == 0  # order of first appearance
    assert np.array_equal(r["voxel_id"][:192], r["voxel_id"][192:384]) and r["voxel_id"].min() == 0 and r["voxel_id"].max() == 47


def test_a_point_seen_in_frames_0_and_2():
    pts = np.array([[0.3, 0.3, 1.1], [5.5, 0.5, 0.5], [7.5, 0.5, 0.5], [9.5, 0.5, 0.5], [0.6, 0.4, 1.9], [9.7, 0.5, 0.5]], dtype=np.float32)
    col = np.zeros((6, 3), dtype=np.uint8)
    r = RS.restate(pts, col, 3, [0, 0, 0, 1.0])  # HW = 2: frames (0, 1), (2, 3), (4, 5)
    assert r["counters"]["n_voxels"] == 4 and r["counters"]["n_kept"] == 2
    assert r["n_frames"].tolist() == [2, 2] and r["first_frame"].tolist() == [0, 1] and r["last_frame"].tolist() == [2, 2]
    assert r["first_point"].tolist() == [0, 3] and r["count"].tolist() == [2, 2]
    assert r["voxel_id"].tolist() == [0, -1, -1, 1, 0, 1]
    one = RS.restate(pts, col, 3, [0, 0, 0, 1.0], min_frames=1)
    assert one["voxel_id"].tolist() == [0, 1, 2, 3, 0, 3] and one["n_frames"].tolist() == [2, 1, 1, 2]
    # two points of ONE frame in a voxel are one frame
    same = RS.restate(pts[[0, 4, 1, 2]], col[:4], 2, [0, 0, 0, 1.0], min_frames=1)
    assert same["n_frames"].tolist() == [1, 1, 1] and same["count"].tolist() == [2, 1, 1]
    assert RS.restate(pts[[0, 4, 1, 2]], col[:4], 2, [0, 0, 0, 1.0], min_frames=1, min_points=2)["voxel_id"].tolist() == [0, 0, -1, -1]


def test_negative_coordinates_use_floor_not_truncation():
    pts = np.array([[-0.1, 0.1, -1.0], [-0.0, -1.5, -1.25], [0.1, -0.1, 0.9]], dtype=np.float32)
    status, key, f = RS.keys_of(pts, [0, 0, 0, 1.0])
    assert status.tolist() == [0, 0, 0]
    idx = np.stack([((key >> s) & 0x1FFFFF) - (1 << 20) for s in (0, 21, 42)], axis=1)
    assert idx.tolist() == [[-1, 0, -1], [0, -2, -2], [0, -1, 0]]
    assert f[1].tolist() == [0, 32768, 49152] and f[0, 2] == 0 and f[0, 0] == int(np.floor((np.float32(-0.1) + np.float32(1)) * 65536))
    # an origin and a voxel size: the index is floor((p - o) / v)
    _, key, _ = RS.keys_of(np.array([[0.2, 0.3, 0.0]], dtype=np.float32), [0.25, 0.25, 0.25, 0.5])
    assert [int(((key[0] >> s) & 0x1FFFFF) - (1 << 20)) for s in (0, 21, 42)] == [-1, 0, -1]


def test_the_clouds_of_the_gpu_cases_are_what_their_names_say():
    assert _restate(RS.one_voxel_case())["counters"]["n_voxels"] == 1 and _restate(RS.one_voxel_case())["count"].tolist() == [4096]
    n = _restate(RS.tight_table_case(), min_frames=1)["counters"]["n_voxels"]
    assert 760 <= n <= 840 and len(RS.tight_table_case()["points"]) == 884  # about 800 voxels for 1024 slots
    assert _restate(RS.overflow_case(), min_frames=1)["counters"]["n_voxels"] == 200
    fr = _restate(RS.frames_case(), min_frames=1)["all"]
    assert np.bincount(fr["n_frames"]).tolist() == [0, 48, 8, 0, 8] and np.bincount(fr["count"]).tolist() == [0, 48, 8, 0, 8]
    big = _restate(RS.scene_case(5, 6, 40, 44, 0.6))  # the scan case: leaders in every one of its 11 blocks of 1024 points
    assert big["counters"]["n_kept"] >= 2000 and big["counters"]["n_voxels"] > big["counters"]["n_kept"] + 500
    # (a voxel that first appears in the last frame has one frame: the kept leaders end before the last blocks)
    assert len(set(big["all"]["first_point"] // 1024)) == 11 and len(set(big["first_point"] // 1024)) >= 8
    assert big["counters"]["n_masked"] > 500
    for origin in ((0.0, 0.0, 0.0), (0.25, -0.5, 1.0)):
        c = RS.edges_case(origin)
        r = _restate(c, min_frames=1)
        k = r["counters"]
        assert (k["n_nonfinite"], k["n_masked"], k["n_out_of_range"]) == (12, 10, 10) and k["n_used"] == 44
        idx = np.stack([((r["key"] >> s) & 0x1FFFFF) - (1 << 20) for s in (0, 21, 42)], axis=1)
        assert idx.min() == -(1 << 20) and idx.max() == (1 << 20) - 1  # the first and the last index are kept
        status, _, _ = RS.keys_of(c["points"], c["grid"], c["mask"], c["keep"])
        logit = c["mask"]
        assert (status[(logit == 0) | np.isnan(logit)] == 0).all() and (status[np.isfinite(c["points"]).all(1) & (logit > 0)] == 2).all()


def test_the_scene_generator_keeps_the_mover_out_and_fuses_the_rest():
    s = RS.make_scene(5, 6, 40, 44)
    assert np.array_equal(s["mover"], s["mask"] > 0) and 500 < s["mover"].sum() < 2000
    v = 2.0 * s["px"]
    r = RS.restate(s["points"], s["colors"], 6, [0, 0, 0, v], mask=s["mask"])
    assert (r["voxel_id"][s["mover"]] == -1).all()
    k = r["counters"]
    assert k["n_points"] == k["n_used"] + k["n_masked"] and k["n_used"] / k["n_kept"] > 6  # each piece of surface once, not T times
    without = RS.restate(s["points"], s["colors"], 6, [0, 0, 0, v])
    assert without["counters"]["n_voxels"] > k["n_voxels"]  # unmasked, the mover leaves its trail in the map
    # every kept voxel's position lies inside its voxel
    idx = np.stack([((r["key"] >> sh) & 0x1FFFFF) - (1 << 20) for sh in (0, 21, 42)], axis=1)
    assert (r["xyz"] >= (idx * np.float64(np.float32(v))).astype(np.float32)).all()
    assert (r["xyz"] <= ((idx + 1) * np.float64(np.float32(v))).astype(np.float32)).all()


def _load_demo():
    spec = importlib.util.spec_from_file_location("demo_static_map_args", os.path.join(ROOT, "demo", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_plan_with_and_without_static_map():
    demo = _load_demo()
    base = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]
    kw = dict(crop_size=(64, 224, 224), estimation_directions=[1], track_2d_querry_sampling_spacing=0.04)
    a = demo.parse_args(["--synthetic", "--static-map", "out"])
    assert a.static_map == "out" and demo.plan(a) == (base + ["camray"], kw)
    a = demo.parse_args(["--synthetic", "--static-map", "out", "--recon4d", "r", "--frames", "16"])
    assert demo.plan(a) == (base + ["camray"], dict(kw, crop_size=(16, 224, 224)))
    a = demo.parse_args(["--synthetic", "--davis", "X", "--static-map", "out"])
    assert demo.plan(a) == (base + ["camray"], dict(kw, track_2d_querry_sampling_spacing=0.02))
    # every combination without the flag, as literals: what plan() returned before the flag existed
    dv = dict(kw, track_2d_querry_sampling_spacing=0.02)
    for argv, want in (
            (["--synthetic"], (base, kw)),
            (["--synthetic", "--vis", "o"], (base, kw)),
            (["--synthetic", "--save", "o", "--frames", "16"], (base, dict(kw, crop_size=(16, 224, 224)))),
            (["--synthetic", "--recon4d", "o"], (base + ["camray"], kw)),
            (["--synthetic", "--view4d", "o"], (base + ["camray"], kw)),
            (["--synthetic", "--scene-flow", "o"], (base + ["camray"], kw)),
            (["--synthetic", "--scene-flow", "o", "--view4d", "v", "--frames", "16"], (base + ["camray"], dict(kw, crop_size=(16, 224, 224)))),
            (["--synthetic", "--bidirectional"], (base, dict(kw, estimation_directions=[1, -1]))),
            (["--synthetic", "--davis", "X"], (base, dv)),
            (["--synthetic", "--davis", "X", "--recon4d", "o"], (base + ["camray"], dict(dv, crop_size=(56, 224, 224)))),
            (["--synthetic", "--davis", "X", "--view4d", "o"], (base + ["camray"], dict(dv, crop_size=(56, 224, 224)))),
            (["--synthetic", "--dycheck", "X"], (base + ["camray"], dict(kw, resize_size=(298, 224), stride=2))),
            (["--synthetic", "--spacing", "0.1", "--max-queries", "8"], (base, dict(kw, track_2d_querry_sampling_spacing=0.1)))):
        a = demo.parse_args(argv)
        assert a.static_map is None and demo.plan(a) == want, argv


def test_argument_errors_are_raised_before_any_gpu_work():
    M, T = 12, 3
    p, c = torch.zeros(M, 3), torch.zeros(M, 3, dtype=torch.uint8)
    g = torch.tensor([0.0, 0.0, 0.0, 1.0])
    for kw, name in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=-1.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"),
                     (dict(voxel_size=float("inf")), "voxel_size"), (dict(), "exactly one"), (dict(voxel_size=1.0, grid=g), "exactly one"),
                     (dict(grid=g[:3]), "grid"), (dict(grid=g.to(torch.int32)), "grid"), (dict(grid=[0, 0, 0, 1]), "grid"),
                     (dict(voxel_size=1.0, origin=(0, 0)), "origin"), (dict(voxel_size=1.0, origin=(0, float("nan"), 0)), "origin"),
                     (dict(voxel_size=1.0, T=5), "do not divide"), (dict(voxel_size=1.0, T=0), "do not divide"),
                     (dict(voxel_size=1.0, points=p.reshape(3, M)), "points"), (dict(voxel_size=1.0, points=p.reshape(-1)), "points"),
                     (dict(voxel_size=1.0, points=p.to(torch.int32)), "points"), (dict(voxel_size=1.0, points=p[:0], colors=c[:0]), "do not divide"),
                     (dict(voxel_size=1.0, colors=c[:-1]), "colors"), (dict(voxel_size=1.0, colors=c.float()), "colors"),
                     (dict(voxel_size=1.0, dyn_mask=torch.zeros(M - 1)), "dyn_mask"), (dict(voxel_size=1.0, dyn_mask=torch.zeros(M, dtype=torch.int32)), "dyn_mask"),
                     (dict(voxel_size=1.0, keep=torch.ones(M + 1, dtype=torch.uint8)), "keep"), (dict(voxel_size=1.0, keep=torch.ones(M)), "keep"),
                     (dict(voxel_size=1.0, table_capacity=48), "table_capacity"), (dict(voxel_size=1.0, table_capacity=0), "table_capacity"),
                     (dict(voxel_size=1.0, table_capacity=1 << 31), "table_capacity"),
                     (dict(voxel_size=1.0, min_frames=0), "min_frames"), (dict(voxel_size=1.0, min_points=0), "min_points")):
        args = dict(points=p, colors=c, T=T)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            SM.fuse_points(**args)
    with pytest.raises(AssertionError, match="GPU"):  # valid arguments, host tensors: the device check comes after the argument checks
        SM.fuse_points(p, c, T, voxel_size=1.0)
    assert SM.default_capacity(884) == 2048 and SM.default_capacity(1024) == 2048 and SM.default_capacity(1025) == 4096
    assert SM.default_capacity(1) == 2
    batch = {"rgb_b3thw": torch.zeros(1, 3, T, 2, 2), "seq_name": ["clip"]}
    out = {"depth_est_b1thw": torch.zeros(1, 1, T, 2, 2)}
    tasks = ["depth", "camray"]
    for missing in tasks:
        with pytest.raises(AssertionError, match="Tasks must include"):
            SM.static_map_from_outputs(batch, out, [t for t in tasks if t != missing])
    with pytest.raises(AssertionError, match="batch size 1"):
        SM.static_map_from_outputs({"rgb_b3thw": torch.zeros(2, 3, T, 2, 2)}, out, tasks)
    with pytest.raises(ValueError, match="camray_est_b6thw"):
        SM.static_map_from_outputs(batch, dict(out, camray_est_b6thw=p), tasks)
    with pytest.raises(ValueError, match="traj3d_est_b16t"):
        SM.static_map_from_outputs(batch, out, tasks)
    full = dict(out, traj3d_est_b16t=torch.zeros(1, 16, T), traj3d_intrinsics_est_b16t=torch.zeros(1, 16, T))
    with pytest.raises(ValueError, match="voxel_px"):
        SM.static_map_from_outputs(batch, full, tasks, voxel_px=0.0)


def test_native_entries_refuse_bad_sizes_and_null_pointers():
    """The argument checks come before anything touches a device: L4P_E_INVALID and a text that names the entry."""
    from l4p_amd import _lib

    lib = _lib.load()
    p = 256  # never dereferenced: every call below is refused
    assert lib.l4p_static_map_ws_bytes(1024, 884) >= 1024 * 64 + 884 * 4
    assert lib.l4p_static_map_ws_bytes(2048, 884) - lib.l4p_static_map_ws_bytes(1024, 884) == 1024 * 64
    for cap, m in ((1000, 884), (0, 884), (-4, 884), (1 << 31, 884), (1024, 0), (1024, (1 << 24) + 1)):
        assert lib.l4p_static_map_ws_bytes(cap, m) == 0, (cap, m)
    good = {"l4p_static_map_insert": [None, p, p, None, None, p, 2, 3, 64, p],
            "l4p_static_map_count": [None, p, 2, 3, 64, 1, 1, p],
            "l4p_static_map_emit": [None, p, p, 2, 3, 64, 1, p, p, p, p, p, p, p, p, p]}
    for name, args in good.items():
        fn = getattr(lib, name)
        for k, v in enumerate(args):
            if v is None:
                continue
            bad = list(args)
            bad[k] = None if v == p else -1
            assert fn(*bad) == -1, (name, k)
            assert name + ":" in lib.l4p_last_error().decode(), (name, k)
    for bad_cap in (48, 0, 1 << 31):
        assert lib.l4p_static_map_insert(None, p, p, None, None, p, 2, 3, bad_cap, p) == -1, bad_cap
    assert lib.l4p_static_map_insert(None, p, p, None, None, p, 1 << 13, 1 << 12, 64, p) == -1  # T HW > 2^24
    assert lib.l4p_static_map_count(None, p, 2, 3, 64, 0, 1, p) == -1 and lib.l4p_static_map_count(None, p, 2, 3, 64, 1, 0, p) == -1
    assert lib.l4p_static_map_emit(None, p, p, 2, 3, 64, 7, p, p, p, p, p, p, p, p, p) == -1  # n_kept > T HW
