"""GPU: the moving-object stage (l4p_amd/utils/moving_objects.py, csrc/objects.hip) against the numpy restatement
(tests/moving_objects_restate.py).

Pass rule of every comparison with the restatement: every array the entry points emit - object_id, label, root, n_pixels,
first_frame, last_frame, the 2D and 3D tables, the track assignment, the overlay - and the six counters are EQUAL, byte for byte.
The design is integer except for the stated f32 / f64 steps, each rounded operation by operation, so there is no tolerance; n_guard
is 0 in every case."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import moving_objects as MO
from l4p_amd.utils import recon4d as R
from l4p_amd.utils import static_map as SM
from tests import moving_objects_restate as RS
from tests import scene_flow_restate as SFRS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAKE = (3, 2 * RS.TILE_H + 9, 2 * RS.TILE_W + 22)  # (3, 41, 150): a little over two tiles each way


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None


def _same(got, want, fields, tag):
    for k in fields:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        w = np.ascontiguousarray(want[k])
        assert g.dtype == RS.DTYPES[k] and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.shape)
        differ = int((np.ascontiguousarray(g).view(np.uint8) != w.view(np.uint8)).sum())
        print(f"{tag}: {k} {g.shape}: {differ} bytes differ")
        assert differ == 0, (tag, k)


def _label(c, tag, **kw):
    """label_components on a clip of the restatement module, held equal to the restatement; returns (GPU result, restatement)."""
    res = MO.label_components(_t(c["mask"]), _t(c.get("depth")), _t(c.get("flow")), _t(c.get("keep")), **kw)
    want = RS.label(c["mask"], c.get("depth"), c.get("flow"), c.get("keep"), **kw)
    print(f"{tag}: counters {res['counters']}")
    assert tuple(res["counters"]) == RS.COUNTERS and res["counters"] == want["counters"], (tag, res["counters"], want["counters"])
    assert res["counters"]["n_guard"] == 0 and res["K"] == want["K"]
    _same(res, want, RS.LABEL_FIELDS, tag)
    return res, want


def _tables(res, want, tag, points=None, grid=None):
    got = MO.object_tracks(res["object_id"], res["K"], _t(points), _t(grid))
    ref = RS.tables(want["object_id"], want["K"], points, grid)
    _same(got, ref, RS.TABLES_2D + (RS.TABLES_3D if points is not None else ()), tag)
    assert set(got) == set(ref)
    return got


@pytest.mark.parametrize("seed,shape", [(1, (3, 5, 7)), (2, (4, 13, 17))])
def test_ragged_random_clips(dev, seed, shape):
    """Fewer pixels than one workgroup; sizes that are no multiple of 4, 16 or 64; every optional input in every combination."""
    c = RS.random_case(seed, *shape)
    g = np.random.default_rng(seed)
    pts = g.normal(0, 2, (int(np.prod(shape)), 3)).astype(np.float32)
    pts[g.random(len(pts)) < 0.05] = np.nan
    grid = np.array([0.1, -0.2, 0.3, 0.05], dtype=np.float32)
    for keys, kw in (((), {}), (("depth",), dict(max_depth_ratio=1.5)), (("flow",), dict(connectivity=4)), (("keep",), dict(min_pixels=3)),
                     (("depth", "flow", "keep"), dict(max_depth_ratio=1.25, min_frames=2)), (("depth", "flow"), dict(max_depth_ratio=0.0))):
        sub = dict(mask=c["mask"], **{k: c[k] for k in keys})
        res, want = _label(sub, f"ragged {shape} {keys} {kw}", **kw)
        _tables(res, want, f"ragged {shape} {keys} tables", pts, grid)


@pytest.mark.parametrize("mirrored", [False, True])
def test_serpentine_across_tile_seams(dev, mirrored):
    T, H, W = SNAKE
    c = RS.serpentine(T, H, W, mirrored)
    res, want = _label(c, f"serpentine mirrored={mirrored}")
    assert res["K"] == 1 and res["root"].tolist() == [0] and res["n_pixels"].tolist() == [int((c["mask"] > 0).sum())]
    _label(c, "serpentine, 4-connected", connectivity=4)
    _label(dict(c, mask=c["mask"][:, ::-1].copy()), "serpentine, upside down")
    _tables(res, want, "serpentine tables")
    again = MO.label_components(_t(c["mask"]))  # the largest clip of this file, a second time
    assert again["counters"] == res["counters"] and all(torch.equal(again[k], res[k]) for k in RS.LABEL_FIELDS)


def test_checkerboard_connectivity_and_empty_tables(dev):
    c = RS.checkerboard(9, 11)
    res, _ = _label(c, "checkerboard 8", connectivity=8)
    assert res["K"] == 1
    res, _ = _label(c, "checkerboard 4", connectivity=4)
    assert res["K"] == int((c["mask"] > 0).sum()) and (res["n_pixels"] == 1).all()
    res, want = _label(c, "checkerboard 4, min_pixels 2", connectivity=4, min_pixels=2)
    assert res["K"] == 0 and res["root"].shape == (0,) and (res["object_id"] == -1).all()
    pts = np.zeros((99, 3), dtype=np.float32)
    got = _tables(res, want, "no objects", pts, np.array([0, 0, 0, 1], dtype=np.float32))
    assert got["count"].shape == (0, 1) and got["box3d"].shape == (0, 1, 6)
    assert MO.overlay(torch.zeros(1, 9, 11, 3, dtype=torch.uint8, device="cuda"), res["object_id"], 0).sum() == 0
    tr = MO.assign_tracks(res["object_id"], torch.zeros(0, 2, 1, device="cuda"), torch.zeros(0, 1, device="cuda"))
    assert tr["track_object"].shape == (0,) and tr["track_object_nt"].shape == (0, 1)


def test_temporal_linking(dev):
    c = RS.moving_square()
    res, _ = _label(dict(mask=c["mask"]), "square, no flow")
    assert res["K"] == 4
    assert _label(dict(mask=c["mask"]), "square, no flow, two frames", min_frames=2)[0]["K"] == 0
    res, _ = _label(c, "square, flow", min_frames=2)
    assert res["K"] == 1 and res["n_pixels"].tolist() == [64] and res["last_frame"].tolist() == [3]
    variants = {}
    f = c["flow"].copy()
    f[0, 2][c["fg"][2]] = np.nan
    variants["NaN on frame 2"] = (f, 2)
    f = c["flow"].copy()
    ys, xs = np.nonzero(c["fg"][2])
    f[1, 2, ys[1:], xs[1:]] = np.inf
    variants["Inf on all but one pixel"] = (f, 1)
    f = c["flow"].copy()
    f[0, 1] = -100.0
    variants["outside the frame"] = (f, 2)
    for dx, n in ((-5.5, 1), (-4.5, 1), (-8.5, 1), (-9.5, 4)):
        f = c["flow"].copy()
        f[0][c["fg"]] = dx
        variants[f"flow x {dx}"] = (f, n)
    for name, (f, n) in variants.items():
        res, _ = _label(dict(mask=c["mask"], flow=f), "square, " + name)
        assert res["counters"]["n_components"] == n, name


def test_depth_gate(dev):
    c = RS.two_rectangles()
    assert _label(c, "rectangles, ratio 1.5", max_depth_ratio=1.5)[0]["n_pixels"].tolist() == [54, 60]
    assert _label(c, "rectangles, ratio 0", max_depth_ratio=0.0)[0]["K"] == 1
    assert _label(dict(mask=c["mask"]), "rectangles, no depth", max_depth_ratio=1.5)[0]["K"] == 1
    d = c["depth"].copy()
    for (y, x), v in zip(((3, 3), (3, 4), (4, 3), (4, 4), (6, 6)), (0.0, -1.0, np.nan, np.inf, -np.inf)):
        d[0, y, x] = v
    res, _ = _label(dict(c, depth=d), "rectangles, bad depths", max_depth_ratio=1.5)
    assert (res["label"][0, 3:5, 3:5] == -1).all() and res["label"][0, 6, 6] == -1


def test_order_filters_and_gaps(dev):
    c = RS.blobs()
    res, _ = _label(c, "blobs")
    assert res["first_frame"].tolist() == [0, 0, 1, 2, 4] and res["n_pixels"].tolist() == [54, 4, 60, 4, 12]
    assert _label(c, "blobs, min_pixels 5", min_pixels=5)[0]["K"] == 3 and _label(c, "blobs, min_frames 2", min_frames=2)[0]["K"] == 4
    res, want = _label(c, "blobs, both filters", min_pixels=12, min_frames=3)
    assert res["counters"] == dict(n_pixels=6 * 24 * 40, n_foreground=134, n_components=5, n_kept=2, n_kept_pixels=114, n_guard=0)
    # points: NaN, a coordinate outside the fixed-point range, -0 next to +0; object 0 without a valid point in frame 2
    g = np.random.default_rng(5)
    pts = g.normal(0, 1, (6 * 24 * 40, 3)).astype(np.float32)
    on = np.nonzero(want["object_id"].reshape(-1) >= 0)[0]
    pts[on[::7], 0], pts[on[1::7], 1], pts[on[2::7], 2], pts[on[3::7], 0], pts[on[4::7], 0] = np.nan, 3e7, -np.inf, -0.0, 0.0
    frame2 = want["object_id"][2].reshape(-1) == 0
    pts.reshape(6, -1, 3)[2][frame2] = np.nan
    grid = np.array([0.25, 0.5, -1.0, 0.03125], dtype=np.float32)
    got = _tables(res, want, "blobs tables", pts, grid)
    assert got["count"][1, 0] == 0 and got["bbox"][1, 0].tolist() == [0, 0, -1, -1] and got["count3d"][0, 2] == 0
    assert (got["step"][0, 2:4] == 0).all() and (got["speed"][0, 4:] > 0).all() and (got["step"][1, :2] == 0).all()
    for v in (0.0, float("nan")):
        _tables(res, want, f"blobs tables, v = {v}", pts, np.array([0, 0, 0, v], dtype=np.float32))
    _tables(res, want, "blobs tables, 2D only")


def test_contention_on_one_object(dev):
    """(4, 64, 64), all foreground: one object of 16384 pixels, every atomic of a frame on one accumulator; and the largest case
    twice, every output byte-equal."""
    c = RS.dyadic_plane()
    res, want = _label(c, "plane")
    assert res["K"] == 1 and res["n_pixels"].tolist() == [16384]
    got = _tables(res, want, "plane tables", c["points"], c["grid"])
    assert (got["count"] == 4096).all() and (got["centroid_px"] == 31.5).all() and got["speed"][0].tolist() == [0, 0.25, 0.25, 0.25]
    again = MO.label_components(_t(c["mask"]))
    assert again["counters"] == res["counters"]
    for k in RS.LABEL_FIELDS:
        assert torch.equal(again[k], res[k]), k
    t2 = MO.object_tracks(again["object_id"], again["K"], _t(c["points"]), _t(c["grid"]))
    for k in got:
        assert torch.equal(t2[k].view(torch.uint8), got[k].view(torch.uint8)), k


def test_tracks(dev):
    c = RS.blobs()
    res, want = _label(c, "blobs for tracks")
    T, H, W = c["mask"].shape
    g = np.random.default_rng(9)
    N = 70  # more than one wave
    traj = np.stack([g.uniform(-3, W + 3, (N, T)), g.uniform(-3, H + 3, (N, T))], axis=1).astype(np.float32)
    vis = g.normal(0.5, 1.0, (N, T)).astype(np.float32)
    traj[:8, 0], traj[:8, 1] = 4.0, 3.0  # on blob 0
    traj[0, 0, 3:], traj[0, 1, 3:] = 11.5, 15.5  # three frames on blob 0, three on blob 2: a tie, to the smaller id; x.5 rounds up
    vis[0] = 1.0
    vis[1, ::2] = -1.0  # invisible frames
    traj[2, 0, 1], traj[2, 1, 2], traj[2, 0, 3] = np.nan, np.inf, 1e30
    traj[3, 0], traj[3, 1] = [-0.5, -0.51, W - 0.5, W - 0.51, 4.49, 2.5], [2.5, 2.5, 2.5, 2.5, 1.5, 4.49]
    vis[3] = 1.0
    traj[4, 0], traj[4, 1] = 30.0, 1.0  # never on an object
    vis[4] = 1.0
    vis[5, 2] = np.nan
    got = MO.assign_tracks(res["object_id"], _t(traj), _t(vis))
    ref = RS.tracks(want["object_id"], traj, vis)
    _same(got, ref, RS.TRACK_FIELDS, "tracks")
    assert ref["track_object"][0] == 0 and ref["votes"][0] == 3 and ref["track_object_nt"][0].tolist() == [0, 0, 0, 2, 2, 2]
    assert ref["track_object"][4] == -1 and ref["votes"][4] == 0 and ref["track_object_nt"][3].tolist() == [-1, -1, -1, -1, 0, 0]


@pytest.mark.parametrize("alpha", [0, 128, 256])
def test_overlay(dev, alpha):
    c = RS.blobs()
    res, want = _label(c, "blobs for the overlay", min_frames=2)
    frames = np.random.default_rng(3).integers(0, 256, c["mask"].shape + (3,), dtype=np.uint8)
    got = MO.overlay(_t(frames), res["object_id"], res["K"], alpha).cpu().numpy()
    ref = RS.overlay(frames, want["object_id"], MO.object_colours(want["K"]), alpha)
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    off = want["object_id"] < 0
    assert np.array_equal(got[off], frames[off]) and (alpha == 0) == np.array_equal(got, frames)


def _outputs(seed, T, H, W, N=6):
    """A synthetic (batch, out, tasks) of one clip around scene_flow_restate.make_case (one mover: its rectangular object), with
    tracks: three on the mover, three beside it."""
    c = SFRS.make_case(seed, 1, T, H, W)
    g = torch.Generator().manual_seed(seed)
    f = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    batch = {"rgb_b3thw": ((torch.randint(0, 256, (1, 3, T, H, W), generator=g).float() - 128) / 64).cuda(),
             "rgb_mean_b3111": torch.tensor((0.485, 0.456, 0.406)).reshape(1, 3, 1, 1, 1).cuda(),
             "rgb_std_b3111": torch.tensor((0.229, 0.224, 0.225)).reshape(1, 3, 1, 1, 1).cuda(), "seq_name": ["clip"]}
    traj = torch.zeros(1, N, 2, T)
    traj[0, :3, 0], traj[0, :3, 1] = W // 3 + 1.0, H // 4 + 1.0
    traj[0, 3:, 0], traj[0, 3:, 1] = 1.0, 1.0
    out = {"depth_est_b1thw": f(c["depth"]), "flow_2d_backward_est_b2thw": f(c["flow"]), "dyn_mask_est_b1thw": f(c["mask"]),
           "traj3d_est_b16t": f(c["P"]).reshape(1, 16, T), "traj3d_intrinsics_est_b16t": f(c["K"]).reshape(1, 16, T),
           "track_2d_traj_est_bn2t": traj.cuda(), "track_2d_vis_est_bn1t": torch.ones(1, N, 1, T).cuda()}
    return c, batch, out, ["depth", "flow_2d_backward", "dyn_mask", "camray", "track_2d"]


def test_from_outputs_and_files(dev, tmp_path):
    T, H, W = 4, 17, 19
    c, batch, out, tasks = _outputs(31, T, H, W)
    mover = c["mask"][0, 0] > 0
    res = MO.moving_objects_from_outputs(batch, out, tasks)
    want = RS.label(c["mask"][0, 0], c["depth"][0, 0], c["flow"][0], min_pixels=64, min_frames=2)
    assert res["counters"] == want["counters"] and res["K"] == 1 and res["counters"]["n_guard"] == 0
    _same(res, want, RS.LABEL_FIELDS, "from outputs")
    assert np.array_equal(res["object_id"].cpu().numpy() == 0, mover) and res["n_pixels"].tolist() == [int(mover.sum())]
    rec = R.reconstruct_4d(batch, out, ["depth", "camray"])
    grid = SM.default_grid(out)
    assert torch.equal(res["grid"], grid) and torch.equal(res["points"], rec["points"])
    _same(res, RS.tables(want["object_id"], 1, rec["points"].cpu().numpy(), grid.cpu().numpy()), RS.TABLES_2D + RS.TABLES_3D, "from outputs")
    ref = RS.tracks(want["object_id"], out["track_2d_traj_est_bn2t"][0].cpu().numpy(), out["track_2d_vis_est_bn1t"][0, :, 0].cpu().numpy())
    _same(res, ref, RS.TRACK_FIELDS, "from outputs")
    assert res["track_object"].tolist() == [0, 0, 0, -1, -1, -1] and res["votes"].tolist() == [T] * 3 + [0] * 3
    # fewer tasks: no flow (the mover does not move in the image: still one object), no 3D tables, no tracks
    few = MO.moving_objects_from_outputs(batch, out, ["dyn_mask"], min_pixels=1, min_frames=1)
    _same(few, RS.label(c["mask"][0, 0]), RS.LABEL_FIELDS, "mask only")
    assert "speed" not in few and "track_object" not in few and few["count"].shape == (few["K"], T)
    # files
    name = MO.generate_moving_objects(batch, out, tasks, str(tmp_path))
    assert name == os.path.join(str(tmp_path), "clip_objects.json")
    info = json.load(open(name))
    assert info["counters"] == res["counters"] and info["n_objects"] == 1 and len(info["objects"]) == 1
    o = info["objects"][0]
    assert o["n_pixels"] == int(mover.sum()) and (o["first_frame"], o["last_frame"], o["n_tracks"]) == (0, T - 1, 3)
    assert o["bbox"] == res["bbox"][0].tolist() and o["speed"] == res["speed"][0].tolist() and o["count"] == res["count"][0].tolist()
    assert np.array_equal(np.array(o["centroid_xyz"], dtype=np.float32), res["centroid_xyz"][0].cpu().numpy())
    assert json.loads(json.dumps(info)) == info
    ply = R.read_ply(os.path.join(str(tmp_path), "clip_objects.ply"))
    on = (res["object_id"].reshape(-1) >= 0).cpu().numpy()
    assert np.array_equal(ply["xyz"], rec["points"].cpu().numpy()[on]) and (ply["rgb"] == MO.object_colours(1)[0]).all()
    video = os.path.join(str(tmp_path), "clip_objects")
    assert os.path.exists(video + ".mp4") or len(os.listdir(video)) == T


def test_demo_objects_branch(dev, tmp_path, capsys):
    """demo.run's objects branch on a synthetic `out` (a run of demo.main builds the full-size model: not a few seconds)."""
    spec = importlib.util.spec_from_file_location("demo_objects_run", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    _, batch, out, tasks = _outputs(32, 4, 16, 20)
    d = str(tmp_path / "objects")
    demo.objects(batch, out, tasks, d)
    res = MO.moving_objects_from_outputs(batch, out, tasks)
    info = json.load(open(os.path.join(d, "clip_objects.json")))
    assert info["counters"] == res["counters"] and info["n_objects"] == res["K"] == 1
    line = capsys.readouterr().out
    assert "objects: 1 of 1 components kept" in line and "3 tracks on objects" in line
