"""GPU: the static scene map (l4p_amd/utils/static_map.py, csrc/static_map.hip) against the numpy restatement
(tests/static_map_restate.py).

Pass rule of every comparison with the restatement: every array the entry points emit - xyz, colours, count, n_frames, first_frame,
last_frame, first_point, key, voxel_id - and the eight counters are EQUAL, bit for bit.  The design is integer (counts, sums of
16-bit fractions, minima, maxima) and the two float stages are correctly rounded operation by operation, so there is no tolerance."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from l4p_amd import _lib
from l4p_amd.utils import recon4d as R
from l4p_amd.utils import static_map as SM
from tests import scene_flow_restate as SFRS
from tests import static_map_restate as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = dict(xyz=np.float32, colors=np.uint8, count=np.int32, n_frames=np.int32, first_frame=np.int32, last_frame=np.int32,
              first_point=np.int32, key=np.int64, voxel_id=np.int32)


def _fuse(c, **kw):
    """fuse_points on a case of the restatement module; ``grid`` goes in as a device tensor."""
    t = lambda k: torch.from_numpy(c[k]).cuda() if c.get(k) is not None else None  # noqa: E731
    return SM.fuse_points(t("points"), t("colors"), c["T"], grid=t("grid"), dyn_mask=t("mask"), keep=t("keep"), **kw)


def _want(c, **kw):
    return RS.restate(c["points"], c["colors"], c["T"], c["grid"], c.get("mask"), c.get("keep"), **kw)


def _check(res, want, tag):
    got = {k: res[k].cpu().numpy() for k in RS.FIELDS}
    print(f"{tag}: counters {res['counters']}")
    assert tuple(res["counters"]) == RS.COUNTERS and res["counters"] == want["counters"], (res["counters"], want["counters"])
    for k in RS.FIELDS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        differ = int((got[k].view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)).sum())
        print(f"{tag}: {k} {got[k].shape}: {differ} bytes differ")
        assert differ == 0, k
    return got


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 13, 17)])
def test_ragged_clouds(dev, shape):
    """Fewer points than one workgroup; sizes that are no multiple of 64 or 256."""
    c = RS.scene_case(3 + shape[0], *shape, 1.0)
    want = _want(c)
    assert 0 < want["counters"]["n_kept"] < want["counters"]["n_voxels"] and want["counters"]["n_masked"] > 0
    _check(_fuse(c), want, f"ragged {shape}")
    _check(_fuse(dict(c, mask=None), min_frames=1), _want(dict(c, mask=None), min_frames=1), f"ragged {shape}, no mask, one frame")


def test_leader_scan_across_blocks(dev):
    c = RS.scene_case(5, 6, 40, 44, 0.6)
    want = _want(c)
    assert want["counters"]["n_kept"] >= 2000
    got = _check(_fuse(c), want, "scan")
    assert np.array_equal(got["first_point"], np.sort(got["first_point"]))  # order of first appearance
    lead = got["first_point"]
    assert np.array_equal(got["voxel_id"][lead], np.arange(len(lead)))


def test_one_voxel(dev):
    """Maximal contention: 4096 points, one slot."""
    c = RS.one_voxel_case()
    got = _check(_fuse(c), _want(c), "one voxel")
    assert got["count"].tolist() == [4096] and got["n_frames"].tolist() == [4] and got["first_point"].tolist() == [0]
    assert (got["voxel_id"] == 0).all()
    assert got["colors"][0].tolist() == ((2 * c["colors"].astype(np.int64).sum(0) + 4096) // 8192).tolist()


def test_tight_table(dev):
    """About 800 voxels in 1024 slots: long probe chains; and the same map from the default table."""
    c = RS.tight_table_case()
    want = _want(c, min_frames=1)
    a = _check(_fuse(c, min_frames=1, table_capacity=1024), want, "tight table")
    b = _check(_fuse(c, min_frames=1), want, "default table")
    assert all(np.array_equal(a[k], b[k]) for k in RS.FIELDS)
    _check(_fuse(c, min_frames=2, table_capacity=1024), _want(c, min_frames=2), "tight table, two frames")


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.25, -0.5, 1.0)])
def test_edges(dev, origin):
    c = RS.edges_case(origin)
    for mf in (1, 2):
        want = _want(c, min_frames=mf)
        got = _check(_fuse(c, min_frames=mf), want, f"edges {origin} min_frames {mf}")
    k = want["counters"]
    assert (k["n_nonfinite"], k["n_masked"], k["n_out_of_range"], k["n_used"]) == (12, 10, 10, 44)
    n = len(c["points"]) // 2
    dropped = ~np.isfinite(c["points"][:n]).all(1) | (c["mask"][:n] > 0) | (c["keep"][:n] == 0)
    assert (got["voxel_id"][:n][dropped] == -1).all()
    # host numbers for the grid give the same map as the device tensor
    t = lambda x: torch.from_numpy(c[x]).cuda()  # noqa: E731
    res = SM.fuse_points(t("points"), t("colors"), 2, voxel_size=0.5, origin=origin, dyn_mask=t("mask"), keep=t("keep"))
    _check(res, want, "edges, host grid")
    # a grid without a positive finite voxel size holds nothing
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad = dict(c, grid=np.array(list(origin) + [v], dtype=np.float32))
        res = _check(_fuse(bad, min_frames=1), _want(bad, min_frames=1), f"edges, v = {v}")
        assert res["xyz"].shape == (0, 3) and (res["voxel_id"] == -1).all()


def test_frames_and_points_filters(dev):
    c = RS.frames_case()
    kept = {}
    for mf in (1, 2, 3):
        want = _want(c, min_frames=mf)
        got = _check(_fuse(c, min_frames=mf), want, f"min_frames {mf}")
        kept[mf] = len(got["count"])
        assert (got["n_frames"] >= mf).all()
        filtered = want["all"]["first_point"][~want["all"]["kept"]]
        assert (got["voxel_id"][filtered] == -1).all() and (got["voxel_id"] >= 0).sum() == got["count"].sum()
    assert kept == {1: 64, 2: 16, 3: 8}
    got = _check(_fuse(c, min_frames=2), _want(c, min_frames=2), "frames {0, 2}")
    two = got["n_frames"] == 2
    assert two.sum() == 8 and (got["first_frame"][two] == 0).all() and (got["last_frame"][two] == 2).all()
    assert (got["last_frame"][~two] == 3).all()
    for mp in (2, 3, 5):
        got = _check(_fuse(c, min_frames=1, min_points=mp), _want(c, min_frames=1, min_points=mp), f"min_points {mp}")
        assert len(got["count"]) == {2: 16, 3: 8, 5: 0}[mp]


def test_a_full_table_is_an_error_and_the_call_returns(dev):
    """200 voxels, 64 slots: the probe loop ends after 64 steps, the overflow is counted and raised."""
    c = RS.overflow_case()
    with pytest.raises(_lib.L4PHipError, match=r"table_capacity 64 .*n_voxels 64 "):
        _fuse(c, min_frames=1, table_capacity=64)
    _check(_fuse(c, min_frames=1, table_capacity=256), _want(c, min_frames=1), "after the overflow")


def test_input_dtype_layout_and_a_second_run_give_the_same_bits(dev):
    c = RS.scene_case(4, 5, 13, 17, 1.0)
    p, col = torch.from_numpy(c["points"]).cuda(), torch.from_numpy(c["colors"]).cuda()
    g, m = torch.from_numpy(c["grid"]).cuda(), torch.from_numpy(c["mask"]).cuda()

    def same(a, b, tag):
        assert a["counters"] == b["counters"] and a["counters"]["n_kept"] > 0, tag
        for k in RS.FIELDS:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (tag, k)

    first = SM.fuse_points(p, col, 5, grid=g, dyn_mask=m)
    same(first, SM.fuse_points(p, col, 5, grid=g, dyn_mask=m), "second run")
    half = p.half()
    same(SM.fuse_points(half, col, 5, grid=g, dyn_mask=m.half()), SM.fuse_points(half.float(), col, 5, grid=g, dyn_mask=m.half().float()), "f16")
    pv, cv = p.t().contiguous().t(), col.t().contiguous().t()
    assert not pv.is_contiguous() and not cv.is_contiguous()
    same(first, SM.fuse_points(pv, cv, 5, grid=g.double(), dyn_mask=m.reshape(5, 13, 17), keep=torch.ones(5, 13, 17, dtype=torch.bool, device="cuda")),
         "layout")


def _outputs(seed, T, H, W):
    """A synthetic (batch, out, tasks) of one clip around scene_flow_restate.make_case, as tests/test_scene_flow_gpu.py builds it."""
    c = SFRS.make_case(seed, 1, T, H, W)
    g = torch.Generator().manual_seed(seed)
    f = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    batch = {"rgb_b3thw": ((torch.randint(0, 256, (1, 3, T, H, W), generator=g).float() - 128) / 64).cuda(),
             "rgb_mean_b3111": torch.tensor((0.485, 0.456, 0.406)).reshape(1, 3, 1, 1, 1).cuda(),
             "rgb_std_b3111": torch.tensor((0.229, 0.224, 0.225)).reshape(1, 3, 1, 1, 1).cuda(), "seq_name": ["clip"]}
    out = {"depth_est_b1thw": f(c["depth"]), "flow_2d_backward_est_b2thw": f(c["flow"]), "dyn_mask_est_b1thw": f(c["mask"]),
           "traj3d_est_b16t": f(c["P"]).reshape(1, 16, T), "traj3d_intrinsics_est_b16t": f(c["K"]).reshape(1, 16, T)}
    return c, batch, out, ["depth", "flow_2d_backward", "dyn_mask", "camray"]


def test_from_outputs_is_fuse_points_on_reconstruct_4d(dev, tmp_path):
    T, H, W = 4, 17, 19
    c, batch, out, tasks = _outputs(31, T, H, W)
    res = SM.static_map_from_outputs(batch, out, tasks)
    rec = R.reconstruct_4d(batch, out, ["depth", "camray"])
    grid = res["grid"].cpu().numpy()
    v = 2.0 * float(np.median(c["depth"][0, 0, 0])) / float(c["K"][0, 0, 0, 0])  # H W is odd: the median is an element
    print(f"default grid {grid}, 2 median(depth_0) / fx_0 = {v:.9g}")
    assert grid.dtype == np.float32 and (grid[:3] == 0).all() and abs(float(grid[3]) - v) <= 1e-6 * v
    mask = out["dyn_mask_est_b1thw"].reshape(-1)
    again = SM.fuse_points(rec["points"], rec["colors"], T, grid=res["grid"], dyn_mask=mask)
    want = RS.restate(rec["points"].cpu().numpy(), rec["colors"].cpu().numpy(), T, grid, c["mask"].reshape(-1))
    got = _check(res, want, "from outputs")
    _check(again, want, "fuse_points on reconstruct_4d")
    k = res["counters"]
    assert k["n_kept"] > 0 and k["n_masked"] > 0 and k["n_points"] == T * H * W
    # a passed reconstruction, another voxel size, min_frames and a keep plane
    keep = torch.ones(1, 1, T, H, W, dtype=torch.uint8, device="cuda")
    keep[..., : W // 2] = 0
    res2 = SM.static_map_from_outputs(batch, out, tasks, voxel_px=3.0, min_frames=1, rec=rec, keep_b1thw=keep)
    g2 = res2["grid"].cpu().numpy()
    assert abs(float(g2[3]) - 1.5 * v) <= 1e-6 * 1.5 * v
    _check(res2, RS.restate(rec["points"].cpu().numpy(), rec["colors"].cpu().numpy(), T, g2, c["mask"].reshape(-1),
                            keep.cpu().numpy().reshape(-1), min_frames=1), "from outputs, keep plane")
    # files
    name = SM.generate_static_map(batch, out, tasks, str(tmp_path))
    assert name == os.path.join(str(tmp_path), "clip_static_map.ply")
    ply = R.read_ply(name)
    assert np.array_equal(ply["xyz"].view(np.uint8), got["xyz"].view(np.uint8)) and np.array_equal(ply["rgb"], got["colors"])
    info = json.load(open(os.path.join(str(tmp_path), "clip_static_map.json")))
    assert {n: info[n] for n in RS.COUNTERS} == k and info["min_frames"] == 2
    assert info["voxel_size"] == float(grid[3]) and info["compression"] == k["n_used"] / k["n_kept"]
    assert info["n_points"] == info["n_used"] + info["n_nonfinite"] + info["n_masked"] + info["n_out_of_range"]


def test_demo_static_map_branch(dev, tmp_path):
    """demo.run's static-map branch on a synthetic `out` (a run of demo.main builds the full-size model: not a few seconds)."""
    spec = importlib.util.spec_from_file_location("demo_static_map_run", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    T, H, W = 4, 16, 20
    _, batch, out, tasks = _outputs(32, T, H, W)
    d = str(tmp_path / "map")
    demo.static_map(batch, out, tasks, d)
    res = SM.static_map_from_outputs(batch, out, tasks)
    ply = R.read_ply(os.path.join(d, "clip_static_map.ply"))
    assert np.array_equal(ply["xyz"], res["xyz"].cpu().numpy()) and np.array_equal(ply["rgb"], res["colors"].cpu().numpy())
    info = json.load(open(os.path.join(d, "clip_static_map.json")))
    assert {n: info[n] for n in RS.COUNTERS} == res["counters"] and info["n_kept"] == len(ply["xyz"]) > 0
    assert info["n_points"] == T * H * W == info["n_used"] + info["n_nonfinite"] + info["n_masked"] + info["n_out_of_range"]
