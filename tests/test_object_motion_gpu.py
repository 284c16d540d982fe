"""GPU: object motion and models (l4p_amd/utils/object_motion.py, csrc/object_motion.hip) against the numpy restatement
(tests/object_motion_restate.py).

Integer part - n_pairs, n_inliers, n_far, valid, pose_valid and the 18 int64 moments: EQUAL, byte for byte, no tolerance.  (The
restatement's rotation is an SVD, the GPU's the closed form, so the two f32 models a refit tests against differ in the last bits;
tests/test_object_motion_cpu.py asserts of every clip here that no residual lies within 1e-3 tau of tau, so the inlier sets agree.)

Model, on valid rows (whose sigma2 / sigma1 >= 1e-3, asserted in the CPU file), against the restatement's float64 model:
  R     1e-6 per entry, t  1e-6 (|A| + |B|) with A, B the centroids t = B - R A is formed from (max norms) - the TOL["f32"] of
        tests/test_umeyama_moments_cpu.py: the outputs are f32;
  rms   1e-6 relative plus the cancellation floor q sqrt(8 eps64) max|d|: rms^2 / q^2 = (Sbb + Saa - 2 tr) / n is a difference of
        terms of up to 3 max|d|^2 + 3 max|d|^2 + 6 max|d|^2 = 12 max|d|^2 each rounded to eps64 / 2 relative, so the mean square is
        known to about 8 eps64 max|d|^2 (with the products and the divisions before it) and a residual near 0 to its square root;
        max|d| is the largest fixed-point offset of a counted pair of the row (rigid_scene: 480 steps of q = 1.95e-4 across a body
        of 0.7 units, max|d| ~ 2200: the floor is 1.8e-8 there against an rms of 1.4e-4);
  pose  the same bounds times the number of composed steps s: R s 1e-6; t s 1e-6 (S + 3 max|t_pose|), S the largest |A| + |B| of the
        object (each step adds the t bound and turns the translation so far by a rotation 1e-6 off per entry, three terms a row);
  canonical   the inverse pose applied to p: 3 s 1e-6 max|p| for the rotation, the pose's t bound, and 2^-23 |c| for the rounding.

Timing is not asserted anywhere."""
import json
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import object_motion as OM
from l4p_amd.utils import recon4d as R4
from l4p_amd.utils import static_map as SM
from tests import object_motion_restate as OR
from tests import static_map_restate as SMRS
from tests.test_moving_objects_gpu import _outputs
from tests.test_object_motion_cpu import ERR_R, ERR_T, MODEL_CAP, SMEAR_MIN

pytestmark = pytest.mark.gpu
TOL = 1e-6
EPS64 = 2.220446049250313e-16
OUT_FIELDS = ("motion", "n_pairs", "n_inliers", "n_far", "rms", "valid", "pose", "pose_valid", "canonical", "moments")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None


def _run(c, **kw):
    return OM.rigid_motion(_t(c["object_id"]), c["K"], _t(c["points"]), _t(c["grid"]), _t(c["flow"]), return_moments=True, **kw)


def _same_integers(got, want, tag):
    for k in OR.INT_FIELDS + ("pose_valid",):
        g, w = got[k].cpu().numpy(), np.ascontiguousarray(want[k]).astype(OR.DTYPES[k])
        assert g.dtype == OR.DTYPES[k] and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.shape)
        differ = int((np.ascontiguousarray(g).view(np.uint8) != w.view(np.uint8)).sum())
        print(f"{tag}: {k} {g.shape}: {differ} bytes differ")
        assert differ == 0, (tag, k)


def _same_model(got, want, c, tag):
    """The bounds of the module docstring; prints every figure before it asserts."""
    K, T = want["valid"].shape
    q = float(c["grid"][3]) / 256.0
    mo, rms, pose = (got[k].cpu().numpy().astype(np.float64) for k in ("motion", "rms", "pose"))
    assert got["motion"].dtype == torch.float32 and mo.shape == (K, T, 12) and pose.shape == (K, T, 12)
    valid = want["valid"].astype(bool)
    scale = np.abs(want["AB"]).max(axis=-1).sum(axis=-1)  # [K, T]: |A| + |B|
    err_r = np.abs(mo[..., :9] - want["motion64"][..., :9]).max(axis=-1)
    err_t = np.abs(mo[..., 9:] - want["motion64"][..., 9:]).max(axis=-1)
    tol_rms = TOL * want["rms"] + q * np.sqrt(8 * EPS64) * want["extent_d"] + 1e-45
    err_rms = np.abs(rms - want["rms"])
    print(f"{tag}: {int(valid.sum())} valid rows; R off by {err_r[valid].max() if valid.any() else 0:.3e}, t / (|A| + |B|) by "
          f"{(err_t[valid] / scale[valid]).max() if valid.any() else 0:.3e}, rms / bound by {(err_rms / tol_rms).max() if K else 0:.3e}")
    assert (err_r[valid] <= TOL).all() and (err_t[valid] <= TOL * scale[valid]).all(), tag
    assert (err_rms <= tol_rms).all(), tag
    # rows without a valid fit: R = I exactly, t = B - A (0 without pairs)
    assert np.array_equal(mo[~valid][:, :9], np.tile(OR.EYE12[:9], (int((~valid).sum()), 1))), tag
    assert (np.abs(mo[~valid][:, 9:] - want["motion64"][~valid][:, 9:]) <= TOL * np.maximum(scale[~valid], 1e-30)[:, None]).all(), tag
    none = want["n_inliers"] == 0
    assert not mo[none][:, 9:].any() and not rms[none].any(), tag
    # poses and canonical points
    ids = np.asarray(c["object_id"])
    HW = ids.shape[1] * ids.shape[2]
    canon, ref = got["canonical"].cpu().numpy(), want["canonical"]
    on = (ids.reshape(-1) >= 0) & (ids.reshape(-1) < K)
    assert np.isnan(canon[~on]).all(), tag
    pts = np.asarray(c["points"], dtype=np.float64)
    for k in range(K):
        present = [t for t in range(T) if (ids[t] == k).any()]
        first = present[0] if present else T
        S = float(scale[k].max())
        for t in range(T):
            s = max(0, t - first)
            tol_t = s * TOL * (S + 3 * np.abs(want["pose"][k, t, 9:]).max())
            assert np.abs(pose[k, t, :9] - want["pose"][k, t, :9]).max() <= s * TOL + 2.0 ** -24, (tag, k, t)
            assert np.abs(pose[k, t, 9:] - want["pose"][k, t, 9:]).max() <= tol_t + 2.0 ** -24 * np.abs(want["pose"][k, t, 9:]).max(), (tag, k, t)
            mm = np.nonzero(ids[t].reshape(-1) == k)[0] + t * HW
            fin = mm[np.isfinite(pts[mm]).all(axis=1)]
            if len(fin):
                bound = 3 * s * TOL * np.abs(pts[fin]).max(axis=1) + tol_t + 2.0 ** -23 * np.abs(ref[fin].astype(np.float64)).max(axis=1)
                assert (np.abs(canon[fin].astype(np.float64) - ref[fin]).max(axis=1) <= bound).all(), (tag, k, t)
            assert not np.isfinite(canon[np.setdiff1d(mm, fin)]).all(axis=1).any(), (tag, k, t)


CASES = OR.gpu_cases()
RESTATED = {}


def _want(name):
    """The restatement of a clip, computed once and shared."""
    if name not in RESTATED:
        c, kw = CASES[name]
        RESTATED[name] = OR.restate(c["object_id"], c["K"], c["points"], c["grid"], c["flow"], **kw)
    return RESTATED[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(dev, name):
    """Ragged and tiny clips with and without flow, NaN / Inf points and NaN flow; the serpentine at (3, 41, 150); runs that straddle
    the wave and workgroup boundaries; one frame; the edge rows; the rigid scene clean and corrupted."""
    c, kw = CASES[name]
    got, want = _run(c, **kw), _want(name)
    _same_integers(got, want, name)
    _same_model(got, want, c, name)


def test_ground_truth_motion(dev):
    """On rigid_scene the GPU's motion is as far from the true one as the restatement's, within 1e-6; with a tenth of the pairs
    corrupted the default single refit is back inside the bound and no refit is outside it."""
    for name, n_refits, inside in (("rigid", 1, True), ("rigid_corrupted", 1, True), ("rigid_corrupted", 0, False)):
        c, _ = CASES[name]
        got = _run(c, n_refits=n_refits)["motion"][0].cpu().numpy().astype(np.float64)
        ref = OR.restate(c["object_id"], 1, c["points"], c["grid"], c["flow"], n_refits=n_refits)["motion64"][0]
        (gr, gt), (rr, rt) = OR.motion_error(got, c["true"]), OR.motion_error(ref, c["true"])
        scale = float(np.abs(ref[:, 9:]).max()) + 1.0
        print(f"{name} n_refits={n_refits}: GPU off by {gr:.3e} / {gt:.3e}, restatement by {rr:.3e} / {rt:.3e}")
        assert gr <= rr + TOL and gt <= rt + TOL * scale
        assert ((gr <= ERR_R + TOL) and (gt <= ERR_T + TOL * scale)) == inside and ((gr > ERR_R) and (gt > ERR_T)) != inside


def test_edge_rows(dev):
    e, _ = CASES["edge"]
    got, k = _run(e), OR.EDGE_OBJECTS
    eye = torch.tensor(OR.EYE12, dtype=torch.float32, device="cuda")
    assert got["n_pairs"][k["few"]].tolist() == [0, 6, 6, 6, 6] and got["valid"][k["few"]].tolist() == [0] * 5
    assert torch.equal(got["motion"][k["few"], :, :9], eye[:9].expand(5, 9)) and got["motion"][k["few"], 1:, 9:].abs().max() > 0.01
    assert torch.equal(got["motion"][k["late"], :3], eye.expand(3, 12)) and torch.equal(got["pose"][k["late"], :3], eye.expand(3, 12))
    assert got["valid"][k["late"]].tolist() == [0, 0, 0, 1, 1] and got["pose_valid"][k["late"]].tolist() == [1] * 5
    assert got["pose_valid"][k["few"]].tolist() == [1, 0, 0, 0, 0]
    assert got["n_far"][k["far"]].tolist() == [0, 2, 2, 2, 2] and got["n_inliers"][k["far"]].tolist() == [0, 23, 23, 23, 23]
    # one frame: no pairs anywhere
    c, kw = CASES["one_frame"]
    one = _run(c, **kw)
    assert not one["n_pairs"].any() and torch.equal(one["pose"], eye.expand(c["K"], 1, 12)) and one["pose_valid"].all()
    # no objects: empty tables
    none = OM.rigid_motion(_t(np.full((2, 3, 4), -1, dtype=np.int32)), 0, _t(np.zeros((24, 3), dtype=np.float32)), _t(OR.GRID),
                           return_moments=True)
    assert none["motion"].shape == (0, 2, 12) and none["moments"].shape == (0, 2, 18) and none["valid"].shape == (0, 2)
    assert torch.isnan(none["canonical"]).all() and none["canonical"].shape == (24, 3)
    models = OM.object_models(dict(object_id=_t(np.full((2, 3, 4), -1, dtype=np.int32)), K=0, grid=_t(OR.GRID)), none,
                              torch.zeros(24, 3, dtype=torch.uint8, device="cuda"), 2)
    assert models["xyz"].shape == (0, 3) and models["offsets"] == [0] and OM.place_models(models, none["pose"], 0).shape == (0, 3)


def _rigid_res(c):
    ids = _t(c["object_id"])
    return dict(object_id=ids, K=1, grid=_t(c["grid"]), n_pixels=(ids.reshape(-1) == 0).sum().to(torch.int32).reshape(1))


def test_fused_model(dev):
    """object_models on rigid_scene: all frames fuse into hardly more voxels than frame 0 alone (cap 1.25), and into at least twice
    as many with the motion replaced by the identity.  The fusion is held equal to tests/static_map_restate.py on the GPU's own
    canonical points, and to the restatement's whole chain where the canonical points are bit-equal (counts only otherwise)."""
    c, _ = CASES["rigid"]
    T = c["object_id"].shape[0]
    got, want, res = _run(c), _want("rigid"), _rigid_res(c)
    colors = _t(c["colors"])
    md = OM.object_models(res, got, colors, T, min_frames=1)
    m = md["models"][0]
    keep = c["object_id"].reshape(-1) == 0
    first = keep & (np.arange(len(keep)) < len(keep) // T)
    n_first = SM.fuse_points(got["canonical"], colors, T, grid=res["grid"], keep=_t(first), min_frames=1)["counters"]["n_kept"]
    identity = dict(got, canonical=_t(c["points"]))
    n_identity = OM.object_models(res, identity, colors, T, min_frames=1)["models"][0]["counters"]["n_kept"]
    n_all = m["counters"]["n_kept"]
    print(f"fused model: {n_all} voxels from {T} frames, {n_first} from frame 0 alone, {n_identity} without the motion")
    assert n_first > 100 and n_all <= MODEL_CAP * n_first and n_identity >= SMEAR_MIN * n_first
    assert md["offsets"] == [0, n_all] and md["xyz"].shape == (n_all, 3) and (md["object"] == 0).all() and md["objects"] == [0]
    own = SMRS.restate(got["canonical"].cpu().numpy(), c["colors"], T, c["grid"], keep=keep, min_frames=1)
    for f in SMRS.FIELDS:
        assert np.array_equal(m[f].cpu().numpy(), own[f]), f
    ref = SMRS.restate(want["canonical"], c["colors"], T, c["grid"], keep=keep, min_frames=1)
    a, b = got["canonical"].cpu().numpy()[keep], want["canonical"][keep]
    if np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        for f in ("voxel_id", "count", "n_frames", "first_frame", "last_frame", "first_point", "key", "colors"):
            assert np.array_equal(m[f].cpu().numpy(), ref[f]), f
    else:
        print(f"canonical points differ in {int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())} of {len(a)} rows: counts only")
        assert ref["counters"]["n_kept"] <= MODEL_CAP * n_first
    # default min_frames = 2: the voxels two frames agree on
    two = OM.object_models(res, got, colors, T)["models"][0]["counters"]["n_kept"]
    assert 0 < two <= n_all


def test_place_models(dev):
    """A model carried to frame t lies on the frame's own object points: every vertex within a voxel's diagonal (its points' mean
    against one of them) plus 1e-3 of a point of frame t; and the frame's own canonical points carried forward land on its points
    within the f32 rounding of the two transforms (the rounded inverse, the rounded pose, three products and three sums each: 8 ulp of
    the largest magnitude involved)."""
    c, _ = CASES["rigid"]
    T, H, W = c["object_id"].shape
    got, res = _run(c), _rigid_res(c)
    md = OM.object_models(res, got, _t(c["colors"]), T, min_frames=1)
    v = float(c["grid"][3])
    pts = c["points"].reshape(T, H * W, 3)
    on = c["object_id"].reshape(T, H * W) == 0
    for t in range(T):
        placed = OM.place_models(md, got["pose"], t).cpu().numpy().astype(np.float64)
        own = pts[t][on[t]].astype(np.float64)
        near = np.sqrt(((placed[:, None, :] - own[None, :, :]) ** 2).sum(axis=-1)).min(axis=1)
        print(f"place_models frame {t}: {len(placed)} vertices, farthest {near.max():.4f} from the frame's points (voxel {v})")
        assert near.max() <= np.sqrt(3.0) * v + 1e-3
        idx = np.nonzero(on[t])[0] + t * H * W
        back = OM.place_models(dict(xyz=got["canonical"][_t(idx)], object=torch.zeros(len(idx), dtype=torch.int32, device="cuda")),
                               got["pose"], t).cpu().numpy().astype(np.float64)
        canon = got["canonical"][_t(idx)].cpu().numpy()
        scale = max(np.abs(own).max(), np.abs(canon).max()) + np.abs(got["pose"][0, t, 9:].cpu().numpy()).max()
        assert np.abs(back - own).max() <= 8 * 2.0 ** -23 * scale, (t, np.abs(back - own).max())  # (G G^-1 = I whatever G is)


def test_determinism(dev):
    """The largest clip of this file a second time: every output equal, byte for byte."""
    name = max(CASES, key=lambda n: CASES[n][0]["object_id"].size)
    assert CASES[name][0]["object_id"].shape == (3, 41, 150)
    c, kw = CASES[name]
    a, b = _run(c, **kw), _run(c, **kw)
    for k in OUT_FIELDS:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


def test_files_end_to_end(dev, tmp_path):
    T, H, W = 4, 32, 48
    _, batch, out, tasks = _outputs(33, T, H, W)
    res = OM.object_motion_from_outputs(batch, out, tasks)
    assert res["K"] >= 1 and res["motion"]["motion"].shape == (res["K"], T, 12) and res["motion"]["canonical"].shape == (T * H * W, 3)
    name = OM.generate_object_models(batch, out, tasks, str(tmp_path))
    assert name == os.path.join(str(tmp_path), "clip_object_motion.json")
    info = json.load(open(name))
    md = res["models"]
    ply = R4.read_ply(os.path.join(str(tmp_path), "clip_object_models.ply"))
    assert len(ply["xyz"]) == md["offsets"][-1] == info["n_vertices"] == sum(o["n_vertices"] for o in info["objects"])
    assert np.array_equal(ply["xyz"], md["xyz"].cpu().numpy()) and np.array_equal(ply["rgb"], md["colors"].cpu().numpy())
    assert info["n_objects"] == res["K"] == len(info["objects"])
    for o in info["objects"]:
        k = o["id"]
        for key in OM.TABLES:
            assert np.array_equal(np.array(o[key], dtype=res["motion"][key].cpu().numpy().dtype), res["motion"][key][k].cpu().numpy()), key
        c = md["models"][k]["counters"]
        assert o["counters"] == c and o["compression"] == (c["n_used"] / c["n_kept"] if c["n_kept"] else None)
    # the same through a result computed before, and without the flow
    assert OM.generate_object_models(batch, out, tasks, str(tmp_path / "again"), res=res) == os.path.join(str(tmp_path / "again"), "clip_object_motion.json")
    assert json.load(open(os.path.join(str(tmp_path / "again"), "clip_object_motion.json"))) == info
    no_flow = OM.object_motion_from_outputs(batch, out, [t for t in tasks if t != "flow_2d_backward"])
    assert no_flow["motion"]["n_pairs"].shape == (no_flow["K"], T)


def test_demo_object_models_branch(dev, tmp_path, capsys):
    """demo.run's object-models branch on a synthetic `out` (a run of demo.main builds the full-size model: not a few seconds)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("demo_object_models_run", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    _, batch, out, tasks = _outputs(34, 4, 32, 48)
    d = str(tmp_path / "models")
    demo.object_models(batch, out, tasks, d)
    info = json.load(open(os.path.join(d, "clip_object_motion.json")))
    ply = R4.read_ply(os.path.join(d, "clip_object_models.ply"))
    assert info["n_objects"] >= 1 and len(ply["xyz"]) == info["n_vertices"]
    assert f"object models: {info['n_objects']} objects" in capsys.readouterr().out


def test_sums_of_squares_past_2_63(dev):
    """A row of 2^20 pairs at the far bound (big_sums_case): the two sums of squares pass 2^63 and are read as unsigned; the rms of
    about 1.41 would come out as 0 if they were read as signed.  The rms bound of the module docstring is 0.09 here (max|d| = 2^21)."""
    c = OR.big_sums_case()
    got = _run(c, n_refits=0)
    want = OR.restate(c["object_id"], 1, c["points"], c["grid"], None, n_refits=0)
    _same_integers(got, want, "big sums")
    _same_model(got, want, c, "big sums")
    assert 1.3 < float(got["rms"][0, 1]) < 1.5
