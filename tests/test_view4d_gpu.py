"""GPU: the free-viewpoint 4D renderer (l4p_amd/utils/view4d.py, csrc/view4d.hip through the C ABI) against the numpy
restatement of its rules (tests/view4d_restate.py) - bit for bit against the f32 restatement, within a stated count against the
f64 one - on the scene of tests/recon4d_restate.py (T = 24 frames of 32 x 32, 10 tracks) and on constructed edge cases.

Figures of the occlusion view (test 2), from the restatement: 24 192 pixel writes onto 2 232 covered pixels; the f32 restatement
differs from the f64 one at 10 of 6 144 pixels on the GPU's reconstruction, 13 on the host restatement's (near-equal depths whose
order the f32 rounding of z changes); the kernels, equal to the f32 restatement, differ at the same 10 on an MI355X; the bound on
the kernels against f64 is 0.5 % = 30 pixels."""
import os

import numpy as np
import pytest
import torch

from l4p_amd import _lib
from l4p_amd.ops import _p, _stream
from l4p_amd.utils import recon4d as R
from l4p_amd.utils import view4d as V4
from l4p_amd.utils import vis2d
from tests import recon4d_restate as RS
from tests import view4d_restate as VS

pytestmark = pytest.mark.gpu
TASKS = ["depth", "camray", "track_2d"]
T, HW = 24, 1024


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope="module")
def scene():
    sc = RS.make_scene()
    batch, out = RS.scene_tensors(sc, "cuda")
    rec = R.reconstruct_4d(batch, out, TASKS)
    return sc, batch, out, rec, _np(rec)


def _same(got, want, what=""):
    """image, index and the bits of depth, at every pixel."""
    g = _np(got)
    for k in ("index", "image"):
        bad = int((g[k] != want[k]).sum())
        print(what, k, "differs at", bad, "of", want[k].size)
        assert bad == 0, (what, k, bad)
    assert want["depth"].dtype == np.float32
    bad = int((g["depth"].view(np.int32) != want["depth"].view(np.int32)).sum())
    print(what, "depth bits differ at", bad)
    assert bad == 0, (what, "depth", bad)


def _off_axis(nrec):
    W = np.transpose(nrec["world_T_cam"][0], (2, 0, 1)).astype(np.float64)
    pose = W[12] @ V4._tz(2) @ V4._ry(0.35) @ V4._tz(-2) @ V4._tz(-1)
    return np.linalg.inv(pose)[None], (60.0, 56.0, 47.5, 32.0), (64, 96), [12], dict(point_size=0.12, max_half=6)


def test_identity_views_return_the_frames(scene):
    sc, _, _, rec, nrec = scene
    cams = rec["cam_T_ref"][0].permute(2, 0, 1).contiguous()  # the estimated cameras, world = frame 0's camera
    K = torch.from_numpy(np.stack([sc["K"][0], sc["K"][5], sc["K"][2], sc["K"][6]], 1))
    got = V4.render_4d_views(rec, T, HW, cams, K, (32, 32), torch.arange(T), point_size=0.0, tracks=False, frusta="none")
    assert torch.equal(got["image"], rec["colors"].reshape(T, 32, 32, 3))
    assert torch.equal(got["index"], torch.arange(HW, dtype=torch.int32, device="cuda").reshape(1, 32, 32).expand(T, 32, 32))
    assert got["image"].dtype == torch.uint8 and got["depth"].dtype == torch.float32 and got["index"].dtype == torch.int32
    _same(got, VS.render(nrec, T, HW, cams.cpu().numpy(), K.numpy(), (32, 32), np.arange(T), point_size=0.0, tracks=False, stride=-1),
          "identity")


def test_occlusion_off_axis(scene):
    _, _, _, rec, nrec = scene
    cam, K, size, frames, kw = _off_axis(nrec)
    got = V4.render_4d_views(rec, T, HW, cam, K, size, frames, frusta="none", **kw)
    want = VS.render(nrec, T, HW, cam, K, size, frames, stride=-1, **kw)
    assert (want["writes"], want["covered"]) == (24192, 2232)
    _same(got, want, "occlusion")
    w64 = VS.render(nrec, T, HW, cam, K, size, frames, stride=-1, dtype=np.float64, **kw)
    diff = int((got["index"].cpu().numpy() != w64["index"]).sum())
    print("occlusion: index differs from the f64 restatement at", diff, "of", w64["index"].size, "pixels; the f32 restatement at",
          int((want["index"] != w64["index"]).sum()))
    assert diff <= 0.005 * w64["index"].size


def test_frusta(scene):
    _, _, _, rec, nrec = scene
    cam, K, size, frames, kw = _off_axis(nrec)
    for frusta, stride in ((4, 4), ("current", 0)):
        got = V4.render_4d_views(rec, T, HW, cam, K, size, frames, frusta=frusta, **kw)
        want = VS.render(nrec, T, HW, cam, K, size, frames, stride=stride, **kw)
        assert (want["index"] < -1).sum() > (100 if stride else 0)
        _same(got, want, f"frusta {frusta}")


def _plane_rec(n=16, z=2.0, K=(8.0, 8.0, 7.5, 7.5), T_=2):
    """T_ frames of an n x n plane of points at depth z, one per pixel of an n x n image under K and the identity camera."""
    yy, xx = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    P = np.stack([(xx - K[2]) * z / K[0], (yy - K[3]) * z / K[1], np.full_like(xx, z)], -1).reshape(-1, 3)
    g = np.random.default_rng(3)
    return {"points": np.tile(P, (T_, 1)).astype(np.float32), "colors": g.integers(0, 256, (T_ * n * n, 3), dtype=np.uint8),
            "frustum": np.zeros((T_, 8, 3), np.float32)}


def _dev(nrec):
    return {k: torch.from_numpy(v).cuda() for k, v in nrec.items()}


def test_a_triangle_in_front_of_a_point_wins_and_one_behind_it_loses():
    nrec = _plane_rec()
    v = R.frustum_camera_vertices()
    nrec["frustum"][0] = v + [-0.5, 0.0, 0.9]  # z 0.91 .. 1.55: in front of the plane at z = 2
    nrec["frustum"][1] = v + [0.6, 0.1, 2.5]  # z 2.51 .. 3.15: behind it
    K, eye = (8.0, 8.0, 7.5, 7.5), np.eye(4)[None]
    got = V4.render_4d_views(_dev(nrec), 2, 256, eye, K, (16, 16), [1], point_size=0.0, frusta=1)
    want = VS.render(nrec, 2, 256, eye, K, (16, 16), [1], point_size=0.0, stride=1)
    _same(got, want, "front / behind")
    idx, dep = got["index"][0].cpu().numpy(), got["depth"][0].cpu().numpy()
    tri = idx < -1
    codes = idx[tri].view(np.uint32) & 0x7FFFFFFF
    assert tri.sum() >= 4 and set((codes >> 4).tolist()) == {0}  # frame 0's frustum is seen, frame 1's nowhere
    assert (dep[tri] < 2.0).all() and (dep[tri] >= 0.9).all()
    assert np.array_equal(idx[~tri], np.arange(256, dtype=np.int32).reshape(16, 16)[~tri]) and (dep[~tri] == 2.0).all()
    far_centre = np.array([0.6, 0.1, 2.5 + R.FRUSTUM_FAR])  # the centre of frame 1's far face projects onto a pixel the plane holds
    px, py = int(np.floor(8 * far_centre[0] / far_centre[2] + 7.5 + 0.5)), int(np.floor(8 * far_centre[1] / far_centre[2] + 7.5 + 0.5))
    assert idx[py, px] == py * 16 + px
    # without the plane in front of it (near pushed past the plane) frame 1's frustum is what that pixel shows
    got2 = V4.render_4d_views(_dev(nrec), 2, 256, eye, K, (16, 16), [1], point_size=0.0, frusta=1, near=2.25)
    _same(got2, VS.render(nrec, 2, 256, eye, K, (16, 16), [1], point_size=0.0, stride=1, near=2.25), "behind, alone")
    i2 = got2["index"][0].cpu().numpy()
    assert i2[py, px] < -1 and ((int(i2[py, px]) & 0x7FFFFFFF) >> 4) == 1 and (i2 >= 0).sum() == 0


def _edge_rec():
    """Two frames of 32 hand-placed points (identity camera, K = (10, 10, 7.5, 7.5), 16 x 16 image), frame 0 with 5 trail points,
    frame 1 with none."""
    nan, inf = np.nan, np.inf
    pts = np.zeros((2, 32, 3), np.float32)
    pts[:, :, 2] = -1.0  # unused slots sit behind the camera
    pts[0, :22] = [
        [0.0, 0.0, 5e-4], [0.1, 0.1, -2.0], [nan, 0.0, 2.0], [0.0, inf, 2.0], [0.0, 0.0, -inf], [0.0, 0.0, inf],  # dropped (steps 2)
        [1000.0, 0.0, 0.002], [0.0, -1000.0, 0.002],  # beyond 2^20 (step 4)
        [-1.5, 0.0, 2.0], [1.7, 0.1, 2.0], [0.0, -1.5, 2.0], [0.1, 1.7, 2.0],  # straddle the left, right, top, bottom border
        [-1.5, -1.5, 2.0], [1.7, 1.7, 2.0], [-2.0, 0.0, 1.9], [-4.0, 0.0, 2.0],  # corners; centre outside reaching in; fully outside
        [0.05, 0.05, 0.25],  # at the max_half cap: ((1.2 * 10) / 0.25) * 0.5 = 24 > 3
        [0.5, -0.5, 3.0], [0.5, -0.5, 3.0], [0.52, -0.5, 3.0],  # equal z on one pixel: the lower index wins
        [-6e-4, -6e-4, 1e-3], [0.3, 0.3, 4.0]]  # z = near is kept
    pts[1, :3] = [[0.2, 0.2, 1.5], [0.2, 0.2, 1.5], [-0.4, 0.3, 2.5]]
    g = np.random.default_rng(5)
    trail = np.array([[0.5, -0.5, 3.0], [-0.8, 0.8, 1.0], [nan, nan, nan], [0.0, 0.0, 0.6], [1.6, -1.6, 2.0]], np.float32)
    return {"points": pts.reshape(-1, 3), "colors": g.integers(0, 256, (64, 3), dtype=np.uint8), "frustum": np.zeros((2, 8, 3), np.float32),
            "track_xyz": trail, "track_colors": g.integers(0, 256, (5, 3), dtype=np.uint8),
            "track_offsets": np.array([0, 5, 5], dtype=np.int64)}


@pytest.mark.parametrize("tracks", [True, False])
def test_edges(tracks):
    nrec = _edge_rec()
    K, eye = (10.0, 10.0, 7.5, 7.5), np.tile(np.eye(4)[None], (3, 1, 1))
    kw = dict(point_size=1.2, max_half=3, near=1e-3, background=(9, 200, 31))
    frames = [0, 1, 0]
    got = V4.render_4d_views(_dev(nrec), 2, 32, eye, K, (16, 16), frames, tracks=tracks, frusta="none", **kw)
    want = VS.render(nrec, 2, 32, eye, K, (16, 16), frames, tracks=tracks, stride=-1, **kw)
    _same(got, want, f"edges tracks={tracks}")
    idx, img = want["index"], want["image"]
    assert set(np.unique(idx[0]).tolist()) & set(range(8)) == set()  # the dropped points are nowhere
    assert 17 in idx[0] and 18 not in idx[0]  # equal z: the lower index
    assert (idx[0] == 16).sum() == 49  # the capped splat: 7 x 7
    assert (idx[0][:, 0] == 14).any() and 15 not in idx[0] and 20 in idx[0]  # reaching in from outside; fully outside
    assert (idx == -1).any() and (img[idx == -1] == [9, 200, 31]).all()
    assert (idx[1] >= 32).sum() == 0 and ((idx[0] >= 32).sum() > 0) == tracks  # frame 1 has no trail points
    assert np.array_equal(idx[0], idx[2])


def test_no_queries(scene):
    sc = scene[0]
    sc0 = dict(sc, traj=sc["traj"][:0], vis_logit=sc["vis_logit"][:0], track_depth=sc["track_depth"][:0])
    batch, out = RS.scene_tensors(sc0, "cuda")
    rec = R.reconstruct_4d(batch, out, TASKS)
    assert rec["track_xyz"].shape == (0, 3)
    nrec = _np(rec)
    cam, K, size, frames, kw = _off_axis(nrec)
    got = V4.render_4d_views(rec, T, HW, cam, K, size, frames, **kw)
    _same(got, VS.render(nrec, T, HW, cam, K, size, frames, stride=0, **kw), "no queries")
    assert int(got["index"].max()) < HW


def test_more_points_than_one_pass_of_the_grid():
    """The splat launches at most 2048 workgroups of 256 points per view and strides: 600 000 points, all but 3 000 behind the
    camera (the restatement loops over the survivors only), the survivors on both sides of point 2048 * 256."""
    g = np.random.default_rng(11)
    HW_ = 600_000
    pts = np.zeros((HW_, 3), np.float32)
    pts[:, 2] = -1.0
    keep = np.concatenate([g.choice(524288, 1500, replace=False), 524288 + g.choice(HW_ - 524288, 1500, replace=False)])
    pts[keep] = np.concatenate([g.uniform(-1.2, 1.2, (3000, 2)), g.uniform(1.0, 3.0, (3000, 1))], 1)
    nrec = {"points": pts, "colors": g.integers(0, 256, (HW_, 3), dtype=np.uint8), "frustum": np.zeros((1, 8, 3), np.float32)}
    K, eye, kw = (20.0, 20.0, 15.5, 15.5), np.eye(4)[None], dict(point_size=0.2, max_half=4)
    got = V4.render_4d_views(_dev(nrec), 1, HW_, eye, K, (32, 32), [0], frusta="none", **kw)
    _same(got, VS.render(nrec, 1, HW_, eye, K, (32, 32), [0], stride=-1, **kw), "strided")
    idx = got["index"].cpu().numpy()
    assert idx.max() >= 524288 and ((idx >= 0) & (idx < 524288)).any()


def test_chunking_and_determinism(scene):
    _, _, _, rec, nrec = scene
    cam, K, size, _, kw = _off_axis(nrec)
    W = np.transpose(nrec["world_T_cam"][0], (2, 0, 1)).astype(np.float64)
    cams = np.concatenate([cam] + [np.linalg.inv(W[t] @ V4._tz(2) @ V4._ry(a) @ V4._tz(-3))[None] for t, a in ((3, -0.3), (20, 0.2), (7, 0.0), (23, 0.5))])
    frames = [12, 3, 20, 7, 23]
    one = V4.render_4d_views(rec, T, HW, cams, K, size, frames, frusta=4, **kw)
    again = V4.render_4d_views(rec, T, HW, cams, K, size, frames, frusta=4, **kw)
    for budget in (8 * 64 * 96 * 2, 1):  # two views per chunk: 3 chunks; below one view: 5 chunks of one view
        parts = V4.render_4d_views(rec, T, HW, cams, K, size, frames, frusta=4, workspace_bytes=budget, **kw)
        for k in ("image", "depth", "index"):
            assert torch.equal(one[k], parts[k]), (budget, k)
    for k in ("image", "depth", "index"):
        assert torch.equal(one[k], again[k]), k
    assert all(int((one["index"][v] != -1).sum()) > 500 for v in range(5))  # every view does show the scene


def test_bad_arguments_are_refused():
    lib, st = _lib.load(), _stream()
    z = torch.empty(1, 8, 8, dtype=torch.int64, device="cuda")
    p = torch.zeros(4, 3, device="cuda")
    c = torch.zeros(4, 3, dtype=torch.uint8, device="cuda")
    M, K = torch.eye(4, device="cuda")[None].contiguous(), torch.tensor([[8.0, 8.0, 3.5, 3.5]], device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = lambda **o: lib.l4p_view_splat(st, _p(p), None, None, 1, 4, 0, _p(M), _p(K), _p(f), o.get("V", 1), 8, 8, o.get("ps", 0.1),  # noqa: E731
                                        o.get("mh", 4), o.get("near", 1e-3), _p(z))
    assert ok() == 0
    assert ok(V=0) == -1 and ok(ps=-1.0) == -1 and ok(ps=float("nan")) == -1 and ok(mh=65) == -1 and ok(mh=-1) == -1
    assert ok(near=0.0) == -1 and ok(near=float("nan")) == -1
    assert b"l4p_view_splat" in lib.l4p_last_error()
    assert lib.l4p_view_mesh(st, None, 1, _p(M), _p(K), _p(f), 1, 8, 8, 0, 1e-3, _p(z)) == -1
    assert lib.l4p_view_mesh(st, _p(p), 1, _p(M), _p(K), _p(f), 1, 8, 8, -1, 1e-3, _p(z)) == -1
    i, d, n = torch.empty(1, 8, 8, 3, dtype=torch.uint8, device="cuda"), torch.empty(1, 8, 8, device="cuda"), torch.empty(1, 8, 8, dtype=torch.int32, device="cuda")
    assert lib.l4p_view_resolve(st, _p(z), _p(c), None, None, 1, 4, 0, _p(f), 1, 8, 8, 0, 256, 0, _p(i), _p(d), _p(n)) == -1
    # a view of a frame outside [0, T) stays empty
    f[0] = 7
    assert ok() == 0
    assert lib.l4p_view_resolve(st, _p(z), _p(c), None, None, 1, 4, 0, _p(f), 1, 8, 8, 1, 2, 3, _p(i), _p(d), _p(n)) == 0
    assert (n == -1).all() and torch.isinf(d).all() and (i.reshape(-1, 3) == torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")).all()
    with pytest.raises(ValueError):
        V4.render_4d_views({"points": p, "colors": c}, 1, 4, M, K[0], (8, 8), [0, 0])


def test_generate_4D_video_writes_what_it_returns(scene, tmp_path):
    _, batch, out, rec, _ = scene
    frames, path = V4.generate_4D_video(batch, out, TASKS, str(tmp_path), n_views=6, size=(48, 64), frusta=4)
    assert frames.shape == (6, 48, 64, 3) and frames.dtype == np.uint8 and os.path.exists(path)
    orbit = V4.orbit_views(rec, out["depth_est_b1thw"], T, 6)
    assert orbit["frames"].tolist() == [0, 4, 8, 12, 16, 20]
    K = out["traj3d_intrinsics_est_b16t"].reshape(4, 4, T)[:, :, 0].cpu().numpy().astype(np.float64)
    img = V4.render_4d_views(rec, T, HW, orbit["cam_T_world"], V4.scaled_intrinsics(K, (32, 32), (48, 64)), (48, 64), orbit["frames"],
                             frusta=4)["image"]
    assert np.array_equal(frames, img.cpu().numpy())
    assert all(int((frames[v] != 0).any(-1).sum()) > 300 for v in range(6))  # the scene is in the picture
    try:
        import mediapy  # noqa: F401
    except ImportError:
        assert path == str(tmp_path / "scene_4d") and np.array_equal(vis2d.read_png_frames(path), frames)
    else:
        assert path == str(tmp_path / "scene_4d.mp4")
    assert V4.generate_4D_video(batch, out, TASKS, None, n_views=2, size=(16, 16))[1] is None
