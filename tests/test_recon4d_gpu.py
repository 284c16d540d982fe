"""GPU: 4D reconstruction (l4p_amd/utils/recon4d.py, csrc/recon4d.hip) against the reference's recorded output
(tests/golden/recon4d_T24.npz) and the plain-torch restatement (tests/recon4d_restate.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from l4p_amd.utils import recon4d as R
from tests import recon4d_restate as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recon4d_T24")
TASKS = ["depth", "camray", "track_2d"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD + ".npz")
    g = {k: z[k] for k in z.files}
    sc = {k: g[k] for k in ("rgb_u8", "depth_q", "poses", "K", "traj", "vis_logit", "track_depth")}
    return g, json.load(open(GOLD + ".json")), sc


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_against(got, want, tracks=True, tol=1e-5):
    ext = RS.extent(want["points"])
    assert np.abs(got["points"] - want["points"]).max() <= tol * ext
    assert np.array_equal(got["colors"], want["colors"])
    assert np.abs(got["frustum"] - want["frustum"]).max() <= tol * RS.extent(want["frustum"])
    if tracks:
        assert np.array_equal(got["track_counts"], want["track_counts"])
        assert np.array_equal(got["track_offsets"], want["track_offsets"])
        assert np.array_equal(got["track_order"], want["track_order"])
        assert np.array_equal(got["track_colors"], want["track_colors"])
        assert np.abs(got["track_xyz"] - want["track_xyz"]).max() <= tol * max(ext, RS.extent(want["track_xyz"]))


def test_fixture_through_reconstruct_4d_and_files(gold, tmp_path):
    g, prov, sc = gold
    T, H, W = g["depth_q"].shape
    batch, out = RS.scene_tensors(sc, "cuda")
    rec = R.reconstruct_4d(batch, out, TASKS)
    got = _np(rec)
    # the scale is bit-equal to torch.median of the same f32 ratios (the restatement on the device) and to the reference's
    want = RS.restate(batch, out, TASKS)
    assert got["scale"].view(np.int32)[0] == want["scale"].view(np.int32)[0] == g["scale"].view(np.int32)[0]
    assert np.array_equal(got["track_counts"], g["vis_count"])
    _check_against(got, want)
    # against the reference's own points, frame by frame
    ext = RS.extent(g["track_xyz_0"])
    counts = []
    for t in range(T):
        a, b = got["track_offsets"][t], got["track_offsets"][t + 1]
        counts.append(H * W + b - a)
        if t in prov["keep_frames"]:
            pts = np.concatenate([got["points"][t * H * W:(t + 1) * H * W], got["track_xyz"][a:b]])
            col = np.concatenate([got["colors"][t * H * W:(t + 1) * H * W], got["track_colors"][a:b]])
            assert np.abs(pts - g[f"track_xyz_{t}"]).max() <= 1e-5 * ext, t
            assert np.array_equal(col, g[f"track_rgb_{t}"]), t
    assert np.array_equal(np.array(counts), g["track_count"])
    fr = np.asarray(g["track_frustum"])
    assert np.abs(got["frustum"] - fr).max() <= 1e-5 * RS.extent(fr)
    # generate_4D_visualization: side effect, return value, files
    for tasks, tag in ((TASKS, "track"), (TASKS[:2], "plain")):
        batch, out = RS.scene_tensors(sc, "cuda")
        ret = R.generate_4D_visualization(batch, out, tasks, str(tmp_path / tag))
        assert torch.equal(batch["intrinsics_b44t"], out["traj3d_intrinsics_est_b16t"].reshape(1, 4, 4, T))
        want_ret = [{k: v.replace(os.path.join("OUT", "scene"), str(tmp_path / tag / "scene")) for k, v in e.items()}
                    for e in prov["returns"][tag]]
        assert ret == want_ret
        for t in range(T):
            m = R.read_ply(ret[t]["mesh_cam"])
            assert np.array_equal(m["xyz"], got["frustum"][t]) and np.array_equal(m["faces"], R.FRUSTUM_TRIANGLES)
            assert np.array_equal(m["normals"], R.frustum_normals()) and (m["rgb"] == [255, 127, 127]).all()
            pc = R.read_ply(ret[t]["pc_depth_track" if tag == "track" else "pc_depth"])
            pts, col = got["points"][t * H * W:(t + 1) * H * W], got["colors"][t * H * W:(t + 1) * H * W]
            if tag == "track":
                a, b = got["track_offsets"][t], got["track_offsets"][t + 1]
                pts, col = np.concatenate([pts, got["track_xyz"][a:b]]), np.concatenate([col, got["track_colors"][a:b]])
            assert np.array_equal(pc["xyz"], pts) and np.array_equal(pc["rgb"], col), (tag, t)


def _demo_inputs(T=64, H=224, W=224, seed=5):
    """Demo-size seeded tensors (no model): 625 queries on a 25 x 25 grid (tied y at frame 0), drifting tracks, ~85 % visible."""
    g = torch.Generator().manual_seed(seed)
    n = 25
    gy, gx = torch.meshgrid(torch.linspace(4.48, 219.52, n), torch.linspace(4.48, 219.52, n), indexing="ij")
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    N = x0.numel()
    drift = torch.randn(N, 2, 1, generator=g) * torch.arange(T).float()[None, None] * 0.6
    traj = torch.stack([x0, y0], 1)[:, :, None] + drift
    traj[:, :, 0] = torch.stack([x0, y0], 1)
    logit = torch.randn(N, T, generator=g) * 1.0 + 2.3
    sc = {"rgb_u8": torch.randint(0, 256, (1, 3, T, H, W), generator=g, dtype=torch.uint8).numpy(),
          "depth_q": torch.randint(1, 256, (T, H, W), generator=g, dtype=torch.uint8).numpy(), "traj": traj.numpy(),
          "vis_logit": logit.numpy(), "track_depth": (torch.rand(N, T, generator=g) + 0.5).numpy()}
    s = RS.make_scene(T=T, H=8, W=8, N=4)
    K = s["K"].copy()
    K[0], K[5], K[2], K[6] = 200.0, 200.0, 111.5, 111.5
    sc.update(poses=s["poses"], K=K)
    return sc


def test_demo_size_against_the_restatement():
    sc = _demo_inputs()
    batch, out = RS.scene_tensors(sc, "cuda")
    got = _np(R.reconstruct_4d(batch, out, TASKS))
    y0 = out["track_2d_traj_est_bn2t"][0, :, 1, 0]
    assert np.array_equal(got["track_order"], torch.argsort(y0, stable=True).cpu().numpy())
    want = RS.restate(batch, out, TASKS)
    assert got["scale"].view(np.int32)[0] == want["scale"].view(np.int32)[0]
    _check_against(got, want)
    assert got["track_xyz"].shape[0] == got["track_offsets"][-1] > 5_000_000


def test_nearest_sample_indices_equal_grid_sample_on_adversarial_coordinates():
    from l4p_amd import _lib
    from l4p_amd.ops import _p, _stream

    H, W, T = 7, 9, 1
    dmap = (torch.arange(H * W, dtype=torch.float32) + 1).reshape(1, H, W).cuda()
    xs = []
    for size in (W, H):
        c = [-1.0, -0.5, -0.49999997, 0.0, 0.5, 1.5, 2.5, size - 1.5, size - 1.0, size - 0.5, size - 0.50000006, float(size), size + 3.0]
        # coordinates whose source index lands on k + 0.5 exactly after the reference's normalisation
        c += [((k + 0.5) * 2 + 1) / size * (size - 1) / 2 for k in range(-1, size + 1)]
        xs.append(torch.tensor(c))
    x = xs[0][:, None].expand(-1, len(xs[1])).reshape(-1)
    y = xs[1][None, :].expand(len(xs[0]), -1).reshape(-1)
    N = x.numel()
    traj = torch.stack([x, y], 1)[:, :, None].contiguous().cuda()  # [N, 2, 1]
    ones = torch.ones(N, 1, device="cuda")
    logit = torch.full((N, 1), 10.0, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    order, slot, counts, flag = torch.empty(N, **i32), torch.empty(1, N, **i32), torch.empty(1, **i32), torch.empty(1, **i32)
    ratios = torch.empty(1, N, device="cuda")
    off = torch.empty(3, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().l4p_recon_track_prep(_stream(), _p(traj), _p(logit), _p(ones), _p(dmap), N, T, H, W, 0.75, 16, 20,
                                                _p(order), _p(slot), _p(ratios), _p(flag), _p(counts), _p(off)))
    got = torch.empty(N, device="cuda")
    got[order.long()] = ratios[0]
    grid = torch.stack([traj[:, 0, 0] / (W - 1) * 2 - 1, traj[:, 1, 0] / (H - 1) * 2 - 1], -1).reshape(1, 1, N, 2)
    want = F.grid_sample(dmap[None], grid, mode="nearest", align_corners=False).reshape(-1)
    assert torch.equal(got, want), (traj[got != want, :, 0].tolist(), got[got != want].tolist(), want[got != want].tolist())


def test_zero_visible_pairs_give_nan_scale_and_no_trails(gold):
    _, _, sc = gold
    sc = dict(sc, vis_logit=np.full_like(sc["vis_logit"], -10.0))
    batch, out = RS.scene_tensors(sc, "cuda")
    got = _np(R.reconstruct_4d(batch, out, TASKS))
    assert np.isnan(got["scale"][0]) and got["track_xyz"].shape == (0, 3)
    assert (got["track_counts"] == 0).all() and (got["track_offsets"] == 0).all()


def test_end_to_end_mini_forward(tmp_path):
    from l4p_amd.models.utils import build_model
    from l4p_amd.weights import ModelCfg, seeded_state_dict
    from tests.golden_utils import make_batch

    cfg = ModelCfg.mini()
    tasks = ["depth", "camray", "track_2d"]
    model = build_model(os.path.join(ROOT, "configs", "model.yaml"), max_queries=8, precision="32-true", model_cfg=cfg)
    for h in model.l4p_model.task_heads.values():
        if hasattr(h, "hooks_idx"):
            h.hooks_idx = list(cfg.hooks)
    model.l4p_model.task_heads["camray"].use_intrinsics = True
    model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(cfg).items()})
    model = model.eval()
    batch = make_batch(24, 8)
    batch["rgb_mean_b3111"] = torch.tensor(RS.MEAN).reshape(1, 3, 1, 1, 1)
    batch["rgb_std_b3111"] = torch.tensor(RS.STD).reshape(1, 3, 1, 1, 1)
    with torch.no_grad():
        out = model.forward({k: v.clone() for k, v in batch.items()}, tasks)
    batch["seq_name"] = ["mini"]
    ret = R.generate_4D_visualization(batch, out, tasks, str(tmp_path))
    assert len(ret) == 24 and all(os.path.exists(e["pc_depth_track"]) and os.path.exists(e["mesh_cam"]) for e in ret)
    got = _np(R.reconstruct_4d(batch, out, tasks))
    want = RS.restate(batch, out, tasks)
    _check_against(got, want, tol=1e-4)
    for t in (0, 23):
        pc = R.read_ply(ret[t]["pc_depth_track"])
        a, b = got["track_offsets"][t], got["track_offsets"][t + 1]
        assert pc["xyz"].shape[0] == 224 * 224 + b - a
