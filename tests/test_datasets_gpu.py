"""DavisDataset / DycheckDataset on the GPU (csrc/preprocess.hip through the C ABI) against the reference fixture
(tests/golden/datasets.npz) and the CPU restatement (tests/datasets_restate.py): masks, queries, intrinsics, extrinsics, keys and
dtypes exact; RGB bit-equal to the restatement and within 2e-6 of the reference's own values (tests/test_preprocess_gpu.py TOL, same
reason).  The selection kernel alone; a DAVIS-sized clip; the datasets end to end through DataLoader -> model.forward -> oracle."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib
from l4p_amd.data import DavisDataset, DycheckDataset
from l4p_amd.data import video_dataset as vd
from l4p_amd.data.synthetic import synthetic_masks, synthetic_video, write_davis_tree, write_dycheck_tree
from l4p_amd.ops import _p, _stream
from tests import datasets_restate as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "datasets.npz"))
TOL = 2e-6


def _check(name, s, o, seq_name):
    torch.cuda.synchronize()
    assert sorted(s.keys()) == [str(k) for k in GOLD[name + ".keys"]]
    got_dtypes = [str(s[k].dtype) if torch.is_tensor(s[k]) else type(s[k]).__name__ for k in sorted(s.keys())]
    assert got_dtypes == [str(d) for d in GOLD[name + ".dtypes"]]
    assert all(v.is_cuda and v.is_contiguous() for v in s.values() if torch.is_tensor(v))
    rgb = s["rgb_b3thw"].cpu().numpy()
    assert np.array_equal(rgb, o["rgb_b3thw"])                                                        # bit-equal to the restatement
    assert np.abs(rgb.reshape(-1)[GOLD[name + ".rgb_idx"]] - GOLD[name + ".rgb_val"]).max() <= TOL    # vs the reference itself
    for k, g in (("intrinsics_b44t", "intrinsics_b44t"), ("track_2d_pointquerries_bn3", "queries")):
        v = s[k].cpu().numpy()
        assert np.array_equal(v, GOLD[name + "." + g]) and np.array_equal(v, o[k]), k
    assert s["ori_video_len"] == int(GOLD[name + ".ori_video_len"]) == int(o["ori_video_len"])
    assert s["seq_name"] == seq_name == str(GOLD[name + ".seq_name"])
    N, Tn = s["track_2d_pointquerries_bn3"].shape[0], rgb.shape[1]
    assert s["track_2d_traj_bn2t"].shape == (N, 2, Tn) and not bool(s["track_2d_traj_bn2t"].any())
    assert s["track_2d_vis_bn1t"].shape == (N, 1, Tn) and not bool(s["track_2d_vis_bn1t"].any())
    assert s["track_2d_valid_bn1t"].shape == (N, 1, Tn) and not bool(s["track_2d_valid_bn1t"].any())
    assert s["track_2d_depth_bn1t"].shape == (N, 1, Tn) and float(s["track_2d_depth_bn1t"].min()) == 1.0
    assert s["track_2d_pointlabels_bn"].shape == (N,) and float(s["track_2d_pointlabels_bn"].min()) == 1.0
    assert s["rgb_mean_b3111"].shape == (3, 1, 1, 1) and s["rgb_std_b3111"].flatten().tolist() == torch.tensor(vd._STD).tolist()


@pytest.mark.parametrize("name", list(dr.DAVIS_CASES))
def test_davis_dataset_matches_fixture_and_restatement(dev, tmp_path, name):
    c = dr.DAVIS_CASES[name]
    frames, masks = dr.case_inputs(name)
    root = write_davis_tree(str(tmp_path / "davis"), name, frames, masks, c["mode"])
    ds = DavisDataset(data_root=root, stride=c["stride"], crop_size=c["crop_size"], resize_size=tuple(c["resize_size"]),
                      estimation_directions=[1], track_2d_querry_sampling_spacing=c["spacing"], device=dev)
    assert len(ds) == 1
    s = ds[0]
    o = dr.davis_sample(frames, dr.annotation_arrays(masks, c["mode"]), c["mode"], c["crop_size"], tuple(c["resize_size"]),
                        c["stride"], c["spacing"])
    _check(name, s, o, name)
    m = s["instanceseg_b1thw"].cpu().numpy()
    assert m.dtype == np.float32 and list(m.shape) == GOLD[name + ".mask_shape"].tolist()
    assert np.array_equal(m, o["instanceseg_b1thw"])
    assert np.array_equal(np.packbits(m[0, 0].astype(np.uint8)), GOLD[name + ".mask_frame0_bits"])
    assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).digest() == GOLD[name + ".mask_sha256"].tobytes()


def test_davis_rgb_annotation_reads_the_first_channel_in_place(dev, tmp_path):
    """An RGB 0/255 annotation (to_tensor(...)[:1], davis.py:104): three-channel bilinear passes, pixel stride 3 in the mask kernel."""
    c = dr.DAVIS_CASES["grey"]
    frames, masks = dr.case_inputs("grey")
    root = write_davis_tree(str(tmp_path / "davis"), "grey", frames, masks, "RGB")
    ds = DavisDataset(data_root=root, stride=c["stride"], crop_size=c["crop_size"], resize_size=tuple(c["resize_size"]),
                      track_2d_querry_sampling_spacing=c["spacing"], device=dev)
    s = ds[0]
    assert np.array_equal(np.packbits(s["instanceseg_b1thw"][0, 0].cpu().numpy().astype(np.uint8)), GOLD["grey.mask_frame0_bits"])
    assert np.array_equal(s["track_2d_pointquerries_bn3"].cpu().numpy(), GOLD["grey.queries"])


@pytest.mark.parametrize("name", list(dr.DYCHECK_CASES))
def test_dycheck_dataset_matches_fixture_and_restatement(dev, tmp_path, name):
    c = dr.DYCHECK_CASES[name]
    frames, _ = dr.case_inputs(name)
    root = write_dycheck_tree(str(tmp_path / "dycheck"), name, frames, c["calibration"])
    ds = DycheckDataset(data_root=root, stride=c["stride"], crop_size=c["crop_size"], resize_size=tuple(c["resize_size"]),
                        estimation_directions=[1], track_2d_querry_sampling_spacing=c["spacing"], device=dev)
    assert len(ds) == 1
    s = ds[0]
    o = dr.dycheck_sample(frames, c["calibration"], c["crop_size"], tuple(c["resize_size"]), c["stride"], c["spacing"])
    _check(name, s, o, "Dycheck_" + name)
    e = s["extrinsics_b44t"].cpu().numpy()
    assert np.array_equal(e, GOLD[name + ".extrinsics_b44t"]) and np.array_equal(e, o["extrinsics_b44t"])


def _select(mask, cells, dev):
    M = cells.shape[0]
    m = torch.from_numpy(mask).to(dev)
    cd = torch.from_numpy(cells).to(dev)
    sel = torch.full((M,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().l4p_seg_query_select(_stream(), _p(m), mask.shape[0], mask.shape[1], _p(cd), M, _p(sel), _p(count)),
               "l4p_seg_query_select")
    torch.cuda.synchronize()
    n = int(count.item())
    return sel.cpu().numpy(), n


@pytest.mark.parametrize("M", [1, 625, 2500, 10000])  # one candidate; the demo's spacings 0.04 / 0.02; many chunks of 256
def test_query_selection_kernel_alone(dev, M):
    rng = np.random.default_rng(M)
    h, w = 224, 231
    # blocky random masks (so that a 3x3 erosion leaves something), image borders included
    for density in (0.35, 0.7, 0.97):
        mask = np.kron(rng.random((h // 7 + 1, w // 7 + 1)) < density, np.ones((7, 7)))[:h, :w].astype(np.float32)
        cells = np.stack([rng.integers(0, w, M), rng.integers(0, h, M)], axis=1).astype(np.int32)
        cells[0] = (0, 0)
        cells[-1] = (w - 1, h - 1)
        want = dr.select_over_seg(mask, cells)
        sel, n = _select(mask, cells, dev)
        assert n == want.size and np.array_equal(sel[:n], want), (M, density)  # the same candidates in ascending order
        if n < M:
            assert 0 < n and (sel[n:] == -7).all()  # nothing written past the count
    # nothing survives: the identity and count = M, written by the kernel itself
    for mask in (np.zeros((h, w), dtype=np.float32), np.eye(h, w, dtype=np.float32)):
        sel, n = _select(mask, cells, dev)
        assert n == M and np.array_equal(sel, np.arange(M))
    # everything survives
    sel, n = _select(np.ones((h, w), dtype=np.float32), cells, dev)
    assert n == M and np.array_equal(sel, np.arange(M))


def test_query_selection_on_the_spacing_grid(dev):
    mask = synthetic_masks(5, 1, 224, 224, "blob")[0].astype(np.float32).clip(0, 1)
    for spacing in (1.0, 0.04, 0.02):
        got = vd.select_queries_over_seg(torch.from_numpy(mask).to(dev), spacing).cpu().numpy()
        assert np.array_equal(got, dr.select_over_seg(mask, dr.seg_cells(spacing))), spacing


def test_davis_sized_clip(dev):
    """50 frames of 480 x 854 -> 56: the mirrored mask frames are bitwise copies of their sources; mask and the number of queries
    equal the restatement's."""
    frames = synthetic_video(41, 50, 480, 854)[:, ::1]
    masks = synthetic_masks(42, 50, 480, 854, "blob")
    s = vd.prepare_clip(torch.from_numpy(frames).to(dev), (56, 224, 224), (224, 224), None, 1, 0.02, seq_name="bear",
                        annotations=torch.from_numpy(masks).to(dev), annotation_mode="P", sampling="uniform_over_seg")
    o = dr.davis_sample(frames, masks, "P", (56, 224, 224), (224, 224), 1, 0.02, rgb=False)
    m = s["instanceseg_b1thw"]
    assert m.shape == (1, 56, 224, 224)
    for t in range(50, 56):  # frames 50..55 mirror 48..43
        assert torch.equal(m[0, t], m[0, 98 - t]), t
    assert np.array_equal(m.cpu().numpy(), o["instanceseg_b1thw"])
    N = s["track_2d_pointquerries_bn3"].shape[0]
    assert 0 < N < 2500 and N == o["track_2d_pointquerries_bn3"].shape[0]
    assert np.array_equal(s["track_2d_pointquerries_bn3"].cpu().numpy(), o["track_2d_pointquerries_bn3"])
    assert s["track_2d_traj_bn2t"].shape == (N, 2, 56) and s["ori_video_len"] == 50


def test_error_behaviour(dev, tmp_path):
    frames, masks = dr.case_inputs("border")
    root = write_davis_tree(str(tmp_path / "davis"), "border", frames, masks, "P")
    with pytest.raises(ValueError, match="224"):  # l4p_dataset_mini.py:458-460 index the mask on a 224 grid
        DavisDataset(data_root=root, crop_size=(8, 112, 224), resize_size=(224, 224), device=dev)[0]
    with pytest.raises(ValueError, match="224"):
        DavisDataset(data_root=root, crop_size=(8, 224, 128), resize_size=(224, 224), device=dev)[0]
    for cls in (DavisDataset, DycheckDataset):
        for kw in (dict(center_crop=False), dict(start_crop_time=False)):
            with pytest.raises(NotImplementedError):
                cls(data_root=root, device=dev, **kw)
    with pytest.raises(_lib.L4PHipError):  # no CPU fall-back
        vd.prepare_clip(torch.from_numpy(frames), (8, 224, 224), (224, 224), annotations=torch.from_numpy(masks),
                        sampling="uniform_over_seg")


def test_datasets_to_model_forward(dev, tmp_path):
    """DataLoader(batch_size=1) -> model.forward -> oracle on the same prepared batch, mini geometry, exact f32 engine (as
    tests/test_demo_path_gpu.py): a DAVIS sample with the demo's tasks + camray (dummy intrinsics), a DyCheck sample with the camera
    file's intrinsics (use_intrinsics=True, demo.py:214-258).  One model for both."""
    from l4p_amd.weights import ModelCfg, seeded_state_dict
    from oracle.l4p_oracle import OracleModel
    from tests.test_encoder_dpt_gpu import build

    tasks = ["depth", "flow_2d_backward", "dyn_mask", "track_2d", "camray"]
    cfg = ModelCfg.mini()
    sd = seeded_state_dict(cfg)
    model = build(cfg, sd, "32-true")
    assert model.l4p_model.task_heads["camray"].use_intrinsics is True
    oracle = OracleModel(sd, cfg, use_intrinsics=True)
    frames = synthetic_video(51, 10, 96, 128)
    davis = DavisDataset(data_root=write_davis_tree(str(tmp_path / "davis"), "clip", frames, synthetic_masks(52, 10, 96, 128, "blob")),
                         crop_size=(16, 224, 224), estimation_directions=[1], track_2d_querry_sampling_spacing=0.25, device=dev)
    dycheck = DycheckDataset(data_root=write_dycheck_tree(str(tmp_path / "dycheck"), "clip", synthetic_video(53, 14, 181, 135),
                                                          (403.217, 398.06, 66.9, 91.325)),
                             resize_size=(298, 224), crop_size=(16, 224, 224), stride=2, track_2d_querry_sampling_spacing=0.5, device=dev)
    for ds, seq, nq in ((davis, "clip", None), (dycheck, "Dycheck_clip", 4)):
        batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)))
        assert batch["rgb_b3thw"].shape == (1, 3, 16, 224, 224) and batch["rgb_b3thw"].is_cuda and batch["seq_name"] == [seq]
        N = batch["track_2d_pointquerries_bn3"].shape[1]
        assert (0 < N < 16) if nq is None else N == nq  # DAVIS: a real selection on the mask
        with torch.no_grad():
            out = model.forward(batch, tasks)
            cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}
            ref = oracle.forward(cpu, tasks)
        torch.cuda.synchronize()
        for key in ("depth_est_b1thw", "flow_2d_backward_est_b2thw", "dyn_mask_est_b1thw", "track_2d_traj_est_bn2t",
                    "track_2d_vis_est_bn1t", "traj3d_est_b16t"):
            y, r = out[key].float().cpu(), ref[key].float()
            assert y.shape == r.shape, (seq, key)
            assert bool(torch.isfinite(y).all()), (seq, key)
            assert (y - r).abs().max() <= 1e-3 * r.abs().max(), (seq, key, float((y - r).abs().max() / r.abs().max()))
