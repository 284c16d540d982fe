"""GPU: the L4PDataset base class (l4p_amd/data/l4p_dataset_mini.py, csrc/gt_prep.hip) against the fixture the REAL reference
class wrote (tests/golden/gt_dataset.npz, tools/gen_golden_gt_dataset.py) and against the CPU restatement
(tests/gt_dataset_restate.py).

Everything gathered with nearest, every track field, the queries and the camera tensors equal the reference bit for bit (float
fields compared as uint32, so nan and inf entries count).  The trilinear fields equal the restatement bit for bit (nan for nan)
and the reference within TOL = 2e-6 * max(1, max |finite value|), the bound tests/test_preprocess_gpu.py uses for this arithmetic
(measured on the CPU restatement, which the kernel equals: <= 7.2e-7, the source coordinate's fused multiply-add in ATen)."""
import os

import numpy as np
import pytest
import torch

from tests import gt_dataset_restate as gr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def to_host(sample):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in sample.items()}


_samples = {}


def sample_of(name):
    """(device sample, restatement) of a case, computed once."""
    if name not in _samples:
        case = gr.CASES.get(name) or gr.CASE_J
        raw = gr.case_raw(case)
        strings = dict(dataset_name="synthetic", seq_name=name)
        torch.manual_seed(case["manual_seed"])
        s = gr.make_dataset(raw, name=name, **case["ctor"])[0]
        torch.manual_seed(case["manual_seed"])
        _samples[name] = (s, gr.restate(raw, **case["ctor"], strings=strings))
    return _samples[name]


@pytest.fixture(scope="module")
def golden():
    return gr.load_golden()


@pytest.mark.parametrize("name", list(gr.CASES))
def test_sample_equals_the_reference_and_the_restatement(golden, name):
    s, r = sample_of(name)
    for k, v in s.items():  # form: device, contiguity
        if torch.is_tensor(v):
            assert v.is_cuda and v.is_contiguous(), k
    got = to_host(s)
    gr.compare_with_fixture(golden, name, got)  # keys (sorted), dtypes, shapes; bits, or TOL for the trilinear fields
    for k, v in got.items():  # the restatement: every field bit for bit (a nan for a nan)
        if isinstance(v, np.ndarray):
            assert v.dtype == r[k].dtype and v.shape == r[k].shape, k
            nan = np.isnan(v) if v.dtype == np.float32 else np.zeros(v.shape, bool)
            assert np.array_equal(nan, np.isnan(r[k]) if v.dtype == np.float32 else nan), k
            assert np.array_equal(gr.bits(v)[~nan], gr.bits(r[k])[~nan]), k
        else:
            assert v == r[k], k
    if name == "A":
        assert got["track_2d_pointquerries_bn3"].shape[0] == 3  # the filter matters: 3 of 9 queries survive
    if name == "G":
        q = got["track_2d_pointquerries_bn3"]
        tr = got["track_2d_traj_bn2t"]
        assert q.shape[0] == 9 and ((q[:, 1] < 0) | (q[:, 1] > 9) | (q[:, 2] < 0) | (q[:, 2] > 7)).any()  # outside, and kept
        assert (got["track_2d_vis_bn1t"][:, 0] & ((tr[:, 0] < 0) | (tr[:, 0] >= 9))).any()  # no visibility clearing either


def test_callers_tensors_are_left_alone_on_either_device():
    case = gr.CASES["A"]
    raw = gr.case_raw(case)
    want = to_host(sample_of("A")[0])
    for device in ("cpu", "cuda"):
        ds = gr.make_dataset(raw, name="A", **case["ctor"])
        ds.tensors = {k: v.to(device) for k, v in ds.tensors.items()}
        before = {k: v.clone() for k, v in ds.tensors.items()}
        torch.manual_seed(case["manual_seed"])
        got = to_host(ds[0])
        for k in before:
            assert np.array_equal(gr.bits(ds.tensors[k].cpu().numpy()), gr.bits(before[k].cpu().numpy())), (device, k)
        for k, v in want.items():
            assert np.array_equal(gr.bits(got[k]), gr.bits(v)) if isinstance(v, np.ndarray) else got[k] == v, (device, k)


def _tracks(traj_xy, queries, T=1, **kw):
    """gt_tracks_clip on N hand-made single-point tracks [(x, y), ...] (every point visible and valid)."""
    from l4p_amd.data.l4p_dataset_mini import gt_tracks_clip

    N = len(traj_xy)
    dev = "cuda"
    traj = torch.tensor(traj_xy, dtype=torch.float32, device=dev)[:, :, None].repeat(1, 1, T).contiguous()
    ones = torch.ones((N, 1, T), dtype=torch.uint8, device=dev)
    ftab = torch.tensor([(t, 0) for t in range(T)], dtype=torch.int32, device=dev)
    q = torch.tensor(queries, dtype=torch.float32, device=dev)
    return gt_tracks_clip(traj, ones, ones.clone(), None, q, torch.ones(N, device=dev), None, ftab, **kw)


def test_boundaries_are_exclusive_for_queries_and_half_open_for_visibility():
    from l4p_amd.data.l4p_dataset_mini import gt_query_select

    t0, Tn, i0, Hn, j0, Wn = 2, 4, 3, 5, 1, 7
    inside = (3.5, 4.0, 5.0)
    q = [inside,
         (float(t0), 4.0, 5.0), (float(t0 + Tn), 4.0, 5.0),   # exactly at t0 and t0 + Tn
         (3.5, float(j0), 5.0), (3.5, float(j0 + Wn), 5.0),   # exactly at j0 and j0 + Wn
         (3.5, 4.0, float(i0)), (3.5, 4.0, float(i0 + Hn)),   # exactly at i0 and i0 + Hn
         (float(np.nextafter(F(t0), F(9))), float(np.nextafter(F(j0 + Wn), F(0))), float(np.nextafter(F(i0), F(9)))),  # one ulp inside
         (float("nan"), 4.0, 5.0)]
    sel = gt_query_select(torch.tensor(q, dtype=torch.float32, device="cuda"), t0, Tn, i0, Hn, j0, Wn)
    assert sel.dtype == torch.int32 and sel.cpu().tolist() == [0, 7]
    # trajectories after the shift at exactly Wn, -0.0 and the largest float below 0 (and the same for y against Hn)
    below = float(np.nextafter(F(0), F(-1)))
    xs = [float(Wn), -0.0, below, float(np.nextafter(F(Wn), F(0))), 0.0]
    out = _tracks([(x, 4.0) for x in xs] + [(2.0, y) for y in (float(Hn), -0.0, below)], [inside] * 8, crop=(t0, 0, 0, Hn, Wn))
    assert out["track_2d_vis_bn1t"][:, 0, 0].cpu().tolist() == [False, True, False, True, True, False, True, False]
    assert out["track_2d_valid_bn1t"].all() and out["track_2d_vis_bn1t"].dtype == torch.bool
    x_out = out["track_2d_traj_bn2t"][:5, 0, 0].cpu().numpy()
    assert np.array_equal(x_out.view(np.uint32), np.array(xs, dtype=F).view(np.uint32))  # (-0.0 - 0 stays -0.0)
    assert out["track_2d_pointquerries_bn3"][0].cpu().tolist() == [1.5, 4.0, 5.0]
    out = _tracks([(6.25, 4.5)], [inside], crop=(t0, i0, j0, Hn, Wn))  # the shift itself
    assert out["track_2d_traj_bn2t"][0, :, 0].cpu().tolist() == [5.25, 1.5] and out["track_2d_pointquerries_bn3"][0].cpu().tolist() == [1.5, 3.0, 2.0]
    # without a crop nothing is shifted or cleared
    out = _tracks([(x, 4.0) for x in xs], [inside] * 5)
    assert out["track_2d_vis_bn1t"].all() and out["track_2d_pointquerries_bn3"][0].cpu().tolist() == list(inside)
    # the causal fix compares the frame centre with the shifted query time, inclusively
    for causal, want in ((1, [False, True, True, True]), (-1, [True, True, False, False]), (0, [True] * 4)):
        out = _tracks([(3.0, 4.0)], [(3.5, 4.0, 5.0)], T=4, crop=(t0, i0, j0, Hn, Wn), causal=causal)
        assert out["track_2d_valid_bn1t"][0, 0].cpu().tolist() == want, causal


def test_ordered_compaction_across_rounds_and_empty_results():
    from l4p_amd.data.l4p_dataset_mini import gt_query_select, gt_tracks_clip

    dev = "cuda"
    box = (0, 4, 0, 8, 0, 8)  # t0, Tn, i0, Hn, j0, Wn
    for N, pattern in ((1, [True]), (1, [False]), (257, [n % 2 == 0 for n in range(257)]), (257, [n % 2 == 1 for n in range(257)]),
                       (600, [n % 7 in (0, 3, 4) for n in range(600)])):
        q = torch.tensor([(1.5, 2.0, 3.0) if keep else (1.5, 9.0, 3.0) for keep in pattern], dtype=torch.float32, device=dev)
        sel = gt_query_select(q, *box)
        assert sel.cpu().tolist() == [n for n in range(N) if pattern[n]], N  # ascending, and the count is their number
    # nothing kept: empty tensors of the reference's shapes, and nothing is launched for them
    q = torch.full((5, 3), 100.0, device=dev)
    sel = gt_query_select(q, *box)
    assert tuple(sel.shape) == (0,)
    T0 = 3
    ftab = torch.tensor([(0, 0), (1, 0), (2, 0), (1, 0)], dtype=torch.int32, device=dev)
    out = gt_tracks_clip(torch.zeros(5, 2, T0, device=dev), torch.ones(5, 1, T0, dtype=torch.uint8, device=dev),
                         torch.ones(5, 1, T0, dtype=torch.uint8, device=dev), torch.ones(5, 1, T0, device=dev), q,
                         torch.ones(5, device=dev), sel, ftab, crop=(0, 0, 0, 8, 8))
    shapes = {k: tuple(v.shape) for k, v in out.items()}
    assert shapes == {"track_2d_traj_bn2t": (0, 2, 4), "track_2d_vis_bn1t": (0, 1, 4), "track_2d_valid_bn1t": (0, 1, 4),
                      "track_2d_depth_bn1t": (0, 1, 4), "track_2d_pointquerries_bn3": (0, 3), "track_2d_pointlabels_bn": (0,)}
    assert out["track_2d_vis_bn1t"].dtype == torch.bool and out["track_2d_traj_bn2t"].dtype == torch.float32
    assert tuple(gt_query_select(torch.empty(0, 3, device=dev), *box).shape) == (0,)


def test_bad_arguments_are_refused():
    from l4p_amd import _lib

    lib = _lib.load()
    descs = (_lib.GtField * _lib.GT_MAX_FIELDS)()
    x = torch.zeros(8, device="cuda")
    tab = torch.zeros(8, dtype=torch.int32, device="cuda")
    p, t = x.data_ptr(), tab.data_ptr()
    assert lib.l4p_gt_dense_clip(None, descs, 11, 1, 2, 2, t, t, t, None, None, None, None, None, None, 1, 2, 2) == -1
    assert lib.l4p_gt_dense_clip(None, descs, 1, 1, 2, 2, t, t, t, None, None, None, None, None, None, 1, 2, 2) == -1  # no source
    descs[0].src, descs[0].out, descs[0].channels, descs[0].mode = p, p, 1, _lib.GT_BILINEAR
    assert lib.l4p_gt_dense_clip(None, descs, 1, 1, 2, 2, t, t, t, None, None, None, None, None, None, 1, 2, 2) == -1  # no tables
    assert b"bilinear" in lib.l4p_last_error()
    assert lib.l4p_gt_query_select(None, p, 0, 0, 1, 0, 1, 0, 1, 0, 1.0, 1.0, t, t) == -1
    assert lib.l4p_gt_tracks_clip(None, p, p, p, None, p, p, 2, 1, None, 3, t, 1, 0, 0, 1.0, 1.0, 0, 0, 0, 0, 1, 1, 0, p, p, p, None, p,
                                  p) == -1  # M > N
    assert lib.l4p_gt_tracks_clip(None, p, p, p, None, p, p, 2, 1, None, 1, t, 1, 0, 0, 1.0, 1.0, 0, 0, 0, 0, 1, 1, 2, p, p, p, None, p,
                                  p) == -1  # causal 2
    torch.cuda.synchronize()


def test_scale_queries_on_resize_extension():
    """User queries with a resize: NotImplementedError as in the reference; with the flag, the restatement's values."""
    case = gr.CASE_J
    raw = gr.case_raw(case)
    with pytest.raises(NotImplementedError):
        gr.make_dataset(raw, **dict(case["ctor"], scale_queries_on_resize=False))[0]
    s, r = sample_of("J")
    got = to_host(s)
    assert sorted(got) == sorted(k for k in r if not k.startswith("_"))
    assert 0 < got["track_2d_pointquerries_bn3"].shape[0] < 9
    for k, v in got.items():
        if isinstance(v, np.ndarray):
            nan = np.isnan(v) if v.dtype == np.float32 else np.zeros(v.shape, bool)
            assert v.shape == r[k].shape and np.array_equal(gr.bits(v)[~nan], gr.bits(r[k])[~nan]), k
        else:
            assert v == r[k], k
    assert np.array_equal(got["track_2d_pointlabels_bn"], np.ones(got["track_2d_pointlabels_bn"].shape, F))


def test_uniform_over_seg_sets_the_track_count():
    """sample_tracks "uniform_over_seg" through the base class: the existing mask selection on the prepared instance mask."""
    from l4p_amd.data.synthetic import synthetic_ground_truth
    from tests import datasets_restate as dr

    raw = synthetic_ground_truth(8, 3, 28, 32, 4)
    for k in gr.TRACKS_T + gr.QUERY:
        raw.pop(k)
    ds = gr.make_dataset(raw, crop_size=(8, 224, 224), resize_size=(224, 224), track_2d_querry_sampling_version="uniform_over_seg",
                      track_2d_querry_sampling_spacing=0.1)
    s = to_host(ds[0])
    keep = dr.select_over_seg(s["instanceseg_b1thw"][0, 0], dr.seg_cells(0.1))
    from oracle import preprocess_oracle as po

    assert 0 < keep.size < 100 and ds.track_2d_traj_per_sample == keep.size
    assert np.array_equal(s["track_2d_pointquerries_bn3"], po.grid_queries(0.1, 8, 224, 224)[keep])
    assert s["track_2d_traj_bn2t"].shape == (keep.size, 2, 8) and not s["track_2d_valid_bn1t"].any()


def test_end_to_end_raw_clips_to_test_step(tmp_path):
    """NpzClipDataset on two raw clips -> DataLoader(batch_size=1) -> test_step of the mini-geometry seeded model with L4PMetrics."""
    import importlib.util

    from l4p_amd.data import NpzClipDataset
    from l4p_amd.metrics import L4PMetrics
    from l4p_amd.models.utils import build_model
    from l4p_amd.weights import ModelCfg, seeded_state_dict
    from tests import metrics_restate as R

    spec = importlib.util.spec_from_file_location("evaluate_mod", os.path.join(ROOT, "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    ev.write_synthetic_raw(str(tmp_path))
    # what tools/evaluate.py --raw --resize 224 224 --crop 16 224 224 builds (raw_loader)
    ctor = dict(crop_size=(16, 224, 224), resize_size=(224, 224), center_crop=True, start_crop_time=True, estimation_directions=[1],
                track_2d_querry_sampling_version="uniform", track_2d_querry_sampling_spacing=0.02, scale_queries_on_resize=True)
    cfg = ModelCfg.mini()
    model = build_model(os.path.join(ROOT, "configs", "model.yaml"), max_queries=8, precision="32-true", model_cfg=cfg)
    for h in model.l4p_model.task_heads.values():
        if hasattr(h, "hooks_idx"):
            h.hooks_idx = list(cfg.hooks)
    model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(cfg).items()})
    model = model.eval()
    model.metrics_module = L4PMetrics()
    seen = {}
    model.metrics_module.register_forward_hook(lambda mod, args, output: seen.update(extras=output[1]))
    loader = ev.raw_loader(str(tmp_path), (224, 224), (16, 224, 224), 0.02, 0)
    assert isinstance(loader.dataset, NpzClipDataset) and loader.batch_size == 1
    assert all(getattr(loader.dataset, "length_multiply_of" if k == "length_mutiply_of" else k) == v for k, v in ctor.items())
    files = sorted(os.listdir(tmp_path))
    names = ("depth_abs_rel depth_rmse depth_delta1 depth_delta2 depth_delta3 flow_epe flow_1px flow_3px flow_5px dyn_mask_iou "
             "dyn_mask_precision dyn_mask_recall dyn_mask_f1 dyn_mask_accuracy track_2d_occlusion_accuracy "
             "track_2d_average_pts_within_thresh track_2d_average_jaccard camray_ate camray_rpe_trans camray_rpe_rot").split()
    names += [f"track_2d_{m}_{t}" for m in ("pts_within", "jaccard") for t in (1, 2, 4, 8, 16)]
    n = 0
    for i, batch in enumerate(loader):
        assert batch["seq_name"] == [files[i][:-4]] and tuple(batch["rgb_b3thw"].shape) == (1, 3, 16, 224, 224)
        assert batch["rgb_b3thw"].is_cuda and batch["ori_video_len"].tolist() == [9]
        with torch.no_grad():
            res = model.test_step(batch, i)
        for key in names:
            assert f"scalars/val/{key}" in model.last_log, key
        # the counts against the metric restatement on the restatement's batch (the model's own estimates)
        with np.load(tmp_path / files[i], allow_pickle=False) as z:
            raw = {k: z[k] for k in z.files}
        torch.manual_seed(0)
        r = gr.restate(raw, **ctor)
        M = r["track_2d_pointquerries_bn3"].shape[0]
        assert 0 < M == batch["track_2d_pointquerries_bn3"].shape[1]
        out = {k: v.float().cpu().numpy()[0] for k, v in res["out"].items() if torch.is_tensor(v)}
        ex = {k: v.cpu().numpy() for k, v in seen["extras"].items()}
        d = R.depth(out["depth_est_b1thw"], r["depth_b1thw"], r["depth_valid_b1thw"], "median")
        assert d["count"] > 0 and ex["depth_count"].tolist() == [d["count"]]
        m = R.mask(out["dyn_mask_est_b1thw"], r["dyn_mask_b1thw"], r["dyn_mask_valid_b1thw"])
        assert [ex[f"dyn_mask_{k}"].tolist() for k in ("tp", "fp", "fn", "tn")] == [[m[k]] for k in ("tp", "fp", "fn", "tn")]
        t = R.tracks(out["track_2d_traj_est_bn2t"], r["track_2d_traj_bn2t"], out["track_2d_vis_est_bn1t"].reshape(M, -1),
                     r["track_2d_vis_bn1t"].reshape(M, -1), r["track_2d_valid_bn1t"].reshape(M, -1), r["track_2d_pointquerries_bn3"],
                     (224, 224))
        assert t["count"] > 0
        for k in ("count", "count_occ_correct", "count_gt_visible"):
            assert ex[f"track_2d_{k}"].tolist() == [t[k]], k
        f = R.flow(out["flow_2d_backward_est_b2thw"], r["flow_2d_backward_b2thw"], r["flow_2d_backward_valid_b2thw"])
        assert ex["flow_count"].tolist() == [f["count"]]
        n += 1
    assert n == 2
