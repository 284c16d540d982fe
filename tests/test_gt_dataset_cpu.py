"""CPU: the L4PDataset base class's host side (l4p_amd/data/l4p_dataset_mini.py) and the restatement the GPU tests compare
with (tests/gt_dataset_restate.py) against the fixture the REAL reference class wrote (tests/golden/gt_dataset.npz)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import gt_dataset_restate as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return gr.load_golden()


@pytest.mark.parametrize("name", list(gr.CASES))
def test_restatement_matches_the_reference_fixture(golden, name):
    case = gr.CASES[name]
    torch.manual_seed(case["manual_seed"])
    r = gr.restate(gr.case_raw(case), **case["ctor"], strings=dict(dataset_name="synthetic", seq_name=name))
    assert list(r["_offsets"]) == golden[name + ".offsets"].tolist()
    gr.compare_with_fixture(golden, name, r)
    if name == "A":
        assert r["track_2d_pointquerries_bn3"].shape[0] == 3 and len(r["_kept"]) == 3  # 3 of the 9 queries survive the crop
    if name == "G":
        assert r["_kept"] is None and r["track_2d_pointquerries_bn3"].shape[0] == 9


def test_frame_table_equals_the_iterated_mirror_padding():
    from l4p_amd.data.l4p_dataset_mini import frame_table

    for T0 in range(2, 7):
        for target in range(1, 18):
            # frames labelled (frame, direction): backward = direction 0, forward = direction 1
            x = {"rgb_b3thw": np.arange(T0, dtype=np.float32).reshape(1, T0, 1, 1),
                 "flow_2d_backward_b2thw": np.stack([np.arange(T0), np.zeros(T0)]).astype(np.float32).reshape(2, T0, 1, 1),
                 "flow_2d_forward_b2thw": np.stack([np.arange(T0), np.ones(T0)]).astype(np.float32).reshape(2, T0, 1, 1)}
            x["flow_2d_backward_valid_b2thw"], x["flow_2d_forward_valid_b2thw"] = x["flow_2d_backward_b2thw"], x["flow_2d_forward_b2thw"]
            p = gr.pad(x, target)
            tab = frame_table(T0, target)
            assert len(tab) == p["rgb_b3thw"].shape[1] >= min(target, len(tab))
            assert [f for f, _ in tab] == p["rgb_b3thw"][0, :, 0, 0].astype(int).tolist()
            bwd, fwd = p["flow_2d_backward_b2thw"][:, :, 0, 0], p["flow_2d_forward_b2thw"][:, :, 0, 0]
            assert [(int(f), int(d)) for f, d in bwd.T] == [(f, s) for f, s in tab]
            assert [(int(f), int(d)) for f, d in fwd.T] == [(f, 1 - s) for f, s in tab]
    assert frame_table(1, 4) == [(0, 0)] * 4
    tab = frame_table(5, 16)  # 5 -> 9 -> 17: two mirror rounds, the second one flips the parities of the first in reverse
    assert len(tab) == 17 and [s for _, s in tab] == [0] * 5 + [1] * 4 + [0] * 3 + [1] * 5


def test_crop_offsets_are_drawn_in_the_reference_order(golden):
    from l4p_amd.data.l4p_dataset_mini import draw_crop_offsets

    torch.manual_seed(11)
    want = [int(torch.randint(0, 3, (1,))[0]), int(torch.randint(0, 5, (1,))[0]), int(torch.randint(0, 7, (1,))[0])]
    torch.manual_seed(11)
    assert list(draw_crop_offsets((3, 5, 7), False, False)) == want
    torch.manual_seed(11)  # t0 is drawn and then overridden: i0 and j0 are the SECOND and THIRD draws
    assert list(draw_crop_offsets((3, 5, 7), False, True)) == [0] + want[1:]
    torch.manual_seed(11)  # nothing is drawn for an axis without slack; a centre crop draws t0 only
    a = int(torch.randint(0, 3, (1,))[0])
    b = int(torch.randint(0, 7, (1,))[0])
    torch.manual_seed(11)
    assert list(draw_crop_offsets((3, 0, 7), False, False)) == [a, 0, b]
    torch.manual_seed(11)
    assert list(draw_crop_offsets((3, 5, 7), True, False)) == [a, 2, 3]
    nxt = int(torch.randint(0, 1000, (1,))[0])
    torch.manual_seed(11)
    torch.randint(0, 3, (1,))
    assert int(torch.randint(0, 1000, (1,))[0]) == nxt
    for name in ("A", "D"):  # the same seed gives the reference's offsets
        case = gr.CASES[name]
        torch.manual_seed(case["manual_seed"])
        T = 9  # 5 frames mirror-padded once
        rs = case["ctor"].get("resize_size", (10, 14))
        cs = case["ctor"]["crop_size"]
        assert list(draw_crop_offsets((T - cs[0], rs[0] - cs[1], rs[1] - cs[2]), False, False)) == golden[name + ".offsets"].tolist()


def test_raises_match_the_reference():
    raw = gr.case_raw(gr.CASES["A"])
    single = {k: (v[:, :1] if k in gr.DENSE else v[..., :1] if k in gr.TRACKS_T + gr.CAMERAS else v) for k, v in raw.items()}
    with pytest.raises(NotImplementedError, match="flow"):  # flow fields on a single-frame clip (:198-204)
        gr.make_dataset(single, crop_size=(4, 5, 6))[0]
    with pytest.raises(NotImplementedError, match="track_2d_point"):  # user queries with a resize factor != 1 (:286-288)
        gr.make_dataset(raw, crop_size=(6, 5, 6), resize_size=(7, 9))[0]
    no_q = {k: v for k, v in raw.items() if k != "track_2d_pointquerries_bn3"}
    with pytest.raises(NotImplementedError, match="track_2d_pointlabels_bn"):  # ... or point labels alone
        gr.make_dataset(no_q, crop_size=(6, 5, 6), resize_size=(7, 9))[0]
    with pytest.raises(AssertionError, match="Cropping Error"):  # a crop larger than the clip
        gr.make_dataset(raw, crop_size=(6, 11, 9))[0]
    for missing in ("flow_2d_forward_b2thw", "flow_2d_backward_valid_b2thw"):
        part = {k: v for k, v in raw.items() if k != missing}
        with pytest.raises(ValueError, match=missing):  # one flow direction while mirror padding is needed (KeyError there)
            gr.make_dataset(part, crop_size=(6, 7, 9))[0]
    from l4p_amd.data.l4p_dataset_mini import L4PDataset

    with pytest.raises(NotImplementedError):  # the base class has no clips of its own
        L4PDataset()[0]


def test_record_and_constructor_match_the_reference_surface():
    import dataclasses
    import inspect

    from l4p_amd.data.l4p_dataset_mini import L4PData, L4PDataset

    names = [f.name for f in dataclasses.fields(L4PData)]
    assert names[0] == "rgb_b3thw" and names[-2:] == ["dataset_name", "seq_name"] and len(names) == 21
    assert all(f.default is None for f in dataclasses.fields(L4PData)[1:])
    sig = inspect.signature(L4PDataset.__init__).parameters
    want = dict(crop_size=(16, 224, 224), track_2d_traj_per_sample=128, track_2d_vis_thr=4, track_2d_repeat_traj=True, center_crop=False,
                start_crop_time=False, resize_size=None, resize_mode={"rgb_b3thw": "trilinear"}, estimation_directions=[1, -1],
                traj_sampling_window=None, length_mutiply_of=8, track_2d_querry_sampling_version=None,
                track_2d_querry_sampling_spacing=0.02, remove_queries_outside_bounds=True, scaling_mode=None, device="cuda",
                scale_queries_on_resize=False)
    assert list(sig)[1:] == list(want) and all(sig[k].default == v for k, v in want.items())
    ds = L4PDataset(resize_size=7, resize_mode={"depth_b1thw": "trilinear"})
    assert ds.resize_size == (7, 7) and ds.resize_mode["depth_b1thw"] == "trilinear" and ds.resize_mode["flow_2d_forward_b2thw"] == "nearest"
    assert len(ds.resize_mode) == 10 and not hasattr(ds, "generate_point_qurries")


def test_reference_import_path_is_the_engine_module():
    import l4p.data.l4p_dataset_mini as alias  # ModuleNotFoundError before this module existed
    import l4p_amd.data.l4p_dataset_mini as real
    from l4p.data.l4p_dataset_mini import L4PData, L4PDataset
    from l4p_amd.data import NpzClipDataset

    assert alias is real and L4PDataset is real.L4PDataset and L4PData is real.L4PData
    assert issubclass(NpzClipDataset, L4PDataset) and issubclass(L4PDataset, torch.utils.data.Dataset)


def test_host_steps_leave_the_callers_tensors_alone():
    raw = gr.case_raw(gr.CASES["A"])
    ds = gr.make_dataset(raw, crop_size=(6, 7, 9), device="cpu")
    before = {k: v.clone() for k, v in ds.tensors.items()}
    sample, strings = ds.get_dict_with_valid_vals(ds.getitem_helper(0))
    assert strings == {"dataset_name": "synthetic", "seq_name": "clip"} and all(sample[k] is ds.tensors[k] for k in sample)
    cams = ds._cameras(sample, [1, 2, 3, 4, 3, 2], False, (0.7, 9 / 14), (1, 2, 2, 7, 9))
    assert all(np.array_equal(gr.bits(ds.tensors[k].numpy()), gr.bits(before[k].numpy())) for k in before)
    # ... and compute what the restatement computes: resize (:281-285), then the crop shift (:386-388)
    k = gr.intrinsics_resize(raw["intrinsics_b44t"][..., [1, 2, 3, 4, 3, 2]], (0.7, 9 / 14))
    k[0, 2] -= np.float32(2)
    k[1, 2] -= np.float32(2)
    assert np.array_equal(cams["intrinsics_b44t"].numpy(), k)
    assert np.array_equal(cams["extrinsics_b44t"].numpy(), raw["extrinsics_b44t"][..., [1, 2, 3, 4, 3, 2]])
    with pytest.raises(Exception, match="GPU"):  # the per-element work has no CPU fallback
        ds[0]


def test_npz_dataset_reads_raw_clips(tmp_path):
    from l4p_amd.data import NpzClipDataset

    raw = gr.case_raw(gr.CASES["A"])
    raw8 = dict(raw, rgb_b3thw=np.rint(raw["rgb_b3thw"] * 255).astype(np.uint8), not_a_field=np.zeros(3))
    np.savez(tmp_path / "b.npz", **raw)
    np.savez(tmp_path / "a.npz", **raw8)
    ds = NpzClipDataset(str(tmp_path), crop_size=(6, 7, 9))
    assert len(ds) == 2
    a, b = ds.getitem_helper(0), ds.getitem_helper(1)
    assert (a.seq_name, b.seq_name, a.dataset_name) == ("a", "b", "npz")
    assert a.rgb_b3thw.dtype == torch.float32 and torch.equal(a.rgb_b3thw, torch.from_numpy(raw8["rgb_b3thw"]).float().div(255))
    assert torch.equal(b.rgb_b3thw, torch.from_numpy(raw["rgb_b3thw"])) and b.track_2d_vis_bn1t.dtype == torch.bool
    assert np.array_equal(b.depth_b1thw.numpy().view(np.uint32), raw["depth_b1thw"].view(np.uint32))


def test_evaluate_npz_to_batch_is_unchanged():
    spec = importlib.util.spec_from_file_location("evaluate_mod", os.path.join(ROOT, "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    arrays = {"rgb_b3thw": np.zeros((3, 2, 4, 4), np.float64), "track_2d_vis_bn1t": np.ones((5, 1, 2), bool),
              "ori_video_len": np.array(7), "seq_name": np.array("clip"), "dataset_name": np.array(["d"])}
    b = ev.npz_to_batch(arrays)
    assert b["rgb_b3thw"].dtype == torch.float32 and tuple(b["rgb_b3thw"].shape) == (1, 3, 2, 4, 4)
    assert b["track_2d_vis_bn1t"].dtype == torch.bool and tuple(b["track_2d_vis_bn1t"].shape) == (1, 5, 1, 2)
    assert b["ori_video_len"].dtype == torch.int64 and b["ori_video_len"].reshape(-1).tolist() == [7]
    assert b["seq_name"] == ["clip"] and b["dataset_name"] == ["d"] and list(b) == list(arrays)
    assert callable(ev.raw_loader)
