"""CPU: the DAVIS / DyCheck datasets' host side.  The restatement (tests/datasets_restate.py) against the reference fixture
(tests/golden/datasets.npz, tools/gen_golden_datasets.py); the library's two host index rules against Pillow and torch themselves;
the composed mask tables against the materialised three-stage pipeline; the candidate cells against the reference's loop; the
synthetic-tree writers; the `l4p.data.davis` / `l4p.data.dycheck_dataset` alias imports; the demo's argument handling."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import datasets_restate as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "datasets.npz"))
TOL = 2e-6  # tests/test_preprocess_gpu.py TOL: ATen fuses some multiply-adds the float32 restatement does not

# (in, out) pairs of one axis: the DAVIS round trips 854 -> 224 -> 854 and 480 -> 224 -> 480, up-scales, odd sizes, identity, doubling
SIZE_PAIRS = [(854, 224), (224, 854), (480, 224), (224, 480), (120, 224), (224, 120), (214, 224), (224, 214), (7, 3), (3, 7),
              (135, 241), (241, 135), (100, 100), (50, 100), (101, 33), (33, 101), (1, 5), (5, 1), (298, 224), (640, 298),
              (1080, 224), (224, 1080), (1920, 298)]


def _check_sample_against_fixture(name, o, with_mask):
    assert np.array_equal(o["intrinsics_b44t"], GOLD[name + ".intrinsics_b44t"])
    assert o["intrinsics_b44t"].dtype == np.float32
    assert np.array_equal(o["track_2d_pointquerries_bn3"], GOLD[name + ".queries"])
    assert int(o["ori_video_len"]) == int(GOLD[name + ".ori_video_len"])
    rgb = o["rgb_b3thw"]
    assert list(rgb.shape) == GOLD[name + ".rgb_shape"].tolist()
    assert np.abs(rgb.reshape(-1)[GOLD[name + ".rgb_idx"]] - GOLD[name + ".rgb_val"]).max() <= TOL
    if with_mask:
        m = o["instanceseg_b1thw"]
        assert m.dtype == np.float32 and list(m.shape) == GOLD[name + ".mask_shape"].tolist()
        assert np.array_equal(np.packbits(m[0, 0].astype(np.uint8)), GOLD[name + ".mask_frame0_bits"])
        assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).digest() == GOLD[name + ".mask_sha256"].tobytes()
    else:
        assert np.array_equal(o["extrinsics_b44t"], GOLD[name + ".extrinsics_b44t"])


@pytest.mark.parametrize("name", list(dr.DAVIS_CASES))
def test_davis_restatement_matches_reference_fixture(name):
    c = dr.DAVIS_CASES[name]
    frames, masks = dr.case_inputs(name)
    o = dr.davis_sample(frames, dr.annotation_arrays(masks, c["mode"]), c["mode"], c["crop_size"], tuple(c["resize_size"]),
                        c["stride"], c["spacing"])
    _check_sample_against_fixture(name, o, True)
    assert "instanceseg_b1thw" in [str(k) for k in GOLD[name + ".keys"]] and str(GOLD[name + ".seq_name"]) == name


def test_fixture_cases_cover_what_they_are_named_for():
    M = {n: dr.seg_cells(c["spacing"]).shape[0] for n, c in dr.DAVIS_CASES.items()}
    for n in ("palette", "grey", "border", "crop_none"):
        assert 0 < GOLD[n + ".queries"].shape[0] < M[n], n          # a real selection
    for n in ("no_annotation", "thin"):
        assert GOLD[n + ".queries"].shape[0] == M[n], n             # nothing valid: all kept
    assert float(GOLD["no_annotation.mask_sum"]) == 0 and float(GOLD["thin.mask_sum"]) > 0
    assert GOLD["border.queries"][0].tolist() == [0.5, 0.5, 0.5]    # the corner candidate survives: geodesic border, not zero padding
    assert GOLD["crop_none.mask_shape"].tolist() == [1, 24, 224, 224]  # ceil(max(18, 16) / 8) * 8


@pytest.mark.parametrize("name", list(dr.DYCHECK_CASES))
def test_dycheck_restatement_matches_reference_fixture(name):
    c = dr.DYCHECK_CASES[name]
    frames, _ = dr.case_inputs(name)
    o = dr.dycheck_sample(frames, c["calibration"], c["crop_size"], tuple(c["resize_size"]), c["stride"], c["spacing"])
    _check_sample_against_fixture(name, o, False)
    keys = [str(k) for k in GOLD[name + ".keys"]]
    assert "instanceseg_b1thw" not in keys and "extrinsics_b44t" in keys and str(GOLD[name + ".seq_name"]) == "Dycheck_" + name


def _table(fn, a, b):
    from l4p_amd.data.video_dataset import _index_table

    return _index_table(fn, a, b)  # the library loads without a GPU; these are host functions


@pytest.mark.parametrize("a,b", SIZE_PAIRS)
def test_pil_nearest_table_is_pillows_resize_of_a_palette_image(a, b):
    Image = pytest.importorskip("PIL.Image")
    t = _table("l4p_pil_nearest_table", a, b)
    assert np.array_equal(t, dr.pil_nearest_index(a, b))
    for part in (np.arange(a) % 256, np.arange(a) // 256):  # low and high byte of the source index
        ramp = part.astype(np.uint8)
        h = np.asarray(Image.fromarray(np.tile(ramp[None], (2, 1)), mode="P").resize((b, 2), resample=Image.Resampling.BILINEAR))
        v = np.asarray(Image.fromarray(np.tile(ramp[:, None], (1, 2)), mode="P").resize((2, b), resample=Image.Resampling.BILINEAR))
        assert np.array_equal(h[0], ramp[t]) and np.array_equal(h[1], ramp[t])
        assert np.array_equal(v[:, 0], ramp[t]) and np.array_equal(v[:, 1], ramp[t])


@pytest.mark.parametrize("a,b", SIZE_PAIRS)
def test_torch_nearest_table_is_f_interpolate(a, b):
    t = _table("l4p_torch_nearest_table", a, b)
    assert np.array_equal(t, dr.torch_nearest_index(a, b))
    ramp = torch.arange(a, dtype=torch.float32)
    w = torch.nn.functional.interpolate(ramp[None, None, None, None, :].repeat(1, 1, 3, 2, 1), (3, 2, b), mode="nearest")
    h = torch.nn.functional.interpolate(ramp[None, None, None, :, None].repeat(1, 1, 3, 1, 2), (3, b, 2), mode="nearest")
    assert np.array_equal(w[0, 0, 1, 1].numpy().astype(np.int32), t) and np.array_equal(h[0, 0, 2, :, 0].numpy().astype(np.int32), t)


@pytest.mark.parametrize("H,W,pil,res,crop", [(480, 854, (224, 224), (224, 224), (224, 224)), (120, 214, (224, 224), (224, 224), (224, 224)),
                                              (135, 241, (298, 224), (298, 224), (224, 224)), (250, 260, (224, 224), (250, 260), (224, 224)),
                                              (224, 300, (224, 224), (224, 224), (224, 224))])
def test_composed_mask_tables_equal_the_materialised_pipeline(H, W, pil, res, crop):
    """ytab / xtab (Pillow round trip o torch nearest o crop, composed on the host) against the three stages run one after the other
    on an image whose pixels are their own (row, column), Pillow itself doing the round trip."""
    Image = pytest.importorskip("PIL.Image")
    from l4p_amd.data.video_dataset import mask_index_table

    i0, j0 = int((res[0] - crop[0]) * 0.5), int((res[1] - crop[1]) * 0.5)
    ytab = mask_index_table(H, pil[1], res[0], i0, crop[0])
    xtab = mask_index_table(W, pil[0], res[1], j0, crop[1])
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    got = []
    for idx in (rows, cols):
        parts = []
        for part in (idx % 256, idx // 256):
            im = Image.fromarray(part.astype(np.uint8), mode="P")
            im = im.resize(pil, resample=Image.Resampling.BILINEAR).resize((W, H), resample=Image.Resampling.BILINEAR)  # davis.py:101-102
            parts.append(np.asarray(im).astype(np.int64))
        full = torch.from_numpy((parts[0] + 256 * parts[1]).astype(np.float32))[None, None, None]
        if not (res[0] / H == 1.0 and res[1] / W == 1.0):
            full = torch.nn.functional.interpolate(full, (1, res[0], res[1]), mode="nearest")  # l4p_dataset_mini.py:266
        got.append(full[0, 0, 0, i0:i0 + crop[0], j0:j0 + crop[1]].numpy().astype(np.int64))
    assert np.array_equal(got[0], np.broadcast_to(ytab[:, None], crop)) and np.array_equal(got[1], np.broadcast_to(xtab[None, :], crop))
    # without the round trip (8-bit annotations): torch nearest + crop only
    assert np.array_equal(mask_index_table(H, None, res[0], i0, crop[0]), dr.torch_nearest_index(H, res[0])[i0:i0 + crop[0]])


@pytest.mark.parametrize("spacing", [0.02, 0.04, 0.05, 0.1, 0.25, 0.5])
def test_candidate_cells_equal_the_reference_loop(spacing):
    from l4p_amd.data.video_dataset import seg_cells

    got = seg_cells(spacing)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), dr.seg_cells(spacing))  # int(dummy[n, 1] * 224) per candidate
    assert int(got.max()) < 224


def test_erosion_restatement_border_rule():
    m = np.zeros((6, 7), dtype=np.float32)
    m[:3, :4] = 1
    er = dr.erosion3(m)
    want = np.zeros_like(m)
    want[:2, :3] = 1  # the border pixels survive: neighbours outside the image do not count
    assert np.array_equal(er, want)


def test_synthetic_trees_round_trip(tmp_path):
    pytest.importorskip("PIL.Image")
    from l4p_amd.data.davis import read_davis_sequence
    from l4p_amd.data.dycheck_dataset import read_dycheck_sequence
    from l4p_amd.data.synthetic import synthetic_masks, synthetic_video, write_davis_tree, write_dycheck_tree

    frames = synthetic_video(3, 5, 30, 44)
    masks = synthetic_masks(4, 5, 30, 44, "blob")
    assert set(np.unique(masks)) == {0, 1, 2}
    for mode in ("P", "L", "RGB"):
        root = write_davis_tree(str(tmp_path / ("davis_" + mode)), "seq", frames, masks, mode)
        f, a, got_mode = read_davis_sequence(os.path.join(root, "JPEGImages", "480p", "seq"))
        assert got_mode == mode and np.array_equal(f, frames) and np.array_equal(a, dr.annotation_arrays(masks, mode))
    f, a, _ = read_davis_sequence(os.path.join(root, "JPEGImages", "480p", "seq"), stride=2)
    assert np.array_equal(f, frames[::2]) and a.shape[0] == 3
    # a sequence without annotations, and one where a single frame's annotation is missing
    root = write_davis_tree(str(tmp_path / "davis_none"), "seq", frames)
    assert read_davis_sequence(os.path.join(root, "JPEGImages", "480p", "seq"))[1] is None
    root = write_davis_tree(str(tmp_path / "davis_gap"), "seq", frames, [m if i != 2 else None for i, m in enumerate(masks)])
    a = read_davis_sequence(os.path.join(root, "JPEGImages", "480p", "seq"))[1]
    assert not a[2].any() and np.array_equal(a[3], masks[3])
    calib = (403.217, 398.06, 66.9, 91.325)
    root = write_dycheck_tree(str(tmp_path / "dycheck"), "apple", frames, calib)
    f, k = read_dycheck_sequence(os.path.join(root, "apple"), stride=2)
    assert np.array_equal(f, frames[::2]) and k == calib


def test_dataset_constructors_take_the_reference_arguments(tmp_path):
    import inspect

    from l4p_amd.data import DavisDataset, DycheckDataset

    ref = ["data_root", "dataset_type", "stride", "crop_size", "resize_size", "center_crop", "start_crop_time", "estimation_directions",
           "resize_mode", "track_2d_querry_sampling_spacing"]
    for cls in (DavisDataset, DycheckDataset):
        assert list(inspect.signature(cls.__init__).parameters)[1:11] == ref
        for kw in (dict(center_crop=False), dict(start_crop_time=False)):
            with pytest.raises(NotImplementedError):
                cls(data_root=str(tmp_path), **kw)
        assert len(cls(data_root=str(tmp_path))) == 0


def test_demo_import_lines_resolve_to_the_engine():
    code = ("from l4p.data.davis import DavisDataset\n"                    # demo.py:15
            "from l4p.data.dycheck_dataset import DycheckDataset\n"        # demo.py:17
            "import l4p_amd.data.davis as a, l4p_amd.data.dycheck_dataset as b, l4p_amd.data as d\n"
            "assert DavisDataset is a.DavisDataset is d.DavisDataset and DycheckDataset is b.DycheckDataset is d.DycheckDataset\n"
            "try:\n    import l4p.data.kubric\n    raise SystemExit('training datasets must not resolve')\nexcept ImportError:\n    pass\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_demo_argument_handling():
    code = ("import sys\nsys.path.insert(0, 'demo')\nimport demo\n"
            "a = demo.parse_args(['--synthetic', '--davis', 'X', '--vis', 'out'])\n"
            "t, kw = demo.plan(a)\n"
            "assert a.spacing == 0.02 and t == ['depth', 'flow_2d_backward', 'dyn_mask', 'track_2d'] and kw['crop_size'] == (64, 224, 224), (t, kw)\n"
            "t, kw = demo.plan(demo.parse_args(['--synthetic', '--davis', 'X', '--recon4d', 'out']))\n"
            "assert t[-1] == 'camray' and kw['crop_size'] == (56, 224, 224) and 'resize_size' not in kw, (t, kw)\n"
            "a = demo.parse_args(['--ckpt', 'c', '--dycheck', 'X', '--frames', '16'])\n"
            "t, kw = demo.plan(a)\n"
            "assert t[-1] == 'camray' and kw == dict(crop_size=(16, 224, 224), estimation_directions=[1], "
            "track_2d_querry_sampling_spacing=0.04, resize_size=(298, 224), stride=2), (t, kw)\n"
            "a = demo.parse_args(['--synthetic'])\n"
            "assert a.spacing == 0.04 and demo.plan(a)[0] == ['depth', 'flow_2d_backward', 'dyn_mask', 'track_2d']\n"
            "assert demo.parse_args(['--synthetic', '--davis', 'X', '--spacing', '0.1']).spacing == 0.1\n"
            "for bad in (['--davis', 'X'], ['--synthetic', '--davis', 'X', '--dycheck', 'Y'], ['--ckpt', 'c']):\n"
            "    try:\n        demo.parse_args(bad)\n        raise RuntimeError(bad)\n    except SystemExit:\n        pass\n"
            "import tempfile, os\n"
            "with tempfile.TemporaryDirectory() as tmp:\n"
            "    r = demo.synthetic_tree(demo.parse_args(['--synthetic', '--davis', 'X']), tmp)\n"
            "    assert os.path.isfile(os.path.join(r, 'JPEGImages', '480p', 'synthetic', '00000.jpg'))\n"
            "    assert os.path.isfile(os.path.join(r, 'Annotations', '480p', 'synthetic', '00019.png'))\n"
            "    r = demo.synthetic_tree(demo.parse_args(['--synthetic', '--dycheck', 'X']), tmp)\n"
            "    assert os.path.isfile(os.path.join(r, 'synthetic', 'calibration.txt'))\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-2000:])
