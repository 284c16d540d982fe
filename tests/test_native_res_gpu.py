"""GPU: guided up-sampling to the video's own resolution (l4p_amd/utils/native_res.py, csrc/upsample.hip) against the numpy
restatement (tests/native_res_restate.py).

Pass rule of every comparison with the restatement: `valid` exactly equal (coordinates, `inside` and the window centre are f32 on
both sides, operation by operation), every channel within 1e-4 max|src[c]| of the float64 result.  Derivation: a weight above the
floor (range_floor = 1e-4) has an exponent below ln(1e4) = 9.2, so at sigma_r = 0.1 a colour distance below 0.43; the f32 rounding
of the three colour differences (values of at most 1, 6e-8 each) moves that exponent by at most about 2 * 0.43 * 3 * 6e-8 /
(2 sigma_r^2) = 1.5e-5, the spatial exponent by less.  Twice that, for numerator and denominator, plus about 35 roundings of 6e-8
for the sums of up to 49 taps, the hardware exponential and the division, is 3.5e-5 relative to the largest |src|; the bound leaves
3x over that.  A wrong tap, centre or coordinate costs 1e-2 or more."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from l4p_amd import _lib
from l4p_amd.data import VideoDataset
from l4p_amd.ops import _p, _stream
from l4p_amd.utils import native_res as NR
from l4p_amd.utils import vis2d
from tests import native_res_restate as RS
from tests.golden_utils import synthetic_video

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_BOUND = 1e-4
_CASES = {}


def _case(name):
    """(keyword arguments, restatement without the scale) of a parity case, computed once and left unchanged."""
    if name not in _CASES:
        kw = RS.parity_case(name)
        _CASES[name] = (kw, RS.restate(**dict(kw, scale=None)))
    return _CASES[name]


def _geometry(kw):
    _, _, H, W, _ = kw["guide_hi"].shape
    T, h, w = kw["src"].shape[2:]
    fidx = kw["frame_index"] if kw["frame_index"] is not None else range(T)
    return NR.ClipGeometry((H, W), tuple(kw["res_hw"]), tuple(kw["crop_ij"]), (h, w), tuple(fidx))


def _gpu(kw, scale=None, **knobs):
    """(out, valid) device tensors of the wrapper on a case's arrays."""
    knobs = {k: kw[k] for k in ("radius", "sigma_s", "sigma_r", "range_floor") if k in kw} | knobs
    return NR.guided_upsample(torch.from_numpy(kw["guide_hi"]).cuda(), torch.from_numpy(kw["guide_lo"]).cuda(),
                              torch.from_numpy(kw["src"]).cuda(), _geometry(kw), scale=scale, **knobs)


def _check(got, want, src, tag):
    """valid equal, every channel within REL_BOUND max|src[c]|, invalid pixels zero.  ``src``: the fields the bound is taken from."""
    (out, valid), (wout, wvalid) = got, want
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    assert out.shape == wout.shape and out.dtype == np.float32 and valid.shape == wvalid.shape and valid.dtype == np.uint8
    nv = int((valid != wvalid).sum())
    amp = np.abs(np.where(np.isfinite(src), src, 0)).max(axis=(0, 2, 3, 4))
    assert np.isfinite(out).all(), tag
    err = np.abs(out - wout).max(axis=(0, 2, 3, 4))
    print(f"{tag}: valid differs on {nv} of {valid.size}; largest error / max|src[c]| per channel "
          f"{', '.join(f'{e / a:.2e}' for e, a in zip(err, amp))} (bound {REL_BOUND:.0e})")
    assert nv == 0
    assert (err <= REL_BOUND * amp).all()
    assert (out[np.broadcast_to(valid == 0, out.shape)] == 0).all()
    return out, valid


@pytest.mark.parametrize("name", [c[0] for c in RS.PARITY_CASES])
def test_parity_with_the_restatement(dev, name):
    kw, want = _case(name)
    out_t, valid_t = _gpu(kw)
    _, valid = _check((out_t, valid_t), want, kw["src"], name)
    H, W = kw["guide_hi"].shape[2:4]
    if name == "c":  # the cropped-away columns
        _, in_x, _ = RS.coords(W, kw["res_hw"][1], kw["crop_ij"][1], kw["src"].shape[-1])
        assert 0 < in_x.sum() < W and not valid[..., ~in_x].any() and valid[..., in_x].all()
    else:
        assert valid.all()
    # the scale multiplies the f32 result: the same bits as the product formed afterwards
    s_t, v_t = _gpu(kw, scale=kw["scale"])
    assert torch.equal(v_t, valid_t)
    assert torch.equal(s_t, out_t * torch.from_numpy(kw["scale"]).cuda()[None, :, None, None, None])


def test_adversarial_inputs(dev):
    base, _ = _case("b")
    ref_t, refv_t = _gpu(base)
    ref, refv = ref_t.cpu().numpy(), refv_t.cpu().numpy()
    B, Cn, T, h, w = base["src"].shape
    H, W = base["guide_hi"].shape[2:4]
    geo = (H, W, base["res_hw"], base["crop_ij"], base["radius"])
    kw = dict(base, src=base["src"].copy(), guide_hi=base["guide_hi"].copy())
    changed = np.zeros((B, T, h, w), dtype=bool)
    inf, nan = float("inf"), float("nan")
    for (b, c, t, i, j), val in {(0, 0, 0, 3, 4): nan, (0, 2, 0, 8, 15): inf, (0, 3, 1, 0, 0): -inf, (1, 1, 2, 11, 19): nan,
                                 (1, 0, 2, 5, 9): inf}.items():  # single taps
        kw["src"][b, c, t, i, j] = val
        changed[b, t, i, j] = True
    kw["src"][1, 1, 0, 1:10, 4:15] = nan  # a block that covers whole 5 x 5 windows
    changed[1, 0, 1:10, 4:15] = True
    # guide pixels of a colour far from every tap of their window (frame (0, 2), whose taps are unchanged)
    far = [(2, 3), (11, 20), (17, 33), (22, 39), (0, 0), (9, 14)]
    x, _, cx = RS.coords(W, base["res_hw"][1], 0, w)
    y, _, cy = RS.coords(H, base["res_hw"][0], 0, h)
    lo = base["guide_lo"][0, :, 2].astype(np.float64) * np.asarray(RS.STD)[:, None, None] + np.asarray(RS.MEAN)[:, None, None]
    corners = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float64)
    for Y, X in far:  # the corner of the colour cube farthest from the window's taps: every range weight below the floor
        win = lo[:, max(cy[Y] - 2, 0):cy[Y] + 3, max(cx[X] - 2, 0):cx[X] + 3].reshape(3, -1)
        d2 = ((corners[:, :, None] - win[None]) ** 2).sum(axis=1).min(axis=1)
        assert d2.max() >= 0.25, (Y, X, d2.max())  # exp(-0.25 / 0.02) = 3.7e-6 < range_floor
        kw["guide_hi"][0, 2, Y, X] = (corners[d2.argmax()] * 255).astype(np.uint8)
    want = RS.restate(**dict(kw, scale=None))
    out, valid = _check(_gpu(kw), want, base["src"], "adversarial")
    # whole windows in the block: invalid and zero
    block = ~RS.window_hits(~changed[1, 0], *geo)  # no tap of the window outside the block
    assert block.sum() >= 20 and not valid[1, 0, 0][block].any() and (out[1, :, 0][:, block] == 0).all()
    assert valid.sum() == valid.size - block.sum()  # every other pixel keeps a usable tap
    # far colours: finite, and the spatial Gaussian alone
    spatial, _ = RS.restate(**dict(kw, scale=None, spatial_only=True))
    amp = np.abs(base["src"]).max(axis=(0, 2, 3, 4))
    for Y, X in far:
        assert (np.abs(want[0][0, :, 2, Y, X] - spatial[0, :, 2, Y, X]) <= 1e-9 * amp).all(), (Y, X)  # the scene: all taps at the floor
        assert np.isfinite(out[0, :, 2, Y, X]).all() and (np.abs(out[0, :, 2, Y, X] - spatial[0, :, 2, Y, X]) <= REL_BOUND * amp).all()
    # every pixel whose window meets no changed tap and whose own colour is unchanged keeps its bits
    same = np.zeros((B, T, H, W), dtype=bool)
    for b in range(B):
        for t in range(T):
            same[b, t] = ~RS.window_hits(changed[b, t], *geo)
    for Y, X in far:
        same[0, 2, Y, X] = False
    assert same.sum() > same.size // 2 and not same.all()
    assert np.array_equal(np.moveaxis(out, 1, 0)[:, same], np.moveaxis(ref, 1, 0)[:, same])
    assert np.array_equal(valid[:, 0][same], refv[:, 0][same])


def test_frame_index_out_of_range_is_invalid(dev):
    base, _ = _case("f")  # T = 5, Tg = 3
    ref, refv = _gpu(base)
    kw = dict(base, frame_index=(0, -1, 2, 3, 0))
    out, valid = _check(_gpu(kw), RS.restate(**dict(kw, scale=None)), base["src"], "frame_index")
    assert not valid[0, 0, 1].any() and not valid[0, 0, 3].any() and (out[0, :, [1, 3]] == 0).all()
    for t in (0, 2, 4):
        assert valid[0, 0, t].all()
        assert torch.equal(torch.from_numpy(out[0, :, t]), ref[0, :, t].cpu())


@pytest.mark.parametrize("shape", RS.EDGE_SHAPES)
def test_edge_property(dev, shape):
    """The slanted step 1 -> 3 between two colours of ``edge_scene`` (seed 3, default knobs).  Measured with the float64 restatement:
    guided error at most 3.6e-4, bilinear at least 1.5.  Bounds: guided at most 2e-3 = step * 10 * range_floor (about ten wrong-side
    taps at the floor against one right-side tap); bilinear at least 0.5."""
    kw, truth = RS.edge_scene(*shape)
    out, valid = _gpu(kw)
    out, v = out.cpu().numpy()[0, 0, 0].astype(np.float64), valid.cpu().numpy()[0, 0, 0].astype(bool)
    _, in_x, _ = RS.coords(shape[0][1], shape[1][1], shape[2][1], shape[3][1])
    assert np.array_equal(v, np.broadcast_to(in_x[None, :], v.shape)) and (out[~v] == 0).all()
    guided = float(np.abs(out - truth)[v].max())
    rows, cols = np.flatnonzero(v.any(axis=1)), np.flatnonzero(v.any(axis=0))
    up = torch.nn.functional.interpolate(torch.from_numpy(kw["src"][0, :, 0]).cuda()[None], size=(len(rows), len(cols)), mode="bilinear",
                                         align_corners=False)[0, 0].cpu().numpy()
    bilinear = float(np.abs(up - truth[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]).max())
    print(f"{shape}: guided {guided:.3e} (bound {RS.EDGE_GUIDED_BOUND}), bilinear {bilinear:.3f} (at least {RS.EDGE_BILINEAR_BOUND})")
    assert guided <= RS.EDGE_GUIDED_BOUND
    assert bilinear >= RS.EDGE_BILINEAR_BOUND


def _raw_args(kw, out_t, valid_t, frame_index="table", **over):
    """The ABI call's argument list on a case's arrays; ``over`` replaces arguments by name.  Returns (args, keep-alive list)."""
    B, Tg, H, W, _ = kw["guide_hi"].shape
    _, Cn, T, h, w = kw["src"].shape
    dev_t = [torch.from_numpy(kw[k]).cuda() for k in ("guide_hi", "guide_lo", "src")]
    fidx = torch.tensor(list(kw["frame_index"] if kw["frame_index"] is not None else range(T)), dtype=torch.int32).cuda()
    f3 = C.c_float * 3
    a = dict(guide_hi=_p(dev_t[0]), frame_index=_p(fidx) if frame_index == "table" else None, guide_lo=_p(dev_t[1]), mean3=f3(*RS.MEAN),
             std3=f3(*RS.STD), src=_p(dev_t[2]), scale=None, B=B, C=Cn, T=T, Tg=Tg, H=H, W=W, res_h=kw["res_hw"][0], res_w=kw["res_hw"][1],
             crop_i0=kw["crop_ij"][0], crop_j0=kw["crop_ij"][1], h=h, w=w, radius=kw["radius"], sigma_s=1.0, sigma_r=0.1,
             range_floor=1e-4, out=_p(out_t), valid=_p(valid_t))
    a.update(over)
    return [_stream()] + list(a.values()), dev_t + [fidx]


def test_two_calls_give_the_same_bits(dev):
    for name in ("b", "e"):
        kw, _ = _case(name)
        a, av = _gpu(kw)
        b, bv = _gpu(kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(av, bv)
    # a NULL frame_index is the identity table
    out, valid = torch.full_like(a, 7.0), torch.full_like(av, 7)
    args, keep = _raw_args(kw, out, valid, frame_index=None)
    assert _lib.load().l4p_guided_upsample(*args) == 0
    assert torch.equal(out.view(torch.int32), a.view(torch.int32)) and torch.equal(valid, av)


def test_refused_arguments_leave_the_output_alone(dev):
    kw, _ = _case("c")  # res 14 x 25 of 30 x 53, crop (0, 5) to 14 x 14, T = Tg = 2
    B, Cn, T, h, w = kw["src"].shape
    H, W = kw["guide_hi"].shape[2:4]
    out = torch.full((B, Cn, T, H, W), 7.0, device="cuda")
    valid = torch.full((B, 1, T, H, W), 7, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    args, keep = _raw_args(kw, out, valid)
    assert lib.l4p_guided_upsample(*args) == 0 and not (out == 7.0).all()
    out.fill_(7.0), valid.fill_(7)
    nan = float("nan")
    refused = [dict(B=0), dict(C=0), dict(T=0), dict(Tg=0), dict(H=0), dict(W=0), dict(res_h=0), dict(res_w=0), dict(h=0), dict(w=0),
               dict(C=9), dict(radius=0), dict(radius=4), dict(sigma_s=0.0), dict(sigma_s=-1.0), dict(sigma_s=nan), dict(sigma_r=0.0),
               dict(sigma_r=-0.1), dict(range_floor=0.0), dict(range_floor=-1e-4), dict(range_floor=1.5), dict(range_floor=nan),
               dict(res_h=H + 1), dict(res_w=W + 1), dict(crop_i0=1), dict(crop_j0=12), dict(crop_i0=-1, h=13), dict(crop_j0=-1),
               dict(frame_index=None, Tg=3), dict(guide_hi=None), dict(guide_lo=None), dict(mean3=None), dict(std3=None), dict(src=None),
               dict(out=None), dict(valid=None)]
    for over in refused:
        args, keep = _raw_args(kw, out, valid, **over)
        assert lib.l4p_guided_upsample(*args) == _lib.L4P_E_INVALID, over
        assert b"l4p_guided_upsample" in lib.l4p_last_error(), over
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (valid == 7).all()
    with pytest.raises(_lib.L4PHipError):
        NR.guided_upsample(torch.from_numpy(kw["guide_hi"]).cuda(), torch.from_numpy(kw["guide_lo"]).cuda(),
                           torch.from_numpy(kw["src"]).cuda(), _geometry(kw), radius=4)


def test_native_outputs_of_a_video_dataset_sample(dev):
    """(The source must not be smaller than the network's 224 x 224 grid - the entry refuses res > source - so the frames are 240 x
    428, the aspect of the demo's video.)"""
    Hs, Ws = 240, 428
    frames = synthetic_video(1, 20, Hs, Ws)
    ds = VideoDataset(video_paths=["videos/clip.mp4"], crop_size=(16, 224, 224), track_2d_querry_sampling_spacing=0.25,
                      frames={"videos/clip.mp4": frames}, device=dev)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)))
    src_frames, geometry = ds.source_clip(0)
    assert src_frames.dtype == torch.uint8 and tuple(src_frames.shape) == (20, Hs, Ws, 3) and src_frames.is_cuda
    assert geometry == NR.ClipGeometry((Hs, Ws), (224, 224), (0, 0), (224, 224), tuple(range(16)))
    g = torch.Generator().manual_seed(5)
    N = batch["track_2d_pointquerries_bn3"].shape[1]
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    out = {"depth_est_b1thw": rnd(1, 1, 16, 224, 224).abs() + 0.5, "flow_2d_backward_est_b2thw": rnd(1, 2, 16, 224, 224),
           "dyn_mask_est_b1thw": rnd(1, 1, 16, 224, 224), "track_2d_traj_est_bn2t": torch.rand(1, N, 2, 16, generator=g).cuda() * 224,
           "track_2d_vis_est_bn1t": rnd(1, N, 1, 16), "traj3d_intrinsics_est_b16t": batch["intrinsics_b44t"].reshape(1, 16, 16).clone(),
           "traj3d_est_b16t": rnd(1, 16, 16)}
    tasks = ["depth", "flow_2d_backward", "dyn_mask", "track_2d", "camray"]
    res = NR.native_resolution_outputs(batch, out, tasks, src_frames, geometry)
    packed, valid = NR.guided_upsample(src_frames, batch["rgb_b3thw"],
                                       torch.cat([out["depth_est_b1thw"], out["flow_2d_backward_est_b2thw"], out["dyn_mask_est_b1thw"]], 1),
                                       geometry)
    assert valid.all() and torch.equal(res["native_valid_b1thw"], valid)
    assert torch.equal(res["depth_est_b1thw"], packed[:, 0:1]) and torch.equal(res["dyn_mask_est_b1thw"], packed[:, 3:4])
    fx, fy = torch.tensor(Ws / 224, dtype=torch.float32).cuda(), torch.tensor(Hs / 224, dtype=torch.float32).cuda()
    assert torch.equal(res["flow_2d_backward_est_b2thw"][:, 0], packed[:, 1] * fx)
    assert torch.equal(res["flow_2d_backward_est_b2thw"][:, 1], packed[:, 2] * fy)
    assert res["flow_2d_backward_est_b2thw"].shape == (1, 2, 16, Hs, Ws)
    assert res["depth_est_b1thw"].untyped_storage().data_ptr() == res["dyn_mask_est_b1thw"].untyped_storage().data_ptr()  # views
    assert res["traj3d_est_b16t"] is out["traj3d_est_b16t"] and res["track_2d_vis_est_bn1t"] is out["track_2d_vis_est_bn1t"]
    # the dataset's intrinsics, mapped back, are the dummy source intrinsics: clip_geometry is what prepare_clip did
    K = res["traj3d_intrinsics_est_b16t"].reshape(4, 4, 16).cpu()
    want = torch.tensor([[min(Hs, Ws), 0, Ws / 2, 0], [0, min(Hs, Ws), Hs / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    assert (K - want[:, :, None]).abs().max() <= 1e-4
    assert torch.allclose(res["track_2d_traj_est_bn2t"][:, :, 0], out["track_2d_traj_est_bn2t"][:, :, 0] * (Ws / 224), atol=1e-3)
    nb = NR.native_batch(batch, src_frames, geometry)
    rgb01 = nb["rgb_b3thw"] * nb["rgb_std_b3111"] + nb["rgb_mean_b3111"]
    ref01 = src_frames[list(geometry.frame_index)].permute(3, 0, 1, 2)[None].float() / 255
    assert (rgb01 - ref01).abs().max() <= 1e-6
    assert (nb["intrinsics_b44t"][0].cpu() - want[:, :, None]).abs().max() <= 1e-4
    q, q0 = nb["track_2d_pointquerries_bn3"], batch["track_2d_pointquerries_bn3"]
    assert torch.equal(q[..., 0], q0[..., 0]) and torch.allclose(q[..., 1], q0[..., 1] * (Ws / 224)) and \
        torch.allclose(q[..., 2], q0[..., 2] * (Hs / 224))
    video = vis2d.render_video_panels(nb, res, tasks)["video"]
    assert tuple(video.shape) == (16, Hs, 5 * Ws, 3) and bool(torch.isfinite(video).all())
    # a source smaller than the network's grid has nothing to up-sample
    small = NR.ClipGeometry((60, 107), (224, 224), (0, 0), (224, 224), tuple(range(16)))
    with pytest.raises(ValueError):
        NR.native_resolution_outputs(batch, out, tasks, torch.zeros(20, 60, 107, 3, dtype=torch.uint8, device=dev), small)


def test_demo_native(dev, tmp_path):
    """The one whole-model run: demo.py --synthetic --frames 16 --native DIR --vis DIR on a 50-frame seeded video (240 x 428: not
    smaller than the network's grid)."""
    spec = importlib.util.spec_from_file_location("demo_native_run", os.path.join(ROOT, "demo", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    d = str(tmp_path / "native")
    demo.main(["--synthetic", "--frames", "16", "--synthetic-size", "240", "428", "--native", d, "--vis", d])
    z = np.load(os.path.join(d, "480p.mp4_native.npz"))
    want = {"depth_est_b1thw": ((1, 1, 16, 240, 428), np.float16), "flow_2d_backward_est_b2thw": ((1, 2, 16, 240, 428), np.float16),
            "dyn_mask_est_b1thw": ((1, 1, 16, 240, 428), np.float16), "native_valid_b1thw": ((1, 1, 16, 240, 428), np.uint8)}
    for k, (shape, dt) in want.items():
        assert z[k].shape == shape and z[k].dtype == dt, k
    assert set(z.files) == set(want) | {"track_2d_traj_est_bn2t"} and z["track_2d_traj_est_bn2t"].shape[2:] == (2, 16)
    assert z["native_valid_b1thw"].all() and np.isfinite(z["depth_est_b1thw"].astype(np.float32)).all()
    name = os.path.join(d, "480p.mp4_native")
    try:
        import mediapy  # noqa: F401
    except ImportError:
        frames = vis2d.read_png_frames(name)
        assert frames.shape == (16, 240, 5 * 428, 3)
    else:
        assert os.path.exists(name + ".mp4")
