"""CPU: the host side of results at the video's own resolution (l4p_amd/utils/native_res.py) and the numpy restatement of the
up-sampler (tests/native_res_restate.py) on its own."""
import numpy as np
import pytest
import torch

from l4p_amd import _lib
from l4p_amd.utils import native_res as NR
from tests import native_res_restate as RS


def test_clip_geometry_max_frames_cut():
    g = NR.clip_geometry(300, 480, 854, None, (224, 224))  # 191 frames are read, the clip is padded to 192
    assert len(g.frame_index) == 192 and g.frame_index[:191] == tuple(range(191)) and g.frame_index[191] == 189
    assert g.src_hw == (480, 854) and g.res_hw == (224, 224) and g.crop_ij == (0, 0) and g.out_hw == (224, 224)


def test_clip_geometry_stride():
    g = NR.clip_geometry(50, 120, 214, (16, 224, 224), (224, 224), stride=2)  # 25 frames after the stride, the first 16 kept
    assert g.frame_index == tuple(range(16))
    g = NR.clip_geometry(21, 120, 214, (16, 224, 224), (224, 224), stride=2)  # 11 frames, mirrored
    assert g.frame_index == (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 9, 8, 7, 6, 5)


def test_clip_geometry_mirror_padding():
    g = NR.clip_geometry(5, 60, 107, (16, 224, 224), (224, 224))
    assert g.frame_index == (0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1)
    assert NR.clip_geometry(1, 60, 107, (8, 224, 224), (224, 224)).frame_index == (0,) * 8


def test_clip_geometry_default_crop_rounds_up():
    g = NR.clip_geometry(20, 60, 107, None, (224, 224))
    assert len(g.frame_index) == 24 and g.frame_index[:20] == tuple(range(20)) and g.frame_index[20:] == (18, 17, 16, 15)
    assert len(NR.clip_geometry(3, 60, 107, None, (224, 224)).frame_index) == 16  # default_sample_size[0]
    assert g.out_hw == (224, 224)


def test_clip_geometry_centre_crop_offsets():
    g = NR.clip_geometry(24, 181, 135, (16, 224, 224), (298, 224), stride=2)
    assert g.res_hw == (298, 224) and g.crop_ij == (37, 0) and g.out_hw == (224, 224) and g.src_hw == (181, 135)
    assert NR.clip_geometry(16, 100, 100, (16, 224, 224), (229, 227)).crop_ij == (2, 1)  # int(diff * 0.5)
    assert NR.clip_geometry(16, 100, 120, (16, 50, 60), None).res_hw == (100, 120)       # no resize
    with pytest.raises(ValueError):
        NR.clip_geometry(16, 100, 100, (16, 224, 224), (200, 224))


GEOM = NR.ClipGeometry((181, 135), (298, 224), (37, 3), (224, 218), tuple(range(4)))


def test_track_map_inverts_the_dataset_rule():
    g = torch.Generator().manual_seed(0)
    XY = torch.rand(2, 7, 2, 4, generator=g, dtype=torch.float64) * torch.tensor([135.0, 181.0], dtype=torch.float64)[None, None, :, None]
    fx, fy = 224 / 135, 298 / 181
    lo = torch.stack([XY[:, :, 0] * fx - 3, XY[:, :, 1] * fy - 37], dim=2)  # the dataset's x * f - j0
    assert (NR.map_points(lo, GEOM, dim=-2) - XY).abs().max() <= 1e-4
    q = torch.cat([torch.full((2, 7, 1), 2.5, dtype=torch.float64), lo[..., 0]], dim=-1)
    back = NR.map_queries(q, GEOM)
    assert (back[..., 0] == 2.5).all() and (back[..., 1:] - XY[..., 0]).abs().max() <= 1e-4


def test_intrinsics_map_inverts_the_dataset_rule():
    fx, fy = 224 / 135, 298 / 181
    K = torch.eye(4, dtype=torch.float64)[:, :, None].repeat(1, 1, 4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 403.2, 398.1, 66.9, 91.3
    lo = K.clone()  # prepare_clip: the resize, then the crop shift
    lo[0, 0], lo[1, 1] = K[0, 0] * fx, K[1, 1] * fy
    lo[0, 2], lo[1, 2] = (K[0, 2] + 0.5) * fx - 0.5 - 3, (K[1, 2] + 0.5) * fy - 0.5 - 37
    assert (NR.map_intrinsics(lo[None], GEOM)[0] - K).abs().max() <= 1e-4


@pytest.mark.parametrize("shape", RS.EDGE_SHAPES)
def test_restatement_edge_property(shape):
    kw, truth = RS.edge_scene(*shape)
    out, valid = RS.restate(**kw)
    v = valid[0, 0, 0].astype(bool)
    _, in_x, _ = RS.coords(shape[0][1], shape[1][1], shape[2][1], shape[3][1])
    _, in_y, _ = RS.coords(shape[0][0], shape[1][0], shape[2][0], shape[3][0])
    assert np.array_equal(v, in_y[:, None] & in_x[None, :]) and (out[0, 0, 0][~v] == 0).all()
    guided = float(np.abs(out[0, 0, 0] - truth)[v].max())
    up, ys, xs = RS.bilinear_reference(kw["src"][0, 0, 0], v)
    bilinear = float(np.abs(up - truth[ys, xs]).max())
    print(f"{shape}: guided {guided:.3e} (bound {RS.EDGE_GUIDED_BOUND}), bilinear {bilinear:.3f} (at least {RS.EDGE_BILINEAR_BOUND})")
    assert guided <= RS.EDGE_GUIDED_BOUND and bilinear >= RS.EDGE_BILINEAR_BOUND


def test_restatement_keeps_a_constant_field():
    kw = RS.parity_case("c")
    kw["src"] = np.full_like(kw["src"], 2.5)
    kw["scale"] = None
    out, valid = RS.restate(**kw)
    v = np.broadcast_to(valid.astype(bool), out.shape)
    assert v.any() and not v.all()  # the crop
    assert np.abs(out[v] - 2.5).max() <= 1e-12 and (out[~v] == 0).all()


def test_header_declares_and_binds_the_entry():
    with open(_lib.HEADER_PATH) as fh:
        assert "int l4p_guided_upsample(l4p_stream stream, const unsigned char* guide_hi, const int* frame_index" in fh.read()
    res, args = _lib.SIGNATURES["l4p_guided_upsample"]
    assert len(args) == 26 and _lib.ABI_VERSION >= 24


def test_shape_errors_raise_value_error():
    g = NR.ClipGeometry((23, 40), (12, 20), (0, 0), (12, 20), (0, 1, 2))
    frames = torch.zeros(3, 23, 40, 3, dtype=torch.uint8)
    lo, src = torch.zeros(2, 3, 3, 12, 20), torch.zeros(2, 4, 3, 12, 20)
    bad = [
        (frames, lo, src[0]),                                    # not five-dimensional
        (frames, lo, torch.zeros(2, 9, 3, 12, 20)),              # C > 8
        (frames, lo[:, :2], src),                                # the guide has three channels
        (frames, lo[:1], src),                                   # batch sizes differ
        (frames, lo[..., :19], src[..., :19]),                   # not the geometry's out_hw
        (frames, lo[:, :, :2], src[:, :, :2]),                   # not the geometry's frame count
        (frames[:, :22], lo, src),                               # not the geometry's src_hw
        (frames.float(), lo, src),                               # not uint8
        (frames[None].expand(3, -1, -1, -1, -1), lo, src),       # a batched guide of another batch size
    ]
    for f, l, s in bad:
        with pytest.raises(ValueError):
            NR.guided_upsample(f, l, s, g)
    with pytest.raises(ValueError):
        NR.guided_upsample(frames, lo, src, g, scale=[1.0, 2.0])
    out = {"depth_est_b1thw": torch.zeros(2, 2, 3, 12, 20)}
    with pytest.raises(ValueError):
        NR.native_resolution_outputs({"rgb_b3thw": lo}, out, ["depth"], frames, g)
    with pytest.raises(ValueError):
        NR.native_batch({"rgb_b3thw": lo[:, :, :2]}, frames, g)
