"""`L4PDataset` / `L4PData` — the reference's dataset base class (l4p/data/l4p_dataset_mini.py:16-587) with the per-element
work on the GPU.

A dataset subclasses `L4PDataset` and writes one `getitem_helper(index) -> L4PData`, exactly as for the reference; `ds[i]` is
the reference's sample dict (keys, shapes, dtypes, values) as device tensors.  What runs where:
  * the dense fields (rgb, depth, flows, masks and their valid masks) — mirror padding with the forward / backward flow swap,
    nearest or trilinear resize, flow rescaling, crop, rgb normalisation — are ONE launch of libl4p_hip.so
    (csrc/gt_prep.hip: l4p_gt_dense_clip);
  * the query bounds filter of the crop is one launch (l4p_gt_query_select) whose 4-byte count is the only thing the host
    reads back per sample; the track tensors (gather, rescaling, shift, visibility clearing, query shift, the causal valid
    fix) are one more (l4p_gt_tracks_clip);
  * the control values — the frame table, the index tables, the crop offsets (drawn from torch's global CPU generator in
    the reference's order, so the same torch.manual_seed gives the same crop), dummy queries — and the tiny camera tensors
    (intrinsics, extrinsics, relative poses) are computed with torch in the reference's formulas and order.

The caller's tensors are never written.  Additions to the reference's constructor: ``device`` and
``scale_queries_on_resize`` (user queries together with a resize raise NotImplementedError in the reference, :286-288; with
the flag the query x / y are scaled like the trajectories and the labels pass through).  The reference's
`generate_point_qurries` (:397-416) is dead code there (never called) and is left out.

The product path never imports oracle/ and raises L4PHipError when the HIP library is missing.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from math import ceil
from typing import Any, Dict, List, Literal, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib
from ..ops import _p, _stream
from .video_dataset import _index_table, grid_queries, select_queries_over_seg


@dataclass(eq=False)
class L4PData:
    """Video depth, flow, tracks, ... of one clip; the attribute names show the sizes (the batch dimension comes from the
    dataloader).  Same fields and defaults as the reference's record (:16-44)."""

    rgb_b3thw: torch.Tensor  # rgb in [0,1], fp32
    intrinsics_b44t: Optional[torch.Tensor] = None
    extrinsics_b44t: Optional[torch.Tensor] = None
    rel_pose_b6t: Optional[torch.Tensor] = None  # w_T_c relative to the first frame, xyz + rotvec
    flow_2d_backward_b2thw: Optional[torch.Tensor] = None  # pixels, fp32
    flow_2d_backward_valid_b2thw: Optional[torch.Tensor] = None  # fp32 {0,1}
    flow_2d_forward_b2thw: Optional[torch.Tensor] = None
    flow_2d_forward_valid_b2thw: Optional[torch.Tensor] = None
    depth_b1thw: Optional[torch.Tensor] = None
    depth_valid_b1thw: Optional[torch.Tensor] = None
    instanceseg_b1thw: Optional[torch.Tensor] = None
    dyn_mask_b1thw: Optional[torch.Tensor] = None
    dyn_mask_valid_b1thw: Optional[torch.Tensor] = None
    track_2d_traj_bn2t: Optional[torch.Tensor] = None  # xy pixels, fp32
    track_2d_depth_bn1t: Optional[torch.Tensor] = None
    track_2d_vis_bn1t: Optional[torch.Tensor] = None  # bool
    track_2d_valid_bn1t: Optional[torch.Tensor] = None  # bool
    track_2d_pointquerries_bn3: Optional[torch.Tensor] = None
    track_2d_pointlabels_bn: Optional[torch.Tensor] = None
    dataset_name: Optional["str"] = None
    seq_name: Optional["str"] = None


ESTIMATION_DIRECTIONS = Literal[1, -1]

DENSE_KEYS = ("rgb_b3thw", "depth_b1thw", "depth_valid_b1thw", "instanceseg_b1thw", "dyn_mask_b1thw", "dyn_mask_valid_b1thw",
              "flow_2d_backward_b2thw", "flow_2d_forward_b2thw", "flow_2d_backward_valid_b2thw", "flow_2d_forward_valid_b2thw")
FLOW_KEYS = ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw", "flow_2d_backward_valid_b2thw", "flow_2d_forward_valid_b2thw")
_OPPOSITE = {"flow_2d_backward_b2thw": "flow_2d_forward_b2thw", "flow_2d_forward_b2thw": "flow_2d_backward_b2thw",
             "flow_2d_backward_valid_b2thw": "flow_2d_forward_valid_b2thw", "flow_2d_forward_valid_b2thw": "flow_2d_backward_valid_b2thw"}
TRACK_KEYS = ("track_2d_traj_bn2t", "track_2d_depth_bn1t", "track_2d_vis_bn1t", "track_2d_valid_bn1t")
CAMERA_KEYS = ("intrinsics_b44t", "extrinsics_b44t", "rel_pose_b6t")


def frame_table(n_frames: int, t_target: int) -> List[Tuple[int, int]]:
    """(source frame, swap flag) of every frame after the reference's padding (:555-560): a single frame is repeated
    (repeat_single_frame), otherwise `x = cat([x, flip(x)[1:]])` while the clip is shorter than the target (mirror_and_pad).
    Swap flag 1: a flow field reads the OPPOSITE direction's source there — both new flow tensors are built from the old pair
    (:132-162), so the flag is the direction parity of the mirror rounds."""
    if n_frames == 1:
        return [(0, 0)] * t_target
    tab = [(f, 0) for f in range(n_frames)]
    while len(tab) < t_target:
        tab = tab + [(f, 1 - s) for f, s in tab[::-1][1:]]
    return tab


def draw_crop_offsets(diff: Tuple[int, int, int], center_crop: bool, start_crop_time: bool) -> Tuple[int, int, int]:
    """(t0, i0, j0) of crop (:311-319), drawn from torch's global CPU generator in the reference's order: t0 whenever the clip is
    longer than the crop (before start_crop_time overrides it), then i0, then j0, the latter two only for a random crop."""
    t0 = 0 if diff[0] <= 0 else int(torch.randint(0, diff[0], (1,))[0])
    if start_crop_time:
        t0 = 0
    if center_crop:
        i0 = 0 if diff[1] <= 0 else int(diff[1] * 0.5)
        j0 = 0 if diff[2] <= 0 else int(diff[2] * 0.5)
    else:
        i0 = 0 if diff[1] <= 0 else int(torch.randint(0, diff[1], (1,))[0])
        j0 = 0 if diff[2] <= 0 else int(torch.randint(0, diff[2], (1,))[0])
    return t0, i0, j0


_axis_tables: Dict[Tuple[int, int, int, int, str], Tuple[torch.Tensor, ...]] = {}


def _axis(in_size: int, res_size: int, crop0: int, out_size: int, device: torch.device) -> Tuple[torch.Tensor, ...]:
    """Device tables of one axis resized in_size -> res_size and cropped to [crop0, crop0 + out_size): (nearest, i0, i1, lambda) from
    the library's host rules (l4p_torch_nearest_table, l4p_resize_index_table); cached."""
    key = (in_size, res_size, crop0, out_size, str(device))
    hit = _axis_tables.get(key)
    if hit is None:
        near = np.ascontiguousarray(_index_table("l4p_torch_nearest_table", in_size, res_size)[crop0:crop0 + out_size])
        i0, i1, lam = np.empty(out_size, np.int32), np.empty(out_size, np.int32), np.empty(out_size, np.float32)
        _lib.check(_lib.load().l4p_resize_index_table(in_size, res_size, crop0, out_size, i0.ctypes.data, i1.ctypes.data, lam.ctypes.data),
                   "l4p_resize_index_table")
        if in_size == res_size:  # ATen "simply copies" an axis of unchanged size: both indices on the same element, weights (1, 0)
            i1, lam = i0.copy(), np.zeros(out_size, np.float32)
        hit = tuple(torch.from_numpy(a).to(device) for a in (near, i0, i1, lam))
        if len(_axis_tables) > 256:
            _axis_tables.clear()
        _axis_tables[key] = hit
    return hit


def gt_query_select(queries: torch.Tensor, t0: int, Tn: int, i0: int, Hn: int, j0: int, Wn: int, scale: Optional[Tuple[float, float]] = None
                    ) -> torch.Tensor:
    """Indices (int32, device, ascending) of the queries [N,3] strictly inside the crop (:356-365): one launch and ONE 4-byte copy
    to the host.  ``scale`` = (fw, fh): the queries' x / y are scaled first (scale_queries_on_resize)."""
    N = int(queries.shape[0])
    dev = queries.device
    if N == 0:
        return torch.empty(0, dtype=torch.int32, device=dev)
    sel = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    fw, fh = scale if scale is not None else (1.0, 1.0)
    _lib.check(_lib.load().l4p_gt_query_select(_stream(), _p(queries), N, t0, Tn, i0, Hn, j0, Wn, int(scale is not None), fw, fh, _p(sel),
                                               _p(count)), "l4p_gt_query_select")
    return sel[: int(count.item())]


def gt_tracks_clip(traj: torch.Tensor, vis: torch.Tensor, valid: torch.Tensor, depth: Optional[torch.Tensor], queries: torch.Tensor,
                   labels: torch.Tensor, sel: Optional[torch.Tensor], ftab: torch.Tensor, *, traj_scale: Optional[Tuple[float, float]] = None,
                   query_scale: Optional[Tuple[float, float]] = None, crop: Optional[Tuple[int, int, int, int, int]] = None,
                   causal: int = 0) -> Dict[str, torch.Tensor]:
    """The six track tensors of the kept rows (``sel`` None = all).  traj [N,2,T0] float, vis / valid [N,1,T0] uint8, depth [N,1,T0]
    float or None, queries [N,3], labels [N], ftab int32 [Tn,2] on the device; ``crop`` = (t0, i0, j0, Hn, Wn) or None for a
    no-op crop."""
    dev = traj.device
    N, _, T0 = traj.shape
    Tn = int(ftab.shape[0])
    M = N if sel is None else int(sel.shape[0])
    out = {
        "track_2d_traj_bn2t": torch.empty((M, 2, Tn), dtype=torch.float32, device=dev),
        "track_2d_vis_bn1t": torch.empty((M, 1, Tn), dtype=torch.uint8, device=dev),
        "track_2d_valid_bn1t": torch.empty((M, 1, Tn), dtype=torch.uint8, device=dev),
        "track_2d_pointquerries_bn3": torch.empty((M, 3), dtype=torch.float32, device=dev),
        "track_2d_pointlabels_bn": torch.empty((M,), dtype=torch.float32, device=dev),
    }
    if depth is not None:
        out["track_2d_depth_bn1t"] = torch.empty((M, 1, Tn), dtype=torch.float32, device=dev)
    if M > 0:
        fw, fh = traj_scale or query_scale or (1.0, 1.0)
        t0, i0, j0, Hn, Wn = crop if crop is not None else (0, 0, 0, 1, 1)
        _lib.check(_lib.load().l4p_gt_tracks_clip(
            _stream(), _p(traj), _p(vis), _p(valid), _p(depth), _p(queries), _p(labels), N, T0, _p(sel), M, _p(ftab), Tn,
            int(traj_scale is not None), int(query_scale is not None), fw, fh, int(crop is not None), t0, i0, j0, Hn, Wn, causal,
            _p(out["track_2d_traj_bn2t"]), _p(out["track_2d_vis_bn1t"]), _p(out["track_2d_valid_bn1t"]),
            _p(out.get("track_2d_depth_bn1t")), _p(out["track_2d_pointquerries_bn3"]), _p(out["track_2d_pointlabels_bn"])),
            "l4p_gt_tracks_clip")
    out["track_2d_vis_bn1t"] = out["track_2d_vis_bn1t"].view(torch.bool)
    out["track_2d_valid_bn1t"] = out["track_2d_valid_bn1t"].view(torch.bool)
    return out


class L4PDataset(Dataset):
    """Drop-in for l4p.data.l4p_dataset_mini.L4PDataset (same arguments and defaults; `device` and `scale_queries_on_resize`
    are additions)."""

    default_sample_size = (16, 224, 224)

    def __init__(
        self,
        crop_size: Optional[Tuple[int, int, int]] = default_sample_size,
        track_2d_traj_per_sample: int = 128,
        track_2d_vis_thr: int = 4,
        track_2d_repeat_traj: bool = True,
        center_crop: bool = False,
        start_crop_time: bool = False,
        resize_size: Optional[Union[Tuple[int, int], int]] = None,
        resize_mode: Dict[str, str] = {"rgb_b3thw": "trilinear"},
        estimation_directions: List[ESTIMATION_DIRECTIONS] = [1, -1],
        traj_sampling_window: Optional[List[int]] = None,
        length_mutiply_of: int = 8,
        track_2d_querry_sampling_version: Optional[Literal["uniform", "uniform_over_seg"]] = None,
        track_2d_querry_sampling_spacing: float = 0.02,
        remove_queries_outside_bounds: bool = True,
        scaling_mode: Optional[Literal["avg_pointmapdist", "max_depth"]] = None,
        device: Union[str, torch.device] = "cuda",
        scale_queries_on_resize: bool = False,
    ) -> None:
        super().__init__()
        self.crop_size = crop_size
        self.track_2d_traj_per_sample = track_2d_traj_per_sample
        self.track_2d_vis_thr = track_2d_vis_thr
        self.track_2d_repeat_traj = track_2d_repeat_traj  # stored and unused, as in the reference
        self.center_crop = center_crop
        self.start_crop_time = start_crop_time
        if resize_size is not None:
            resize_size = (resize_size, resize_size) if not isinstance(resize_size, tuple) else resize_size
        self.resize_size = resize_size
        self.resize_mode = self.setup_resize_mode(resize_mode)
        self.estimation_directions = estimation_directions
        self.traj_sampling_window = traj_sampling_window
        self.length_multiply_of = length_mutiply_of
        self.track_2d_querry_sampling_version = track_2d_querry_sampling_version
        self.track_2d_querry_sampling_spacing = track_2d_querry_sampling_spacing
        self.remove_queries_outside_bounds = remove_queries_outside_bounds
        self.scaling_mode = scaling_mode  # stored and unused, as in the reference
        self.device = torch.device(device)
        self.scale_queries_on_resize = scale_queries_on_resize

        self.input_mean = torch.Tensor([0.485, 0.456, 0.406]).to(dtype=torch.float32)
        self.input_std = torch.Tensor([0.229, 0.224, 0.225]).to(dtype=torch.float32)

    def setup_resize_mode(self, resize_mode: Dict[str, str]) -> Dict[str, str]:
        out = {key: "nearest" for key in DENSE_KEYS}  # :107-118 (sparse depth, masks and flow are safer with nearest)
        out["rgb_b3thw"] = "trilinear"
        for key in resize_mode:
            out[key] = resize_mode[key]
        return out

    def getitem_helper(self, index: int) -> L4PData:
        raise NotImplementedError

    def get_dict_with_valid_vals(self, sample: L4PData) -> Tuple[Dict[str, Any], Dict[str, Any]]:
        """The non-None fields of the record: (tensors, strings).  Nothing is copied here: no later step writes to a tensor of the
        caller's (the reference's `asdict` deep-copies them for the same guarantee, :527)."""
        out, out_str = {}, {}
        for f in fields(sample):
            v = getattr(sample, f.name)
            if v is None:
                continue
            if isinstance(v, str):
                out_str[f.name] = v
            else:
                out[f.name] = v
        return out, out_str

    # -- host steps ----------------------------------------------------------------------------------------------------------

    def _cameras(self, sample: Dict[str, torch.Tensor], idx: List[int], single: bool, factor: Optional[Tuple[float, float]],
                 crop: Optional[Tuple[int, int, int, int, int]]) -> Dict[str, torch.Tensor]:
        """intrinsics / extrinsics / rel_pose through padding (:175-184, :214-231), resize (:281-285) and crop (:347, :386-388) with
        torch, out of place, in the reference's order."""
        out = {}
        intr = sample["intrinsics_b44t"]
        Tn = len(idx)
        for key in CAMERA_KEYS:
            if key not in sample:
                continue
            x = sample[key].to(torch.float32)
            if single and key == "extrinsics_b44t":
                x = torch.eye(4, dtype=intr.dtype, device=intr.device)[..., None].repeat(1, 1, Tn)
            elif single and key == "rel_pose_b6t":
                x = torch.zeros(6, Tn, dtype=intr.dtype, device=intr.device)
            else:
                x = x[..., torch.as_tensor(idx, device=x.device)]  # (a copy: the updates below never reach the caller's tensor)
            out[key] = x
        k = out["intrinsics_b44t"]
        if factor is not None:
            k[0, 0, :] = k[0, 0, :] * factor[1]
            k[1, 1, :] = k[1, 1, :] * factor[0]
            k[0, 2, :] = (k[0, 2, :] + 0.5) * factor[1] - 0.5
            k[1, 2, :] = (k[1, 2, :] + 0.5) * factor[0] - 0.5
        if crop is not None:
            k[0, 2, :] = k[0, 2, :] - crop[2]
            k[1, 2, :] = k[1, 2, :] - crop[1]
        return {key: v.to(self.device) for key, v in out.items()}

    def _dummy_tracks(self, dense: Dict[str, torch.Tensor], Tn: int, Hn: int, Wn: int) -> Dict[str, torch.Tensor]:
        """sample_tracks without user queries (:431-495): grid or random queries in the first frame and all-zero dummy tracks."""
        dev = self.device
        version = self.track_2d_querry_sampling_version
        if version is not None:
            q = grid_queries(self.track_2d_querry_sampling_spacing, Tn, Hn, Wn)
            if version == "uniform_over_seg":
                if "instanceseg_b1thw" not in dense:
                    raise ValueError('sampling version "uniform_over_seg" needs instanceseg_b1thw')
                if Hn < 224 or Wn < 224:  # :458-460 look the mask up at int(g * 224): out of range in the reference
                    raise ValueError(f"uniform_over_seg sampling indexes the mask on a 224 grid; the crop is {Hn}x{Wn}")
                q = q.to(dev)[select_queries_over_seg(dense["instanceseg_b1thw"][0, 0], self.track_2d_querry_sampling_spacing)]
            self.track_2d_traj_per_sample = q.shape[0]
        else:
            q = torch.rand((self.track_2d_traj_per_sample, 3)).to(dtype=torch.float32)
            q[..., 0] = 0
            for i, size in enumerate((Tn, Wn, Hn)):
                q[..., i] = torch.round(q[..., i] * (size - 1)) + 0.5
        n = self.track_2d_traj_per_sample
        f32 = dict(dtype=torch.float32, device=dev)
        return {
            "track_2d_traj_bn2t": torch.zeros((n, 2, Tn), **f32),
            "track_2d_vis_bn1t": torch.zeros((n, 1, Tn), dtype=torch.bool, device=dev),
            "track_2d_depth_bn1t": torch.ones((n, 1, Tn), **f32),
            "track_2d_valid_bn1t": torch.zeros((n, 1, Tn), dtype=torch.bool, device=dev),  # (the causal fix only clears bits)
            "track_2d_pointquerries_bn3": q.to(dev),
            "track_2d_pointlabels_bn": torch.ones((n,), **f32),
        }

    # -- the sample ----------------------------------------------------------------------------------------------------------

    def __getitem__(self, index):
        sample, sample_str = self.get_dict_with_valid_vals(self.getitem_helper(index))
        dev = self.device
        if dev.type != "cuda":
            raise _lib.L4PHipError("L4PDataset prepares its clips on the GPU (there is no CPU fallback): device must be a cuda device")
        for key in sample:
            if key not in DENSE_KEYS + TRACK_KEYS + CAMERA_KEYS + ("track_2d_pointquerries_bn3", "track_2d_pointlabels_bn"):
                raise NotImplementedError(f"key {key} not handled")
        _, T0, H, W = sample["rgb_b3thw"].shape
        if "intrinsics_b44t" not in sample:  # :537-539
            sample["intrinsics_b44t"] = torch.eye(4)[:, :, None].repeat(1, 1, T0)

        # -- temporal target and the frame table (:546-560) --
        ori_video_len = T0
        crop_size = self.crop_size
        if crop_size is None:
            m = self.length_multiply_of
            crop_size = (ceil(max(T0, self.default_sample_size[0]) / m) * m,) + tuple(self.default_sample_size[1:])
        Tc, Hn, Wn = (int(v) for v in crop_size)
        single = T0 == 1
        if single:
            for key in FLOW_KEYS:
                if key in sample:
                    raise NotImplementedError(f"{key}: a single frame cannot be extended to a clip with flow (repeat_single_frame)")
        elif T0 < Tc:
            for key in FLOW_KEYS:
                if key in sample and _OPPOSITE[key] not in sample:
                    raise ValueError(f"mirror padding {key} needs {_OPPOSITE[key]}, which the sample does not have")
            for key in ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw"):
                valid_key = key.replace("_b2thw", "_valid_b2thw")
                if key in sample and valid_key not in sample:
                    raise ValueError(f"mirror padding {key} needs {valid_key}, which the sample does not have")
        table = frame_table(T0, Tc)
        T_pad = len(table)

        # -- resize (:237-290) --
        have_queries = "track_2d_pointquerries_bn3" in sample
        res_h, res_w = (int(self.resize_size[0]), int(self.resize_size[1])) if self.resize_size is not None else (H, W)
        factor: Optional[Tuple[float, float]] = (res_h / H, res_w / W)
        if factor[0] == 1.0 and factor[1] == 1.0:
            factor = None
        if factor is not None and not self.scale_queries_on_resize:
            for key in ("track_2d_pointquerries_bn3", "track_2d_pointlabels_bn"):
                if key in sample:
                    raise NotImplementedError(f"key {key} not handled by resize: user queries with a resize factor != 1 (pass "
                                              "scale_queries_on_resize=True to scale them like the trajectories)")
        f32w, f32h = (float(np.float32(factor[1])), float(np.float32(factor[0]))) if factor is not None else (1.0, 1.0)

        # -- crop offsets (:299-319) --
        diff = (T_pad - Tc, res_h - Hn, res_w - Wn)
        assert diff[0] >= 0 and diff[1] >= 0 and diff[2] >= 0, f"Cropping Error: diff_shape {list(diff)}"
        cropped = not (diff[0] == 0 and diff[1] == 0 and diff[2] == 0)
        t0, i0, j0 = draw_crop_offsets(diff, self.center_crop, self.start_crop_time) if cropped else (0, 0, 0)
        table = table[t0:t0 + Tc]
        Tn = Tc
        crop = (t0, i0, j0, Hn, Wn) if cropped else None
        ftab = torch.tensor(table, dtype=torch.int32).to(dev)

        # -- dense fields: one launch --
        out: Dict[str, Any] = {}
        ynear, yi0, yi1, ylam = _axis(H, res_h, i0, Hn, dev)
        xnear, xi0, xi1, xlam = _axis(W, res_w, j0, Wn, dev)
        descs = (_lib.GtField * _lib.GT_MAX_FIELDS)()
        srcs = {key: sample[key].to(device=dev, dtype=torch.float32).contiguous() for key in DENSE_KEYS if key in sample}
        for n, (key, src) in enumerate(srcs.items()):
            if src.dim() != 4 or tuple(src.shape[1:]) != (T0, H, W) or src.shape[0] > 3:
                raise ValueError(f"{key} {tuple(src.shape)} does not match rgb_b3thw [3, {T0}, {H}, {W}]")
            if key in FLOW_KEYS and _OPPOSITE[key] in srcs and srcs[_OPPOSITE[key]].shape != src.shape:
                raise ValueError(f"{key} {tuple(src.shape)} and {_OPPOSITE[key]} {tuple(srcs[_OPPOSITE[key]].shape)} differ in shape")
            d = descs[n]
            out[key] = torch.empty((src.shape[0], Tn, Hn, Wn), dtype=torch.float32, device=dev)
            d.src, d.out, d.channels = _p(src), _p(out[key]), src.shape[0]
            d.src_swap = _p(srcs[_OPPOSITE[key]]) if key in FLOW_KEYS and _OPPOSITE[key] in srcs else None
            mode = self.resize_mode[key]
            if mode not in ("nearest", "trilinear"):
                raise NotImplementedError(f"resize mode {mode!r} for {key}: nearest and trilinear are implemented")
            d.mode = _lib.GT_BILINEAR if (mode == "trilinear" and factor is not None) else _lib.GT_NEAREST
            if key in ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw") and factor is not None:
                d.apply_scale = 1
                d.scale[0], d.scale[1] = f32w, f32h  # u with W, v with H (:268-269)
            if key == "rgb_b3thw":
                d.normalize = 1
                for c in range(3):
                    d.mean[c], d.stdv[c] = float(self.input_mean[c]), float(self.input_std[c])
        _lib.check(_lib.load().l4p_gt_dense_clip(_stream(), descs, len(srcs), T0, H, W, _p(ftab), _p(ynear), _p(xnear), _p(yi0), _p(yi1),
                                                 _p(ylam), _p(xi0), _p(xi1), _p(xlam), Tn, Hn, Wn), "l4p_gt_dense_clip")

        # -- cameras: host --
        out.update(self._cameras(sample, [f for f, _ in table], single, factor, crop))

        # -- tracks: filter (one 4-byte read-back) + one launch, or the dummy ground truth (:418-497) --
        if have_queries:
            seq = sample_str.get("seq_name")
            assert "track_2d_pointlabels_bn" in sample, "need to pass point labels for %s}" % seq
            assert "track_2d_valid_bn1t" in sample, "need to pass valid %s" % seq
            q = sample["track_2d_pointquerries_bn3"].to(device=dev, dtype=torch.float32).contiguous()
            labels = sample["track_2d_pointlabels_bn"].to(device=dev, dtype=torch.float32).contiguous()
            N = int(q.shape[0])
            traj = sample["track_2d_traj_bn2t"].to(device=dev, dtype=torch.float32).contiguous()
            vis = sample["track_2d_vis_bn1t"].to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
            valid = sample["track_2d_valid_bn1t"].to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
            depth = sample.get("track_2d_depth_bn1t")
            depth = depth.to(device=dev, dtype=torch.float32).contiguous() if depth is not None else None
            if tuple(traj.shape) != (N, 2, T0) or tuple(vis.shape) != (N, 1, T0) or tuple(valid.shape) != (N, 1, T0) or \
                    tuple(labels.shape) != (N,) or (depth is not None and tuple(depth.shape) != (N, 1, T0)) or q.shape[1] != 3:
                raise ValueError(f"track tensors do not match {N} queries over {T0} frames")
            scale = (f32w, f32h) if factor is not None else None
            sel = None
            if cropped and self.remove_queries_outside_bounds:
                sel = gt_query_select(q, t0, Tn, i0, Hn, j0, Wn, scale)
            causal = int(self.estimation_directions[0]) if len(self.estimation_directions) != 2 else 0
            out.update(gt_tracks_clip(traj, vis, valid, depth, q, labels, sel, ftab, traj_scale=scale, query_scale=scale, crop=crop,
                                      causal=1 if causal == 1 else (-1 if causal != 0 else 0)))
        else:
            out.update(self._dummy_tracks(out, Tn, Hn, Wn))

        # -- proper form (:576-587) --
        out["rgb_mean_b3111"] = self.input_mean[:, None, None, None].to(dev)
        out["rgb_std_b3111"] = self.input_std[:, None, None, None].to(dev)
        for key in out:
            out[key] = out[key].contiguous()
        out.update(sample_str)
        out["ori_video_len"] = ori_video_len
        return out
