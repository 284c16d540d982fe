"""Results at the video's own resolution (csrc/upsample.hip): the engine's dense outputs carried from the network's 224 x 224 grid to
the pixel grid of the decoded frames by joint bilateral up-sampling (Kopf et al. 2007).

The decoded uint8 frames are the full-resolution guide, the network's own input ``rgb_b3thw`` the matching low-resolution one: a
full-resolution pixel takes the low-resolution values of the taps round its position, weighted by distance and by how well the tap's
colour matches its own, so depth, flow and mask edges follow the edges of the picture where bilinear interpolation smears them over
about one low-resolution pixel.  The definition, operation by operation, is at ``l4p_guided_upsample`` in include/l4p_hip.h and in
DESIGN.md ("Native-resolution results").

``clip_geometry`` restates the bookkeeping of ``prepare_clip`` (which frames, which resize, which crop) on the host;
``VideoDataset.source_clip`` returns the frames it refers to.  Sparse outputs (tracks, queries, intrinsics) are mapped in closed form
by the inverse of the dataset's own rules.  Where ``native_valid_b1thw`` is 0 (pixels the centre crop cut away) the fields are 0.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from math import ceil
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..data.video_dataset import _MEAN, _STD, mirror_pad_indices
from ..ops import _p, _stream
from . import recon4d

MAX_CHANNELS = 8
# (task, output key, channels) of the dense fields, in packing order
DENSE_FIELDS = (("depth", "depth_est_b1thw", 1), ("flow_2d_backward", "flow_2d_backward_est_b2thw", 2),
                ("dyn_mask", "dyn_mask_est_b1thw", 1))


@dataclass(frozen=True)
class ClipGeometry:
    """How ``prepare_clip`` took a clip from the source frames: ``src_hw`` was resized to ``res_hw`` (half-pixel centres) and
    cropped at ``crop_ij`` to ``out_hw``; output frame t is source frame ``frame_index[t]`` (after the max_frames cut and the stride)."""
    src_hw: Tuple[int, int]
    res_hw: Tuple[int, int]
    crop_ij: Tuple[int, int]
    out_hw: Tuple[int, int]
    frame_index: Tuple[int, ...]

    def __post_init__(self):
        object.__setattr__(self, "frame_index", tuple(int(f) for f in self.frame_index))

    @property
    def factor_xy(self) -> Tuple[float, float]:
        """(res_w / W, res_h / H): the dataset's resize factors."""
        return self.res_hw[1] / self.src_hw[1], self.res_hw[0] / self.src_hw[0]


def clip_geometry(n_frames: int, H: int, W: int, crop_size: Optional[Sequence[int]], resize_size: Optional[Sequence[int]],
                  max_frames: Optional[int] = 192, stride: int = 1, default_sample_size: Sequence[int] = (16, 224, 224),
                  length_multiply_of: int = 8) -> ClipGeometry:
    """The geometry ``prepare_clip`` applies to ``n_frames`` decoded frames of H x W: the ``max_frames - 1`` cut, the stride, the
    default crop size (the clip length rounded up to a multiple of ``length_multiply_of``), mirror padding, the temporal crop, the
    resize size and the centre-crop offsets int(diff * 0.5).  Pure host code."""
    n = n_frames if max_frames is None else min(n_frames, max(max_frames - 1, 0))
    T0 = len(range(0, n, max(int(stride), 1)))
    if T0 < 1:
        raise ValueError(f"clip_geometry: no frame is left of {n_frames} (max_frames={max_frames}, stride={stride})")
    if crop_size is None:
        crop_size = (ceil(max(T0, default_sample_size[0]) / length_multiply_of) * length_multiply_of,) + tuple(default_sample_size[1:])
    Tn, Hn, Wn = (int(v) for v in crop_size)
    idx = mirror_pad_indices(T0, Tn)
    if len(idx) < Tn:
        raise ValueError(f"clip_geometry: cropping error, {len(idx)} frames for a crop of {Tn}")
    res_h, res_w = (int(resize_size[0]), int(resize_size[1])) if resize_size is not None else (H, W)
    diff = (res_h - Hn, res_w - Wn)
    if diff[0] < 0 or diff[1] < 0:
        raise ValueError(f"clip_geometry: cropping error, the crop {Hn}x{Wn} exceeds the resized frame {res_h}x{res_w}")
    return ClipGeometry((int(H), int(W)), (res_h, res_w), (int(diff[0] * 0.5), int(diff[1] * 0.5)), (Hn, Wn), tuple(idx[:Tn]))


def map_points(xy: torch.Tensor, geometry: ClipGeometry, dim: int = -2) -> torch.Tensor:
    """Continuous pixel coordinates (pixel centres at .5; x then y along ``dim``) of the network's grid in the source frame's: the
    inverse of the dataset's rule x * f - j0, X = (x + crop_j0) * W / res_w and Y likewise."""
    (i0, j0), (H, W), (rh, rw) = geometry.crop_ij, geometry.src_hw, geometry.res_hw
    shape = [1] * xy.dim()
    shape[dim] = 2
    off = torch.tensor([float(j0), float(i0)], dtype=xy.dtype, device=xy.device).reshape(shape)
    mul = torch.tensor([W / rw, H / rh], dtype=xy.dtype, device=xy.device).reshape(shape)
    return (xy + off) * mul


def map_queries(q_bn3: torch.Tensor, geometry: ClipGeometry) -> torch.Tensor:
    """Point queries (t, x, y): x and y through ``map_points``, t unchanged."""
    return torch.cat([q_bn3[..., :1], map_points(q_bn3[..., 1:], geometry, dim=-1)], dim=-1)


def map_intrinsics(k_b44t: torch.Tensor, geometry: ClipGeometry) -> torch.Tensor:
    """Pixel intrinsics [..., 4, 4, T] of the network's grid in the source frame's: the inverse of the crop shift (c - crop) and of
    the resize (f * factor, (c + 0.5) * factor - 0.5): fx / f, (cx + crop_j0 + 0.5) / f - 0.5, and fy, cy likewise."""
    fx, fy = geometry.factor_xy
    i0, j0 = geometry.crop_ij
    k = k_b44t.clone()
    k[..., 0, 0, :] = k_b44t[..., 0, 0, :] / fx
    k[..., 1, 1, :] = k_b44t[..., 1, 1, :] / fy
    k[..., 0, 2, :] = (k_b44t[..., 0, 2, :] + j0 + 0.5) / fx - 0.5
    k[..., 1, 2, :] = (k_b44t[..., 1, 2, :] + i0 + 0.5) / fy - 0.5
    return k


_frame_tables: Dict[Tuple[Tuple[int, ...], str], torch.Tensor] = {}


def _frame_table(geometry: ClipGeometry, device: torch.device) -> torch.Tensor:
    """``geometry.frame_index`` as int32 on the device, cached per table and device."""
    key = (geometry.frame_index, str(device))
    hit = _frame_tables.get(key)
    if hit is None:
        hit = _frame_tables[key] = torch.tensor(geometry.frame_index, dtype=torch.int32, device=device)
    return hit


def _check_shapes(frames_u8, guide_lo, src, geometry: ClipGeometry) -> tuple:
    if src.dim() != 5:
        raise ValueError(f"guided_upsample: src_bcthw has shape {tuple(src.shape)}, expected [B, C, T, h, w]")
    B, Cn, T, h, w = src.shape
    if min(B, Cn, T, h, w) < 1 or Cn > MAX_CHANNELS:
        raise ValueError(f"guided_upsample: src_bcthw {tuple(src.shape)} needs 1 <= C <= {MAX_CHANNELS} and no empty dimension")
    if tuple(guide_lo.shape) != (B, 3, T, h, w):
        raise ValueError(f"guided_upsample: guide_lo_b3thw has shape {tuple(guide_lo.shape)}, src_bcthw {tuple(src.shape)} needs "
                         f"{(B, 3, T, h, w)}")
    if (h, w) != tuple(geometry.out_hw) or T != len(geometry.frame_index):
        raise ValueError(f"guided_upsample: src_bcthw {tuple(src.shape)} does not match the geometry (out_hw {geometry.out_hw}, "
                         f"{len(geometry.frame_index)} frames)")
    H, W = geometry.src_hw
    if geometry.res_hw[0] > H or geometry.res_hw[1] > W:
        raise ValueError(f"guided_upsample: the source frames ({H} x {W}) are smaller than the resized frame {geometry.res_hw}: the "
                         "network's grid is the finer one, there is nothing to up-sample")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5) or tuple(frames_u8.shape[-3:]) != (H, W, 3) or \
            frames_u8.shape[-4] < 1 or (frames_u8.dim() == 5 and frames_u8.shape[0] != B):
        raise ValueError(f"guided_upsample: frames_u8 is {frames_u8.dtype} {tuple(frames_u8.shape)}, expected uint8 [Tg, {H}, {W}, 3] "
                         f"or [{B}, Tg, {H}, {W}, 3]")
    return B, Cn, T, int(frames_u8.shape[-4]), H, W, h, w


def guided_upsample(frames_u8: torch.Tensor, guide_lo_b3thw: torch.Tensor, src_bcthw: torch.Tensor, geometry: ClipGeometry,
                    mean: Sequence[float] = _MEAN, std: Sequence[float] = _STD, scale: Optional[Sequence[float]] = None,
                    radius: int = 2, sigma_s: float = 1.0, sigma_r: float = 0.1,
                    range_floor: float = 1e-4) -> Tuple[torch.Tensor, torch.Tensor]:
    """``src_bcthw`` (f32 [B, C, T, h, w], C <= 8) at the resolution of ``frames_u8``: (out f32 [B, C, T, H, W], valid uint8
    [B, 1, T, H, W]), device tensors, one launch, no read-back and no synchronisation.

    ``frames_u8``: the decoded frames uint8 [Tg, H, W, 3] (shared by the batch) or [B, Tg, H, W, 3], as ``VideoDataset.source_clip``
    returns them; ``guide_lo_b3thw``: the network's input ``rgb_b3thw`` (normalised with ``mean`` / ``std``); ``geometry``: the
    ``ClipGeometry`` of the clip; ``scale``: C host factors, channel c of the result is multiplied by scale[c].  ``sigma_s`` is in
    low-resolution pixels, ``sigma_r`` in colour units of [0, 1]; ``range_floor`` is the least range weight (a pixel whose colour
    matches no tap degrades to the spatial Gaussian).  valid is 0, and out 0, where the pixel lies outside the crop, its frame
    index is out of range or no tap of its window is finite."""
    B, Cn, T, Tg, H, W, h, w = _check_shapes(frames_u8, guide_lo_b3thw, src_bcthw, geometry)
    if len(mean) != 3 or len(std) != 3 or (scale is not None and len(scale) != Cn):
        raise ValueError(f"guided_upsample: mean and std hold 3 values and scale C = {Cn}")
    assert src_bcthw.is_cuda, "guided_upsample runs on the GPU"
    dev = src_bcthw.device
    src, guide_lo = recon4d._f32(src_bcthw, dev), recon4d._f32(guide_lo_b3thw, dev)
    frames = frames_u8.to(dev)
    if frames.dim() == 4:
        frames = frames[None].expand(B, Tg, H, W, 3)
    frames = frames.contiguous()
    out = torch.empty(B, Cn, T, H, W, dtype=torch.float32, device=dev)
    valid = torch.empty(B, 1, T, H, W, dtype=torch.uint8, device=dev)
    f3 = C.c_float * 3
    sc = (C.c_float * Cn)(*[float(v) for v in scale]) if scale is not None else None
    _lib.check(_lib.load().l4p_guided_upsample(
        _stream(), _p(frames), _p(_frame_table(geometry, dev)), _p(guide_lo), f3(*[float(v) for v in mean]), f3(*[float(v) for v in std]),
        _p(src), sc, B, Cn, T, Tg, H, W, geometry.res_hw[0], geometry.res_hw[1], geometry.crop_ij[0], geometry.crop_ij[1], h, w,
        int(radius), float(sigma_s), float(sigma_r), float(range_floor), _p(out), _p(valid)), "l4p_guided_upsample")
    return out, valid


def native_resolution_outputs(batch: dict, out: dict, tasks: List[str], frames_u8: torch.Tensor, geometry: ClipGeometry,
                              **knobs) -> Dict[str, object]:
    """The engine's outputs in the source frame's pixel grid, under the same keys.  The dense fields of the requested tasks
    (depth_est_b1thw; flow_2d_backward_est_b2thw, its x channel scaled by W / res_w and its y channel by H / res_h so that the
    vectors are in source pixels; dyn_mask_est_b1thw, logits) are packed into one tensor and up-sampled by ONE call of
    ``guided_upsample`` (``knobs``: its keyword arguments); the results are views of the packed output, and native_valid_b1thw is
    added.  track_2d_traj_est_bn2t goes through ``map_points``, traj3d_intrinsics_est_b16t through ``map_intrinsics``; poses,
    visibility logits and everything else pass through."""
    H, W = geometry.src_hw
    parts, scales, names = [], [], []
    for task, key, ch in DENSE_FIELDS:
        if task in tasks and key in out:
            if out[key].dim() != 5 or out[key].shape[1] != ch:
                raise ValueError(f"native_resolution_outputs: {key} has shape {tuple(out[key].shape)}, expected [B, {ch}, T, h, w]")
            parts.append(out[key].float())
            names.append((key, ch))
            scales += [W / geometry.res_hw[1], H / geometry.res_hw[0]] if task == "flow_2d_backward" else [1.0] * ch
    res = dict(out)
    if parts:
        shapes = {tuple(p.shape[:1] + p.shape[2:]) for p in parts}
        if len(shapes) != 1:
            raise ValueError(f"native_resolution_outputs: the dense outputs disagree in shape: {sorted(shapes)}")
        packed, valid = guided_upsample(frames_u8, batch["rgb_b3thw"], torch.cat(parts, dim=1), geometry, scale=scales, **knobs)
        c0 = 0
        for key, ch in names:
            res[key] = packed[:, c0:c0 + ch]
            c0 += ch
        res["native_valid_b1thw"] = valid
    if "track_2d" in tasks and "track_2d_traj_est_bn2t" in out:
        res["track_2d_traj_est_bn2t"] = map_points(out["track_2d_traj_est_bn2t"].float(), geometry, dim=-2)
    if "camray" in tasks and "traj3d_intrinsics_est_b16t" in out:
        k = out["traj3d_intrinsics_est_b16t"].float()
        res["traj3d_intrinsics_est_b16t"] = map_intrinsics(k.reshape(k.shape[0], 4, 4, -1), geometry).reshape(k.shape)
    return res


def native_batch(batch: dict, frames_u8: torch.Tensor, geometry: ClipGeometry) -> Dict[str, object]:
    """The batch the post-processors (``vis2d.render_video_panels``, ``scene_flow_from_outputs``, ``reconstruct_4d``) need at the
    source resolution: rgb_b3thw normalised from the source frames through ``frame_index`` (rgb_mean_b3111 / rgb_std_b3111 as the
    batch has them), the queries and track_2d_traj_bn2t through ``map_points``, intrinsics_b44t through ``map_intrinsics``;
    every other entry is passed on."""
    rgb = batch["rgb_b3thw"]
    dev, B = rgb.device, rgb.shape[0]
    H, W = geometry.src_hw
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5) or tuple(frames_u8.shape[-3:]) != (H, W, 3):
        raise ValueError(f"native_batch: frames_u8 is {frames_u8.dtype} {tuple(frames_u8.shape)}, expected uint8 [Tg, {H}, {W}, 3] or "
                         f"[B, Tg, {H}, {W}, 3]")
    if rgb.shape[2] != len(geometry.frame_index) or not all(0 <= f < frames_u8.shape[-4] for f in geometry.frame_index):
        raise ValueError(f"native_batch: rgb_b3thw {tuple(rgb.shape)} / {frames_u8.shape[-4]} source frames do not match the geometry")
    frames = frames_u8.to(dev)
    frames = frames[None] if frames.dim() == 4 else frames
    sel = frames.index_select(1, _frame_table(geometry, dev).long())                    # [B or 1, T, H, W, 3]
    mean = batch["rgb_mean_b3111"].to(dev).float().reshape(-1, 3, 1, 1, 1)
    std = batch["rgb_std_b3111"].to(dev).float().reshape(-1, 3, 1, 1, 1)
    nb = dict(batch)
    nb["rgb_b3thw"] = ((sel.permute(0, 4, 1, 2, 3).float() / 255.0 - mean) / std).expand(B, 3, -1, H, W).contiguous()
    if "track_2d_pointquerries_bn3" in batch:
        nb["track_2d_pointquerries_bn3"] = map_queries(batch["track_2d_pointquerries_bn3"], geometry)
    if "track_2d_traj_bn2t" in batch:
        nb["track_2d_traj_bn2t"] = map_points(batch["track_2d_traj_bn2t"], geometry, dim=-2)
    if "intrinsics_b44t" in batch:
        nb["intrinsics_b44t"] = map_intrinsics(batch["intrinsics_b44t"], geometry)
    return nb
