"""TEST INFRASTRUCTURE ONLY — CPU restatement (numpy / torch) of the reference's DavisDataset and DycheckDataset on decoded
arrays, and the seeded cases of tests/golden/datasets.npz (tools/gen_golden_datasets.py).

What it restates, reference file:line:
  * DavisDataset.getitem_helper      l4p/data/davis.py:75-141            blur, masks, dummy intrinsics
  * DycheckDataset.getitem_helper    l4p/data/dycheck_dataset.py:67-109  file intrinsics, identity extrinsics
  * L4PDataset.__getitem__           l4p/data/l4p_dataset_mini.py:543-587 (RGB path: oracle.preprocess_oracle)
  * L4PDataset.resize / crop for instanceseg_b1thw, intrinsics_b44t, extrinsics_b44t   :236-288, :290-391
  * L4PDataset.sample_tracks "uniform_over_seg"   :450-465

The mask path is materialised stage by stage (Pillow round trip at full size, nearest resize, crop) with index rules written in
Python here — independent of the library's host tables, which tests/test_datasets_cpu.py pins against Pillow and torch themselves.

kornia.morphology.erosion is not installed and its source is not available: `erosion3` restates its definition for the default
border_type="geodesic" (out-of-image neighbours never lower the minimum), so on a {0,1} mask a pixel survives iff all of its
in-image 3x3 neighbours are 1.  Unpinned by construction; the fixture's provenance JSON says the same.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from l4p_amd.data.synthetic import synthetic_masks, synthetic_video
from oracle import preprocess_oracle as po

# name -> parameters.  Frames / masks are regenerated from the seeds (synthetic_video / synthetic_masks).
DAVIS_CASES = {
    # DAVIS-2017 palette annotation, 480x854 proportions at a quarter of the size, two labels
    "palette": dict(seed=21, T=10, H=120, W=214, mask="blob", mode="P", crop_size=(16, 224, 224), resize_size=(224, 224),
                    stride=1, spacing=0.04),
    # DAVIS-2016 style 0/255 grey annotation: the round trip really is bilinear; stride 2
    "grey": dict(seed=22, T=9, H=96, W=150, mask="blob", mode="L", crop_size=(8, 224, 224), resize_size=(224, 224), stride=2,
                 spacing=0.05),
    # no annotation files at all: all-zero mask, every query kept
    "no_annotation": dict(seed=23, T=4, H=64, W=96, mask=None, mode="P", crop_size=(8, 224, 224), resize_size=(224, 224),
                          stride=1, spacing=0.1),
    # a one-pixel line (the height is untouched by every resize, so it stays one pixel): the erosion empties it, every query kept
    "thin": dict(seed=24, T=3, H=224, W=300, mask="thin", mode="P", crop_size=(8, 224, 224), resize_size=(224, 224), stride=1,
                 spacing=0.1),
    # the mask touches the image border: the candidate at cell (0, 0) survives a geodesic erosion and would not survive zero padding
    "border": dict(seed=25, T=5, H=90, W=128, mask="border", mode="P", crop_size=(8, 224, 224), resize_size=(224, 224), stride=1,
                   spacing=0.05),
    # crop_size None -> ceil(max(T,16)/8)*8 frames; non-square resize + centre crop
    "crop_none": dict(seed=26, T=18, H=135, W=241, mask="blob", mode="P", crop_size=None, resize_size=(298, 224), stride=1,
                      spacing=0.04),
}
DYCHECK_CASES = {
    # the demo's setting (demo.py:214-258): (298, 224), stride 2; odd frame size, a non-trivial calibration line
    "dycheck": dict(seed=31, T=13, H=181, W=135, crop_size=(8, 224, 224), resize_size=(298, 224), stride=2, spacing=0.04,
                    calibration=(403.217, 398.06, 66.9, 91.325)),
}


def case_inputs(name: str):
    """(frames uint8 [T,H,W,3], masks uint8 [T,H,W] or None) of a case, before any stride."""
    c = DAVIS_CASES.get(name) or DYCHECK_CASES[name]
    frames = synthetic_video(c["seed"], c["T"], c["H"], c["W"])
    masks = synthetic_masks(c["seed"] + 100, c["T"], c["H"], c["W"], c["mask"]) if c.get("mask") else None
    return frames, masks


def annotation_arrays(masks: Optional[np.ndarray], mode: str) -> Optional[np.ndarray]:
    """What PIL decodes from the annotation files write_davis_tree writes for ``masks``."""
    if masks is None:
        return None
    if mode == "P":
        return masks
    a = ((masks > 0) * 255).astype(np.uint8)
    return a if mode == "L" else np.repeat(a[..., None], 3, axis=-1)


def pil_nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """Image.resize(NEAREST) along one axis (libImaging/Geometry.c ImagingScaleAffine): the source coordinate starts at half a
    step and is accumulated in double; truncation."""
    a0 = float(in_size) / out_size
    xo = a0 * 0.5
    idx = np.empty(out_size, dtype=np.int64)
    for x in range(out_size):
        idx[x] = int(xo)
        xo += a0
    return idx


def torch_nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """F.interpolate(mode="nearest") given `size` along one axis (ATen nearest_idx, float32 scale)."""
    if out_size == in_size:
        return np.arange(out_size, dtype=np.int64)
    if out_size == 2 * in_size:
        return np.arange(out_size, dtype=np.int64) >> 1
    scale = np.float32(in_size) / np.float32(out_size)
    v = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(v, in_size - 1)


def mask_round_trip(ann: np.ndarray, mode: str, resize_size: Tuple[int, int]) -> np.ndarray:
    """davis.py:98-104 for one decoded annotation frame: Image.resize(resize_size) and back, first channel -> uint8 [H,W]."""
    H, W = ann.shape[:2]
    pw, ph = int(resize_size[0]), int(resize_size[1])
    if mode in ("P", "1"):  # Image.resize turns the filter into NEAREST for these modes
        small = ann[pil_nearest_index(H, ph)][:, pil_nearest_index(W, pw)]
        return small[pil_nearest_index(ph, H)][:, pil_nearest_index(pw, W)]
    a = ann if ann.ndim == 3 else ann[..., None]
    return po.pil_resize_u8(po.pil_resize_u8(a, pw, ph), W, H)[..., 0]


def erosion3(mask_hw: np.ndarray) -> np.ndarray:
    """kornia.morphology.erosion(mask, ones(3,3)) with its default geodesic border (see the module docstring)."""
    h, w = mask_hw.shape
    p = np.full((h + 2, w + 2), np.inf, dtype=np.float32)
    p[1:-1, 1:-1] = mask_hw
    out = np.full((h, w), np.inf, dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            out = np.minimum(out, p[dy:dy + h, dx:dx + w])
    return out


def seg_cells(spacing: float) -> np.ndarray:
    """(x_id, y_id) per grid candidate exactly as the reference's loop computes them (l4p_dataset_mini.py:440-459)."""
    grid_x, grid_y = torch.meshgrid(torch.arange(0, 1, spacing), torch.arange(0, 1, spacing), indexing="xy")
    dummy = torch.cat([torch.zeros_like(grid_x)[..., None], grid_x[..., None], grid_y[..., None]], dim=-1).reshape(-1, 3)
    return np.array([[int(dummy[n, 1] * 224), int(dummy[n, 2] * 224)] for n in range(dummy.shape[0])], dtype=np.int32)


def select_over_seg(mask0_hw: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """valid_ids of :451-463 (all candidates when none is valid)."""
    er = erosion3(mask0_hw)
    keep = np.array([m for m in range(cells.shape[0]) if er[cells[m, 1], cells[m, 0]] > 0], dtype=np.int64)
    return keep if keep.size else np.arange(cells.shape[0], dtype=np.int64)


def _geometry(T0: int, H: int, W: int, crop_size, resize_size):
    if crop_size is None:
        crop_size = (int(math.ceil(max(T0, 16) / 8) * 8), 224, 224)
    rh, rw = (int(resize_size[0]), int(resize_size[1])) if resize_size is not None else (H, W)
    Tn, Hn, Wn = crop_size
    i0, j0 = int((rh - Hn) * 0.5), int((rw - Wn) * 0.5)
    return (Tn, Hn, Wn), rh, rw, i0, j0


def intrinsics_pipeline(K44: torch.Tensor, Tn: int, H: int, W: int, rh: int, rw: int, i0: int, j0: int) -> np.ndarray:
    """intrinsics_b44t through resize (:281-285) and crop (:386-388), torch float32 in the reference's order."""
    intr = K44[:, :, None].repeat(1, 1, Tn).clone()
    f = (rh / H, rw / W)
    if not (f[0] == 1.0 and f[1] == 1.0):
        intr[0, 0, :] = intr[0, 0, :] * f[1]
        intr[1, 1, :] = intr[1, 1, :] * f[0]
        intr[0, 2, :] = (intr[0, 2, :] + 0.5) * f[1] - 0.5
        intr[1, 2, :] = (intr[1, 2, :] + 0.5) * f[0] - 0.5
    intr[0, 2, :] = intr[0, 2, :] - j0
    intr[1, 2, :] = intr[1, 2, :] - i0
    return intr.numpy()


def davis_sample(frames: np.ndarray, anns: Optional[np.ndarray], mode: str, crop_size, resize_size, stride: int,
                 spacing: float, rgb: bool = True) -> Dict[str, np.ndarray]:
    """DavisDataset.__getitem__ on decoded frames [T,H,W,3] and annotation arrays ([T,H,W] / [T,H,W,3] or None)."""
    frames = frames[::stride]
    anns = anns[::stride] if anns is not None else None
    T0, H, W = frames.shape[:3]
    (Tn, Hn, Wn), rh, rw, i0, j0 = _geometry(T0, H, W, crop_size, resize_size)
    out = {}
    if rgb:
        o = po.preprocess_clip(frames, crop_size=(Tn, Hn, Wn), resize_size=(rh, rw), max_frames=10 ** 9, stride=1, spacing=spacing)
        out["rgb_b3thw"] = o["rgb_b3thw"]
    K = torch.Tensor([[min(H, W), 0, W / 2, 0], [0, min(H, W), H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    out["intrinsics_b44t"] = intrinsics_pipeline(K, Tn, H, W, rh, rw, i0, j0)
    # masks: round trip at full size, > 0, mirror-pad, nearest resize, crop - materialised
    if anns is None:
        full = np.zeros((T0, H, W), dtype=np.float32)
    else:
        full = np.stack([(mask_round_trip(a, mode, resize_size).astype(np.float32) / np.float32(255) > 0) for a in anns]).astype(np.float32)
    idx = po.mirror_pad_indices(T0, Tn)
    full = full[idx]
    if not (rh / H == 1.0 and rw / W == 1.0):
        full = full[:, torch_nearest_index(H, rh)][:, :, torch_nearest_index(W, rw)]
    seg = np.ascontiguousarray(full[:Tn, i0:i0 + Hn, j0:j0 + Wn])[None]
    out["instanceseg_b1thw"] = seg
    q = po.grid_queries(spacing, Tn, Hn, Wn)
    sel = select_over_seg(seg[0, 0], seg_cells(spacing))
    out["track_2d_pointquerries_bn3"] = q[sel]
    out["sel"] = sel
    out["ori_video_len"] = np.int64(T0)
    return out


def dycheck_sample(frames: np.ndarray, calibration: Sequence[float], crop_size, resize_size, stride: int, spacing: float,
                   rgb: bool = True) -> Dict[str, np.ndarray]:
    """DycheckDataset.__getitem__ on decoded frames [T,H,W,3] (before the stride) and the calibration line's four numbers."""
    frames = frames[::stride]
    T0, H, W = frames.shape[:3]
    (Tn, Hn, Wn), rh, rw, i0, j0 = _geometry(T0, H, W, crop_size, resize_size)
    out = {}
    if rgb:
        o = po.preprocess_clip(frames, crop_size=(Tn, Hn, Wn), resize_size=(rh, rw), max_frames=10 ** 9, stride=1, spacing=spacing,
                               antialias=False)
        out["rgb_b3thw"] = o["rgb_b3thw"]
    K = torch.eye(4).to(dtype=torch.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = (float(v) for v in calibration)
    out["intrinsics_b44t"] = intrinsics_pipeline(K, Tn, H, W, rh, rw, i0, j0)
    out["extrinsics_b44t"] = np.repeat(np.eye(4, dtype=np.float32)[:, :, None], Tn, axis=2)
    out["track_2d_pointquerries_bn3"] = po.grid_queries(spacing, Tn, Hn, Wn)
    out["ori_video_len"] = np.int64(T0)
    return out
