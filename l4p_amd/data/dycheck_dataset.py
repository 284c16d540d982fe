"""`DycheckDataset` — the reference's DyCheck dataset (l4p/data/dycheck_dataset.py:17-109 on top of L4PDataset,
l4p/data/l4p_dataset_mini.py:48-587): RGB frames plus the camera file's intrinsics, per-pixel work on the GPU.

Same constructor arguments and sample dict as the reference (`device` is an addition).  PNG decoding stays on the host (PIL,
exif_transpose, convert("RGB")); there is no resize-blur-resize here, so the frames go straight to the fused resize / crop /
normalise kernel.  The intrinsics of `<seq>/calibration.txt` go through the reference's resize and crop updates
(l4p_dataset_mini.py:281-285, 386-388) on the host in the reference's order of operations; extrinsics_b44t is the identity.
"""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .video_dataset import ESTIMATION_DIRECTIONS, prepare_clip


def read_dycheck_sequence(seq_dir: str, stride: int = 1) -> Tuple[np.ndarray, Tuple[float, float, float, float]]:
    """Decoded frames uint8 [T,H,W,3] of `<seq>/dense/images/*.png` (every stride-th) and (fx, fy, cx, cy) of the first line of
    `<seq>/calibration.txt` (dycheck_dataset.py:74-89)."""
    import PIL.Image
    from PIL.ImageOps import exif_transpose

    img_list = sorted(glob.glob(os.path.join(seq_dir, "dense", "images", "*.png")))[::stride]
    if not img_list:
        raise FileNotFoundError(f"no frames under {os.path.join(seq_dir, 'dense', 'images')}")
    rgbs = []
    for path in img_list:
        with PIL.Image.open(path) as im:
            rgbs.append(np.asarray(exif_transpose(im).convert("RGB")))
    with open(os.path.join(seq_dir, "calibration.txt"), "r") as f:
        first = f.readlines()[0].split(" ")
    return np.stack(rgbs), (float(first[0]), float(first[1]), float(first[2]), float(first[3]))


class DycheckDataset(torch.utils.data.Dataset):
    """Drop-in for l4p.data.dycheck_dataset.DycheckDataset (same arguments; `device` is an addition)."""

    default_sample_size = (16, 224, 224)

    def __init__(
        self,
        data_root: str,
        dataset_type: str = "dycheck",
        stride: int = 1,
        crop_size: Optional[Tuple[int, int, int]] = None,
        resize_size: Union[None, Tuple[int, int], int] = (224, 224),
        center_crop: bool = True,
        start_crop_time: bool = True,
        estimation_directions: Sequence[ESTIMATION_DIRECTIONS] = (1,),
        resize_mode: Dict[str, str] = {"depth_b1thw": "trilinear"},
        track_2d_querry_sampling_spacing: float = 0.02,
        device: Union[str, torch.device] = "cuda",
    ):
        super().__init__()
        if not (center_crop and start_crop_time):
            raise NotImplementedError("random spatial / temporal crops are a training feature; the demo path uses centre crops")
        if resize_mode.get("rgb_b3thw", "trilinear") != "trilinear":
            raise NotImplementedError("the engine implements the reference's default resize mode (trilinear) for rgb")
        if resize_size is not None and not isinstance(resize_size, tuple):
            resize_size = (resize_size, resize_size)
        self.data_root = data_root
        self.dataset_type = dataset_type
        self.stride = stride
        self.crop_size = crop_size
        self.resize_size = resize_size
        self.estimation_directions = list(estimation_directions)
        self.track_2d_querry_sampling_spacing = track_2d_querry_sampling_spacing
        self.length_multiply_of = 8
        self.device = torch.device(device)
        self.seq_list: List[str] = sorted(glob.glob(os.path.join(data_root, "*")))

    def __len__(self) -> int:
        return len(self.seq_list)

    def __getitem__(self, index: int) -> Dict[str, object]:
        seq = self.seq_list[index].split("/")[-1]
        frames, k = read_dycheck_sequence(os.path.join(self.data_root, seq), self.stride)
        frames = torch.from_numpy(frames).to(self.device, non_blocking=True)
        return prepare_clip(frames, self.crop_size, self.resize_size, None, 1, self.track_2d_querry_sampling_spacing,
                            seq_name=f"Dycheck_{seq}", default_sample_size=self.default_sample_size,
                            length_multiply_of=self.length_multiply_of, intrinsics=k, extrinsics=True, blur=False,
                            instanceseg=False, sampling="uniform")
