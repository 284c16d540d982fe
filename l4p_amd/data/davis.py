"""`DavisDataset` — the reference's DAVIS dataset (l4p/data/davis.py:24-141 on top of L4PDataset,
l4p/data/l4p_dataset_mini.py:48-587) with the per-pixel work on the GPU.

Same constructor arguments and sample dict as the reference (`device` is an addition); tensors live on the GPU.
  * JPEG / PNG decoding stays on the host (PIL), as video decoding does for VideoDataset;
  * the RGB path is VideoDataset's (resize-blur-resize passes + the fused resize / crop / normalise kernel);
  * the instance masks (davis.py:96-110, then mirror padding, nearest resize and centre crop) are one launch of
    l4p_instance_mask_clip on index tables composed on the host - for palette annotations Pillow's resize is NEAREST whatever
    filter is asked for, so the whole chain is an index map; 8-bit annotations go through the bilinear passes first;
  * the queries are sampled on top of the eroded first-frame mask (sample_tracks "uniform_over_seg", :450-465) by
    l4p_seg_query_select; reading the number of kept queries is the only synchronisation.
"""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .video_dataset import ESTIMATION_DIRECTIONS, _BILINEAR_MODES, _NEAREST_MODES, prepare_clip


def read_davis_sequence(scene_dir: str, stride: int = 1) -> Tuple[np.ndarray, Optional[np.ndarray], str]:
    """Decoded frames uint8 [T,H,W,3], annotation frames (uint8 [T,H,W] or [T,H,W,3]; None when the sequence has none) and their PIL
    mode, for `JPEGImages/480p/<seq>/%05d.jpg` and the matching `Annotations/480p/<seq>/%05d.png` (davis.py:82-107)."""
    from PIL import Image

    T = len(glob.glob(os.path.join(scene_dir, "*.jpg")))
    rgbs, anns, mode = [], [], None
    for i in range(0, T, stride):
        rgb_path = os.path.join(scene_dir, "%05d.jpg" % i)
        with Image.open(rgb_path) as im:
            rgbs.append(np.asarray(im.convert("RGB")))
        ann_path = rgb_path.replace("JPEGImages", "Annotations").replace("jpg", "png")
        if os.path.isfile(ann_path):
            with Image.open(ann_path) as im:
                if mode is None:
                    mode = im.mode
                if im.mode != mode:
                    raise NotImplementedError(f"{ann_path}: annotation modes {mode!r} and {im.mode!r} in one sequence")
                if mode not in _NEAREST_MODES + _BILINEAR_MODES:
                    raise NotImplementedError(f"{ann_path}: annotation mode {mode!r}")
                a = np.asarray(im)
                anns.append(a.astype(np.uint8) if a.dtype == bool else a)
        else:
            anns.append(None)  # davis.py:105-106: an all-zero mask
    frames = np.stack(rgbs)
    if mode is None:
        return frames, None, "P"
    zero = np.zeros(next(a for a in anns if a is not None).shape, dtype=np.uint8)
    return frames, np.stack([zero if a is None else a for a in anns]), mode


class DavisDataset(torch.utils.data.Dataset):
    """Drop-in for l4p.data.davis.DavisDataset (same arguments; `device` is an addition)."""

    default_sample_size = (16, 224, 224)

    def __init__(
        self,
        data_root: str,
        dataset_type: str = "davis",
        stride: int = 1,
        crop_size: Union[None, Tuple[int, int, int]] = None,
        resize_size: Tuple[int, int] = (224, 224),
        center_crop: bool = True,
        start_crop_time: bool = True,
        estimation_directions: Sequence[ESTIMATION_DIRECTIONS] = (1,),
        resize_mode: Dict[str, str] = {"rgb_b3thw": "trilinear"},
        track_2d_querry_sampling_spacing: float = 0.02,
        device: Union[str, torch.device] = "cuda",
    ):
        super().__init__()
        if not (center_crop and start_crop_time):
            raise NotImplementedError("random spatial / temporal crops are a training feature; the demo path uses centre crops")
        if resize_mode.get("rgb_b3thw", "trilinear") != "trilinear" or resize_mode.get("instanceseg_b1thw", "nearest") != "nearest":
            raise NotImplementedError("the engine implements the reference's default resize modes (trilinear rgb, nearest masks)")
        if isinstance(resize_size, int):
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
        self.scene_list: List[str] = sorted(glob.glob(os.path.join(self.data_root, "JPEGImages/480p/*")))
        self.len = len(self.scene_list)

    def __len__(self) -> int:
        return self.len

    def __getitem__(self, index: int) -> Dict[str, object]:
        scene = self.scene_list[index]
        frames, anns, mode = read_davis_sequence(scene, self.stride)
        frames = torch.from_numpy(frames).to(self.device, non_blocking=True)
        anns = torch.from_numpy(anns).to(self.device, non_blocking=True) if anns is not None else None
        return prepare_clip(frames, self.crop_size, self.resize_size, None, 1, self.track_2d_querry_sampling_spacing,
                            seq_name=str(os.path.basename(scene)), default_sample_size=self.default_sample_size,
                            length_multiply_of=self.length_multiply_of, annotations=anns, annotation_mode=mode,
                            sampling="uniform_over_seg")
