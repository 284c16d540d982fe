"""`NpzClipDataset` — raw ground-truth clips from a directory of .npz files, prepared by the `L4PDataset` base class.

Each .npz holds one clip as a dataset DECODES it, before any preparation: arrays under the L4PData field names without the batch
dimension, at the dataset's own resolution and length (rgb_b3thw [3, T, H, W] as float in [0, 1] or as uint8; depth_b1thw,
flow_2d_backward_b2thw, track_2d_traj_bn2t [N, 2, T], ...).  Resizing, cropping, mirror padding and query filtering to the
network's geometry happen on the GPU (l4p_dataset_mini.py)."""
from __future__ import annotations

import glob
import os
from dataclasses import fields

import numpy as np
import torch

from .l4p_dataset_mini import L4PData, L4PDataset

_TENSOR_FIELDS = tuple(f.name for f in fields(L4PData) if f.name not in ("dataset_name", "seq_name"))


class NpzClipDataset(L4PDataset):
    def __init__(self, data_root: str, dataset_name: str = "npz", **kwargs) -> None:
        super().__init__(**kwargs)
        self.files = sorted(glob.glob(os.path.join(data_root, "*.npz")))
        self.dataset_name = dataset_name

    def __len__(self) -> int:
        return len(self.files)

    def getitem_helper(self, index: int) -> L4PData:
        path = self.files[index]
        data = {}
        with np.load(path, allow_pickle=False) as z:
            for key in z.files:
                if key not in _TENSOR_FIELDS:
                    continue
                t = torch.from_numpy(np.ascontiguousarray(z[key]))
                if key == "rgb_b3thw" and t.dtype == torch.uint8:
                    t = t.to(torch.float32).div(255)
                elif key in ("track_2d_vis_bn1t", "track_2d_valid_bn1t"):
                    t = t.to(torch.bool)
                else:
                    t = t.to(torch.float32)
                data[key] = t
        return L4PData(dataset_name=self.dataset_name, seq_name=os.path.splitext(os.path.basename(path))[0], **data)
