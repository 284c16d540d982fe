"""Caller side of the hot path: clip preparation on the GPU (mirror of the reference's l4p/data package for the
demo's cases: generic videos, DAVIS, DyCheck; and the L4PDataset base class that prepares ground-truth clips)."""
from .davis import DavisDataset  # noqa: F401
from .dycheck_dataset import DycheckDataset  # noqa: F401
from .l4p_dataset_mini import L4PData, L4PDataset  # noqa: F401
from .npz_dataset import NpzClipDataset  # noqa: F401
from .video_dataset import VideoDataset, pil_resize_blur_resize, prepare_clip  # noqa: F401
