"""Static scene map on the GPU (csrc/static_map.hip): the clip's per-frame world points fused into one voxel map.

``reconstruct_4d`` returns every pixel of every frame as a world point; this stage merges the frames.  Points are hashed into
voxels of a regular grid; a voxel is kept when at least ``min_frames`` different frames put a point in it and none of its points is
covered by the motion mask - so a piece of static surface appears once instead of once per frame, flying pixels that a single
frame saw are rejected, movers stay out, and the size of the map follows the scene, not the clip length.  Every per-voxel quantity
is an integer sum, a minimum or a maximum: the map is the same bit for bit on every run, and voxels leave in the order of their
first point.  The rule, operation by operation, is at ``l4p_static_map_insert`` in include/l4p_hip.h and in DESIGN.md ("Static
scene map").  The reference has no counterpart: its PLY files are per frame.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import torch

from .. import _lib
from ..ops import _p, _stream
from . import recon4d

COUNTERS = ("n_points", "n_used", "n_nonfinite", "n_masked", "n_out_of_range", "n_voxels", "n_kept", "n_overflow")
MAX_POINTS = 1 << 24  # the colour sums of a voxel are 32-bit: 255 * 2^24 < 2^32
MAX_CAPACITY = 1 << 30


def default_capacity(M: int) -> int:
    """The smallest power of two >= 2 M: the table is at most half full."""
    return 1 << max(0, (2 * int(M) - 1).bit_length())


def _check(points, colors, T, voxel_size, origin, grid, dyn_mask, keep, min_frames, min_points, table_capacity) -> tuple:
    """Every argument error of ``fuse_points``, on shapes and host values only: nothing here touches a device."""
    if (voxel_size is None) == (grid is None):
        raise ValueError("fuse_points: give exactly one of voxel_size and grid")
    if voxel_size is not None:
        v = float(voxel_size)
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f"fuse_points: voxel_size must be finite and > 0, got {voxel_size}")
        if len(tuple(origin)) != 3 or not all(math.isfinite(float(o)) for o in origin):
            raise ValueError(f"fuse_points: origin must be three finite numbers, got {origin}")
    elif not torch.is_tensor(grid) or grid.numel() != 4 or not grid.is_floating_point():
        raise ValueError("fuse_points: grid must be a float tensor of 4 elements (ox, oy, oz, voxel size)")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or not points.is_floating_point():
        raise ValueError(f"fuse_points: points must be a float tensor [M, 3], got {_describe(points)}")
    M = int(points.shape[0])
    if not torch.is_tensor(colors) or tuple(colors.shape) != (M, 3) or colors.dtype != torch.uint8:
        raise ValueError(f"fuse_points: colors must be a uint8 tensor [{M}, 3], got {_describe(colors)}")
    if int(T) < 1 or M < 1 or M % int(T) != 0:
        raise ValueError(f"fuse_points: the {M} points do not divide into T = {T} frames of one size")
    if M > MAX_POINTS:
        raise ValueError(f"fuse_points: {M} points, at most {MAX_POINTS}")
    if dyn_mask is not None and (not torch.is_tensor(dyn_mask) or dyn_mask.numel() != M or not dyn_mask.is_floating_point()):
        raise ValueError(f"fuse_points: dyn_mask must be a float tensor of {M} logits, got {_describe(dyn_mask)}")
    if keep is not None and (not torch.is_tensor(keep) or keep.numel() != M or keep.dtype not in (torch.uint8, torch.bool)):
        raise ValueError(f"fuse_points: keep must be a uint8 or bool tensor of {M} elements, got {_describe(keep)}")
    if int(min_frames) < 1:
        raise ValueError(f"fuse_points: min_frames must be >= 1, got {min_frames}")
    if int(min_points) < 1:
        raise ValueError(f"fuse_points: min_points must be >= 1, got {min_points}")
    cap = default_capacity(M) if table_capacity is None else int(table_capacity)
    if cap < 1 or cap & (cap - 1) or cap > MAX_CAPACITY:
        raise ValueError(f"fuse_points: table_capacity must be a power of two in [1, 2^30], got {table_capacity}")
    return M, cap


def _describe(x) -> str:
    return f"{tuple(x.shape)} {x.dtype}" if torch.is_tensor(x) else type(x).__name__


def fuse_points(points: torch.Tensor, colors: torch.Tensor, T: int, voxel_size: Optional[float] = None, origin=(0.0, 0.0, 0.0),
                grid: Optional[torch.Tensor] = None, dyn_mask: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                min_frames: int = 2, min_points: int = 1, table_capacity: Optional[int] = None) -> Dict[str, object]:
    """Fuse the frame-major cloud ``points`` [M, 3] / ``colors`` [M, 3] uint8 (M = T HW, as ``reconstruct_4d`` returns them) into
    one voxel map.  The grid is ``voxel_size`` and ``origin`` (host numbers) or ``grid`` = (ox, oy, oz, v) as a 4-element device
    tensor, e.g. a voxel size computed on the device.  A point is left out when a coordinate is not finite, when its ``dyn_mask``
    logit is > 0, when its ``keep`` byte is 0 or when its voxel index leaves [-2^20, 2^20); a voxel is kept when ``min_frames``
    different frames and ``min_points`` points fell into it.  Returns device tensors, V voxels in the order of their first point:

    xyz [V, 3] f32: the mean position of the voxel's points (of their 16-bit in-voxel fractions: within v / 65536 per axis);
    colors [V, 3] uint8: the mean colour, rounded half up;
    count, n_frames, first_frame, last_frame, first_point [V] int32; key [V] int64 (the packed voxel index);
    voxel_id [M] int32: the row of the point's voxel, -1 where the point or its voxel was left out;
    grid [4] f32: the grid used; counters: a host dict of COUNTERS (n_points = n_used + n_nonfinite + n_masked + n_out_of_range).

    Points of any float dtype and layout are converted to contiguous f32 on entry.  The call reads ``counters`` back once (one
    synchronisation) to size the outputs, as ``reconstruct_4d`` does for its trails.  ``table_capacity`` (a power of two; default
    the smallest >= 2 M) is the number of 64-byte hash slots; a table too small for the voxels raises ``L4PHipError``."""
    M, cap = _check(points, colors, T, voxel_size, origin, grid, dyn_mask, keep, min_frames, min_points, table_capacity)
    assert points.is_cuda, "fuse_points runs on the GPU"
    dev = points.device
    T, HW = int(T), M // int(T)
    pts = recon4d._f32(points, dev)
    col = colors.to(dev).contiguous()
    if grid is None:
        grid = torch.tensor([float(o) for o in origin] + [float(voxel_size)], dtype=torch.float32).to(dev)
    grid = recon4d._f32(grid, dev).reshape(4)
    mask = recon4d._f32(dyn_mask, dev).reshape(M) if dyn_mask is not None else None
    kp = keep.to(device=dev, dtype=torch.uint8).reshape(M).contiguous() if keep is not None else None
    lib, st = _lib.load(), _stream()
    ws = torch.empty(int(lib.l4p_static_map_ws_bytes(cap, M)), dtype=torch.uint8, device=dev)
    counters = torch.empty(8, dtype=torch.int64, device=dev)
    _lib.check(lib.l4p_static_map_insert(st, _p(pts), _p(col), _p(mask), _p(kp), _p(grid), T, HW, cap, _p(ws)), "l4p_static_map_insert")
    _lib.check(lib.l4p_static_map_count(st, _p(ws), T, HW, cap, int(min_frames), int(min_points), _p(counters)), "l4p_static_map_count")
    host = dict(zip(COUNTERS, (int(v) for v in counters.cpu().tolist())))  # the one host read-back: sizes the outputs
    if host["n_overflow"]:
        raise _lib.L4PHipError(f"fuse_points: the hash table is full: table_capacity {cap} slots, n_voxels {host['n_voxels']} "
                               f"voxels found a slot and {host['n_overflow']} points did not; pass a larger table_capacity")
    V = host["n_kept"]
    i32 = dict(dtype=torch.int32, device=dev)
    res = {"xyz": torch.empty(V, 3, dtype=torch.float32, device=dev), "colors": torch.empty(V, 3, dtype=torch.uint8, device=dev)}
    for k in ("count", "n_frames", "first_frame", "last_frame", "first_point"):
        res[k] = torch.empty(V, **i32)
    res["key"] = torch.empty(V, dtype=torch.int64, device=dev)
    res["voxel_id"] = torch.empty(M, **i32)
    _lib.check(lib.l4p_static_map_emit(st, _p(ws), _p(grid), T, HW, cap, V, _p(res["xyz"]), _p(res["colors"]), _p(res["count"]),
                                       _p(res["n_frames"]), _p(res["first_frame"]), _p(res["last_frame"]), _p(res["first_point"]),
                                       _p(res["key"]), _p(res["voxel_id"])), "l4p_static_map_emit")
    res.update(grid=grid, counters=host)
    return res


def default_grid(out: dict, voxel_px: float = 2.0) -> torch.Tensor:
    """(0, 0, 0, v) f32 [4] on the device, v = voxel_px * median(frame-0 depth) / fx_0: the world size of ``voxel_px`` pixels at the
    median depth of frame 0 (``l4p_quantile`` at 0.5: torch.quantile's median; fx_0 from traj3d_intrinsics_est_b16t).  The origin is
    0: the world frame is camera 0.  Formed on the device, no read-back."""
    depth = out["depth_est_b1thw"]
    dev = depth.device
    assert dev.type == "cuda", "default_grid runs on the GPU"
    d0 = recon4d._f32(depth[0, 0, 0], dev).reshape(-1)
    ws = torch.empty(_lib.L4P_QUANTILE_WS_UINTS, dtype=torch.int32, device=dev)
    med = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().l4p_quantile(_stream(), _p(d0), d0.numel(), 0.5, _p(ws), _p(med)), "l4p_quantile")
    T = depth.shape[2]
    fx0 = recon4d._f32(out["traj3d_intrinsics_est_b16t"], dev).reshape(16, T)[0, 0]
    grid = torch.zeros(4, dtype=torch.float32, device=dev)
    grid[3] = (float(voxel_px) * med[0]) / fx0
    return grid


def static_map_from_outputs(batch: dict, out: dict, tasks: List[str], voxel_px: float = 2.0, min_frames: int = 2,
                            rec: Optional[Dict[str, torch.Tensor]] = None, keep_b1thw: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """``fuse_points`` on the engine's outputs: the points and colours of ``recon4d.reconstruct_4d`` (or the passed ``rec``),
    out["dyn_mask_est_b1thw"] as the motion mask when present, ``keep_b1thw`` (uint8 / bool, 0 = leave the pixel out) as a further
    filter, and ``default_grid(out, voxel_px)``.  B = 1 only, with ``reconstruct_4d``'s assertions and errors."""
    B, _, T, H, W = batch["rgb_b3thw"].shape
    assert "depth" in tasks and "camray" in tasks, "Tasks must include depth, camray"
    assert B == 1, "Current implementation supports only batch size 1"
    if "camray_est_b6thw" in out:
        raise ValueError("static_map_from_outputs: the camray_est_b6thw branch of the reference is not supported; this engine's camray "
                         "head returns traj3d_est_b16t / traj3d_intrinsics_est_b16t")
    if "traj3d_est_b16t" not in out or "traj3d_intrinsics_est_b16t" not in out:
        raise ValueError("static_map_from_outputs needs out['traj3d_est_b16t'] and out['traj3d_intrinsics_est_b16t'] (the camray task)")
    if float(voxel_px) <= 0 or not math.isfinite(float(voxel_px)):
        raise ValueError(f"static_map_from_outputs: voxel_px must be finite and > 0, got {voxel_px}")
    if rec is None:
        rec = recon4d.reconstruct_4d(batch, out, [t for t in tasks if t != "track_2d"])
    mask = out.get("dyn_mask_est_b1thw")
    return fuse_points(rec["points"], rec["colors"], T, grid=default_grid(out, voxel_px),
                       dyn_mask=mask.reshape(-1) if mask is not None else None,
                       keep=keep_b1thw.reshape(-1) if keep_b1thw is not None else None, min_frames=min_frames)


def generate_static_map(batch, out, tasks, out_path, voxel_px: float = 2.0, min_frames: int = 2,
                        res: Optional[Dict[str, object]] = None) -> str:
    """Writes <out_path>/<seq_name>_static_map.ply (``recon4d.write_ply``: the voxels' positions and colours) and
    <seq_name>_static_map.json (the counters, voxel_size, min_frames and compression = n_used / n_kept, null for an empty map), and
    returns the PLY's name."""
    if res is None:
        res = static_map_from_outputs(batch, out, tasks, voxel_px=voxel_px, min_frames=min_frames)
    os.makedirs(out_path, exist_ok=True)
    base = os.path.join(out_path, batch["seq_name"][0] + "_static_map")
    recon4d.write_ply(base + ".ply", res["xyz"].cpu().numpy(), res["colors"].cpu().numpy())
    c = res["counters"]
    info = dict(c, voxel_size=float(res["grid"][3]), min_frames=int(min_frames),
                compression=c["n_used"] / c["n_kept"] if c["n_kept"] else None)
    with open(base + ".json", "w") as fh:
        json.dump(info, fh, indent=1)
    return base + ".ply"
