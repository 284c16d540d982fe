"""Dense scene flow and camera-compensated flow on the GPU (csrc/sceneflow.hip): the engine's dense heads combined across time.

For every pixel p of frame t >= 1 the backward flow sends p to q = p + flow(p) in frame t - 1.  Unprojecting p with depth_t and q
with the bilinearly sampled depth_{t-1} through the camera poses gives two world points; their difference is the *scene flow*: the
pixel's 3D motion in the world frame, pointing backward in time like the flow it comes from.  The *rigid flow* is the flow the
pixel would show if its point were static (depth and pose alone); the *camera-compensated flow* flow - rigid is what is left for
object motion.  On a static pixel it should vanish: its magnitude is a per-pixel consistency signal between the depth, pose and
flow heads, and a geometric cross-check of the motion mask.  The definitions, operation by operation, are at ``l4p_scene_flow``
in include/l4p_hip.h and in DESIGN.md ("Scene flow").

Conventions: every field is "backward" (frame t against frame t - 1); frame 0 has no predecessor, so fields and validity are 0
there; 3D vectors live in the world frame of the poses given (``scene_flow_from_outputs`` re-references them to frame 0 exactly
as ``recon4d.reconstruct_4d`` does, so they add to its ``points``).  Where ``scene_flow_valid_b1thw`` is 0 all fields are 0.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from . import recon4d, vis2d

SUMMARY_COLUMNS = ("n_valid", "n_static", "n_dynamic", "sum_comp_static", "sum_comp_dynamic", "sum_scene_static", "sum_scene_dynamic",
                   "n_moving")
SUMMARY_CHUNK = _lib.L4P_SCENE_FLOW_CHUNK
INVALID_COLOUR = (128, 128, 128)


def _check_shapes(depth, flow, world_T_cam, intrinsics, dyn_mask) -> tuple:
    if depth.dim() != 5 or depth.shape[1] != 1:
        raise ValueError(f"scene_flow: depth_b1thw has shape {tuple(depth.shape)}, expected [B, 1, T, H, W]")
    B, _, T, H, W = depth.shape
    want = {"flow_b2thw": (flow, (B, 2, T, H, W)), "world_T_cam_b44t": (world_T_cam, (B, 4, 4, T)),
            "intrinsics_b44t": (intrinsics, (B, 4, 4, T))}
    if dyn_mask is not None:
        want["dyn_mask_b1thw"] = (dyn_mask, (B, 1, T, H, W))
    for name, (x, shape) in want.items():
        if tuple(x.shape) != shape:
            raise ValueError(f"scene_flow: {name} has shape {tuple(x.shape)}, depth_b1thw {tuple(depth.shape)} needs {shape}")
    if min(B, T, H, W) < 1:
        raise ValueError(f"scene_flow: depth_b1thw has an empty dimension: {tuple(depth.shape)}")
    return B, T, H, W


def scene_flow(depth_b1thw: torch.Tensor, flow_b2thw: torch.Tensor, world_T_cam_b44t: torch.Tensor, intrinsics_b44t: torch.Tensor,
               dyn_mask_b1thw: Optional[torch.Tensor] = None, tau_px: float = 1.0) -> Dict[str, torch.Tensor]:
    """Scene flow, rigid flow and camera-compensated flow of B clips (any B >= 1), as device tensors with no host read-back:

    scene_flow_backward_b3thw f32: X'_{t-1} - X_t in the frame of ``world_T_cam_b44t``;
    rigid_flow_2d_backward_b2thw f32: the flow of a static point, from depth and pose alone (pixels, channel 0 = x);
    compensated_flow_2d_backward_b2thw f32: flow - rigid flow;
    scene_flow_valid_b1thw uint8: 1 where q lies inside the image, both depths are positive, the point is in front of camera
        t - 1 and every result is finite; all fields are 0 elsewhere and on frame 0;
    summary_bt8 f64: per frame, the columns of SUMMARY_COLUMNS (``dyn_mask_b1thw`` logits > 0 are dynamic, <= 0 static; without a
        mask every valid pixel is static; n_moving counts |compensated flow| > ``tau_px``), bit-reproducible.  See ``consistency``.

    ``flow_b2thw`` is the backward flow (pixel p of frame t is found at p + flow in frame t - 1), ``intrinsics_b44t`` pixel
    intrinsics (upper-left 3x3, pixel centres at integer coordinates).  Inputs of any float dtype and layout are converted to
    contiguous f32 on entry."""
    B, T, H, W = _check_shapes(depth_b1thw, flow_b2thw, world_T_cam_b44t, intrinsics_b44t, dyn_mask_b1thw)
    assert depth_b1thw.is_cuda, "scene_flow runs on the GPU"
    dev = depth_b1thw.device
    depth, flow = recon4d._f32(depth_b1thw, dev), recon4d._f32(flow_b2thw, dev)
    P, K = recon4d._f32(world_T_cam_b44t, dev), recon4d._f32(intrinsics_b44t, dev)
    mask = recon4d._f32(dyn_mask_b1thw, dev) if dyn_mask_b1thw is not None else None
    lib, st = _lib.load(), _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    scene = torch.empty(B, 3, T, H, W, **f32)
    rigid, comp = torch.empty(B, 2, T, H, W, **f32), torch.empty(B, 2, T, H, W, **f32)
    valid = torch.empty(B, 1, T, H, W, dtype=torch.uint8, device=dev)
    _lib.check(lib.l4p_scene_flow(st, _p(depth), _p(flow), _p(P), _p(K), _p(mask), B, T, H, W, _p(scene), _p(rigid), _p(comp),
                                  _p(valid)), "l4p_scene_flow")
    ws = torch.empty(B * T * ((H * W + SUMMARY_CHUNK - 1) // SUMMARY_CHUNK) * 8, dtype=torch.float64, device=dev)
    rows = torch.empty(B, T, 8, dtype=torch.float64, device=dev)
    _lib.check(lib.l4p_scene_flow_summary(st, _p(scene), _p(comp), _p(valid), _p(mask), B, T, H, W, float(tau_px), _p(ws), _p(rows)),
               "l4p_scene_flow_summary")
    return {"scene_flow_backward_b3thw": scene, "rigid_flow_2d_backward_b2thw": rigid, "compensated_flow_2d_backward_b2thw": comp,
            "scene_flow_valid_b1thw": valid, "summary_bt8": rows}


def scene_flow_from_outputs(batch: dict, out: dict, tasks: List[str], tau_px: float = 1.0) -> Dict[str, torch.Tensor]:
    """``scene_flow`` on the engine's outputs: depth_est_b1thw, flow_2d_backward_est_b2thw, the camray head's intrinsics
    traj3d_intrinsics_est_b16t and its poses traj3d_est_b16t re-referenced to frame 0 as ``recon4d.reconstruct_4d`` does
    (l4p_recon_cameras, a_is_pose = 1, per batch element), and dyn_mask_est_b1thw when present.  The vectors live in the frame of
    ``reconstruct_4d``'s ``points``.  Also returns world_T_cam_b44t and intrinsics_b44t, the matrices used."""
    assert "depth" in tasks and "camray" in tasks and "flow_2d_backward" in tasks, "Tasks must include depth, camray, flow_2d_backward"
    if "camray_est_b6thw" in out:
        raise ValueError("scene_flow_from_outputs: the camray_est_b6thw branch of the reference is not supported; this engine's "
                         "camray head returns traj3d_est_b16t / traj3d_intrinsics_est_b16t")
    if "traj3d_est_b16t" not in out or "traj3d_intrinsics_est_b16t" not in out:
        raise ValueError("scene_flow_from_outputs needs out['traj3d_est_b16t'] and out['traj3d_intrinsics_est_b16t'] (the camray task)")
    depth = out["depth_est_b1thw"]
    B, _, T, H, W = depth.shape
    dev = depth.device
    for name in ("traj3d_est_b16t", "traj3d_intrinsics_est_b16t"):
        if out[name].numel() != B * 16 * T:
            raise ValueError(f"scene_flow_from_outputs: {name} has shape {tuple(out[name].shape)}, depth_est_b1thw "
                             f"{tuple(depth.shape)} needs {(B, 16, T)}")
    assert dev.type == "cuda", "scene_flow_from_outputs runs on the GPU"
    traj = recon4d._f32(out["traj3d_est_b16t"], dev).reshape(B, 16, T)
    K = recon4d._f32(out["traj3d_intrinsics_est_b16t"], dev).reshape(B, 4, 4, T)
    cam_T_ref = torch.empty(B, 4, 4, T, dtype=torch.float32, device=dev)
    world_T_cam = torch.empty_like(cam_T_ref)
    _lib.check(_lib.load().l4p_recon_cameras(_stream(), _p(traj), B, T, 0, 1, 0.0, 0.0, 0.0, _p(cam_T_ref), _p(world_T_cam), None),
               "l4p_recon_cameras")
    res = scene_flow(depth, out["flow_2d_backward_est_b2thw"], world_T_cam, K, out.get("dyn_mask_est_b1thw"), tau_px)
    res.update(world_T_cam_b44t=world_T_cam, intrinsics_b44t=K)
    return res


def consistency(summary_bt8: torch.Tensor, pixels_per_frame: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The user-facing numbers of a summary, per clip ([B] float64 on the summary's device; frames are added first):

    rigid_epe_static / rigid_epe_dynamic: mean |compensated flow| over static / dynamic valid pixels (pixels).  The static one is
        the end-point error between the flow head and the flow implied by depth and pose where nothing should move;
    scene_speed_static / scene_speed_dynamic: mean |scene flow| per frame step (world units);
    moving_fraction: n_moving / n_valid; valid_fraction: n_valid / ((T - 1) pixels_per_frame), only with ``pixels_per_frame``
        (H W: the summary does not hold it).
    A ratio whose denominator is 0 is NaN."""
    if summary_bt8.dim() != 3 or summary_bt8.shape[2] != 8:
        raise ValueError(f"consistency: summary_bt8 has shape {tuple(summary_bt8.shape)}, expected [B, T, 8]")
    s = summary_bt8.to(torch.float64).sum(dim=1)
    nan = torch.full_like(s[:, 0], float("nan"))

    def ratio(num, den):
        return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), nan)

    res = {"rigid_epe_static": ratio(s[:, 3], s[:, 1]), "rigid_epe_dynamic": ratio(s[:, 4], s[:, 2]),
           "scene_speed_static": ratio(s[:, 5], s[:, 1]), "scene_speed_dynamic": ratio(s[:, 6], s[:, 2]),
           "moving_fraction": ratio(s[:, 7], s[:, 0])}
    if pixels_per_frame is not None:
        den = torch.full_like(s[:, 0], float((summary_bt8.shape[1] - 1) * int(pixels_per_frame)))
        res["valid_fraction"] = ratio(s[:, 0], den)
    return res


_LUT_CACHE: Dict[torch.device, torch.Tensor] = {}


def motion_lut() -> np.ndarray:
    """uint8 [256, 3]: ``vis2d.turbo_table()`` through ``recon4d.colour_bytes``."""
    return recon4d.colour_bytes(vis2d.turbo_table())


def default_s_max(res: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The colour scale ``motion_colors`` uses by default, f32 [1] on the device: the 0.98 quantile (``l4p_quantile``:
    torch.quantile's linear interpolation) of |scene flow| over ALL B T H W elements, the zeros of invalid pixels and of frame 0
    included, and 1 when that quantile is 0."""
    scene = res["scene_flow_backward_b3thw"]
    assert scene.is_cuda, "default_s_max runs on the GPU"
    mag = (scene * scene).sum(dim=1).sqrt().contiguous()
    ws = torch.empty(_lib.L4P_QUANTILE_WS_UINTS, dtype=torch.int32, device=scene.device)
    q = torch.empty(1, dtype=torch.float32, device=scene.device)
    _lib.check(_lib.load().l4p_quantile(_stream(), _p(mag), mag.numel(), 0.98, _p(ws), _p(q)), "l4p_quantile")
    return torch.where(q == 0, torch.ones_like(q), q)


def motion_colors(res: Dict[str, torch.Tensor], s_max=None) -> torch.Tensor:
    """uint8 [B, T*H*W, 3], frame-major like ``reconstruct_4d``'s ``colors``: a valid pixel takes entry
    floor(255 min(1, |scene flow| / s_max)) (f32) of ``motion_lut()``, an invalid one INVALID_COLOUR.

    ``s_max`` is a number or a one-element device tensor; by default ``default_s_max(res)``: the 0.98 quantile of |scene flow| over
    all elements, the zeros of invalid pixels included, and 1 when that quantile is 0.  It is formed and consumed on the device."""
    scene, valid = res["scene_flow_backward_b3thw"], res["scene_flow_valid_b1thw"]
    assert scene.is_cuda, "motion_colors runs on the GPU"
    B, _, T, H, W = scene.shape
    dev = scene.device
    lib, st = _lib.load(), _stream()
    if s_max is None:
        s_max = default_s_max(res)
    elif not torch.is_tensor(s_max):
        s_max = torch.full((1,), float(s_max), dtype=torch.float32, device=dev)
    s_max = s_max.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    if dev not in _LUT_CACHE:
        _LUT_CACHE[dev] = torch.from_numpy(motion_lut()).contiguous().to(dev)
    colors = torch.empty(B, T * H * W, 3, dtype=torch.uint8, device=dev)
    _lib.check(lib.l4p_scene_flow_colors(st, _p(scene.contiguous()), _p(valid.contiguous()), _p(_LUT_CACHE[dev]), B, T, H, W,
                                         _p(s_max), _p(colors)), "l4p_scene_flow_colors")
    return colors


def render_scene_flow_panels(batch: dict, out: dict, tasks: List[str], res: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """[RGB | flow | camera-compensated flow] of batch element 0 as a device tensor [T, H, 3 W, 3] float32: two calls of
    ``vis2d.render_video_panels`` with tasks ["flow_2d_backward"], the second on a shallow copy of ``out`` whose flow is the
    compensated flow (each flow panel is normalised by its own largest radius, as that renderer does)."""
    if res is None:
        res = scene_flow_from_outputs(batch, out, tasks)
    W = batch["rgb_b3thw"].shape[-1]
    first = vis2d.render_video_panels(batch, out, ["flow_2d_backward"])["video"]
    out2 = dict(out)
    out2["flow_2d_backward_est_b2thw"] = res["compensated_flow_2d_backward_b2thw"]
    second = vis2d.render_video_panels(batch, out2, ["flow_2d_backward"])["video"]
    return torch.cat([first, second[:, :, W:]], dim=2)


def generate_scene_flow_video(batch, out, tasks, out_path=None, res: Optional[Dict[str, torch.Tensor]] = None):
    """Writes <out_path>/<seq_name>_sceneflow (.mp4 with mediapy, PNG frames in a directory of that name without) through
    ``vis2d.write_video`` and returns (the video float32 [T, H, 3 W, 3] on the host, the name written or None)."""
    video = render_scene_flow_panels(batch, out, tasks, res).cpu().numpy()
    name = vis2d.write_video(video, out_path, batch["seq_name"][0] + "_sceneflow") if out_path is not None else None
    return video, name
