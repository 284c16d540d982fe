"""Pose geometry on the GPU — host mirror of the parts of l4p/utils/geometry_utils.py on the hot path."""
from __future__ import annotations

import torch

from .. import _lib
from ..ops import _p, _stream


def normalize_intrinsics(intrinsics_b44t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """geometry_utils.py:110-116 (kept for callers; the pose kernel re-scales intrinsics itself)."""
    K = intrinsics_b44t.clone().detach()
    K[:, :2, 2] += 0.5
    K[:, 0] = K[:, 0] / w
    K[:, 1] = K[:, 1] / h
    return K


def poses_from_rays(rays_b6thw: torch.Tensor, intrinsics_b44t: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """rays_to_cameras(rays, normalize_intrinsics(K, H, W)) followed by torch.linalg.inv and the b16t reshape
    (geometry_utils.py:331-406; dense_heads.py:322-348) as one kernel: float [B,6,T,h,w] -> float [B,16,T]."""
    assert rays_b6thw.is_cuda and rays_b6thw.dtype == torch.float32
    B, six, T, h, w = rays_b6thw.shape
    assert six == 6 and tuple(intrinsics_b44t.shape) == (B, 4, 4, T)
    rays = rays_b6thw.contiguous()
    K = intrinsics_b44t.to(device=rays.device, dtype=torch.float32).contiguous()
    out = torch.empty(B, 16, T, dtype=torch.float32, device=rays.device)
    _lib.check(_lib.load().l4p_rays_to_pose(_stream(), _p(rays), _p(K), _p(out), B, T, h, w, H, W), "l4p_rays_to_pose")
    return out


def cameras_from_rays_variable_intrinsics(rays_b6thw: torch.Tensor, H: int, W: int, reproj_threshold: float = 0.2):
    """rays_to_cameras_and_variable_per_frame_intrinsics (geometry_utils.py:582-654) + the pose inversion of
    dense_heads.py:346-348: every frame's own K and the rotation of H^-1 = K R as that frame's camera rotation.
    float [B,6,T,h,w] -> (world_T_cam float [B,16,T], K float [B,4,4,T] in pixel units of the H x W image)."""
    assert rays_b6thw.is_cuda and rays_b6thw.dtype == torch.float32
    B, six, T, h, w = rays_b6thw.shape
    rays = rays_b6thw.contiguous()
    K = torch.empty(B, 4, 4, T, dtype=torch.float32, device=rays.device)
    R = torch.empty(B, 9, T, dtype=torch.float32, device=rays.device)
    pose = torch.empty(B, 16, T, dtype=torch.float32, device=rays.device)
    lib = _lib.load()
    _lib.check(lib.l4p_rays_to_intrinsics_frames(_stream(), _p(rays), _p(K), _p(R), None, B, T, h, w, H, W, reproj_threshold),
               "l4p_rays_to_intrinsics_frames")
    _lib.check(lib.l4p_rays_to_pose_rot(_stream(), _p(rays), _p(R), _p(pose), B, T, h, w), "l4p_rays_to_pose_rot")
    return pose, K


def intrinsics_from_rays(rays_b6thw: torch.Tensor, H: int, W: int, reproj_threshold: float = 0.2, frame: int = 0) -> torch.Tensor:
    """Fixed intrinsics from the first frame's ray map (rays_to_cameras_and_fixed_per_frame_intrinsics,
    geometry_utils.py:493-579, K part): float [B,6,T,h,w] -> float [B,4,4,T] in pixel units of the H x W image."""
    assert rays_b6thw.is_cuda and rays_b6thw.dtype == torch.float32
    B, six, T, h, w = rays_b6thw.shape
    rays = rays_b6thw.contiguous()
    K = torch.empty(B, 4, 4, T, dtype=torch.float32, device=rays.device)
    _lib.check(_lib.load().l4p_rays_to_intrinsics(_stream(), _p(rays), _p(K), None, B, T, h, w, H, W, frame, reproj_threshold),
               "l4p_rays_to_intrinsics")
    return K


def _b44t(x: torch.Tensor, device) -> torch.Tensor:
    return x.to(device=device, dtype=torch.float32).contiguous()


def generate_point_map(depth_b1thw: torch.Tensor, intrinsics_b44t: torch.Tensor, world_T_cam_b44t: torch.Tensor) -> torch.Tensor:
    """geometry_utils.py:13-53: every pixel (i, j) -> world_T_cam [depth K^-1 [i, j, 1]^T; 1] (csrc/recon4d.hip, f32).
    depth [B,1,T,H,W], intrinsics / world_T_cam [B,4,4,T] -> [B,3,T,H,W] in depth's dtype."""
    assert depth_b1thw.is_cuda, "generate_point_map runs on the GPU"
    B, _, T, H, W = depth_b1thw.shape
    dev = depth_b1thw.device
    d = _b44t(depth_b1thw, dev)
    K, P = _b44t(intrinsics_b44t, dev), _b44t(world_T_cam_b44t, dev)
    assert tuple(K.shape) == (B, 4, 4, T) and tuple(P.shape) == (B, 4, 4, T)
    out = torch.empty(B, 3, T, H, W, dtype=torch.float32, device=dev)
    thw = T * H * W
    _lib.check(_lib.load().l4p_point_map(_stream(), _p(d), _p(K), _p(P), B, T, H, W, _p(out), 1, thw, 3 * thw, None, None, None, None),
               "l4p_point_map")
    return out.to(dtype=depth_b1thw.dtype)


def generate_3d_track_point_map(track_2d_traj_bn2t: torch.Tensor, track_2d_depth_bn1t: torch.Tensor, intrinsics_b44t: torch.Tensor,
                                world_T_cam_b44t: torch.Tensor) -> torch.Tensor:
    """geometry_utils.py:84-106 with unproject_2d_track_to_3d (:56-81): X = (x - cx) Z / fx, Y = (y - cy) Z / fy, then
    world_T_cam [X Y Z 1] (csrc/recon4d.hip, f32).  traj [B,N,2,T], depth [B,N,1,T], [B,4,4,T] matrices -> [B,N,3,T] f32."""
    assert track_2d_traj_bn2t.is_cuda, "generate_3d_track_point_map runs on the GPU"
    B, N, _, T = track_2d_traj_bn2t.shape
    dev = track_2d_traj_bn2t.device
    tr, dp = _b44t(track_2d_traj_bn2t, dev), _b44t(track_2d_depth_bn1t, dev)
    K, P = _b44t(intrinsics_b44t, dev), _b44t(world_T_cam_b44t, dev)
    out = torch.empty(B, N, 3, T, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().l4p_track_point_map(_stream(), _p(tr), _p(dp), _p(K), _p(P), None, None, B, N, T, _p(out)),
               "l4p_track_point_map")
    return out


def get_cam_T_ref(cam_T_world_b44t: torch.Tensor, ref_idx: int = 0) -> torch.Tensor:
    """geometry_utils.py:128-143: cam_T_world[t] @ inv(cam_T_world[ref_idx]) per frame, [B,4,4,T] -> [B,4,4,T] f32
    (csrc/recon4d.hip; the product runs in double and rounds once)."""
    assert cam_T_world_b44t.is_cuda, "get_cam_T_ref runs on the GPU"
    B, _, _, T = cam_T_world_b44t.shape
    A = _b44t(cam_T_world_b44t, cam_T_world_b44t.device)
    out = torch.empty_like(A)
    _lib.check(_lib.load().l4p_recon_cameras(_stream(), _p(A), B, T, int(ref_idx) % T, 0, 0.0, 0.0, 0.0, _p(out), None, None),
               "l4p_recon_cameras")
    return out
