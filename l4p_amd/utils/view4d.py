"""The 4D reconstruction from a free viewpoint, rendered on the GPU: what the reference's demo shows through its viser viewer
(``visualize_point_cloud_viser``, l4p/utils/viser.py:58-75 - the world point cloud of frame t, its 3D track trails and the camera
frustum, from a camera the user moves, with a slider over t) as depth-tested images, with every stage in csrc/view4d.hip.

``render_4d_views`` turns the device tensors of ``recon4d.reconstruct_4d`` into images without a host synchronisation;
``orbit_views`` supplies a camera path (there is no user to move the camera); ``generate_4D_video`` chains reconstruction, path,
renderer and ``vis2d.write_video``.  The module is not named ``viser``: ``import l4p.utils.viser`` keeps raising ImportError.

The viewer's rasteriser (WebGL point sprites) cannot be run or read where this was written; the projection, coverage and depth
rules are the project's own, stated at ``l4p_view_splat`` / ``l4p_view_mesh`` / ``l4p_view_resolve`` (include/l4p_hip.h) and
restated in numpy by tests/view4d_restate.py, which the GPU tests hold bit for bit.  A point is a screen-aligned square of
world size ``point_size`` (capped at ``2 * max_half + 1`` pixels), the nearest surface wins, ties go to the lowest index.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from . import vis2d
from .recon4d import _f32, reconstruct_4d

FRUSTUM_COLOUR_U8 = (255, 127, 127)  # colour_bytes(recon4d.FRUSTUM_COLOUR)
# triangle k of recon4d.FRUSTUM_TRIANGLES is drawn in FRUSTUM_COLOUR_U8 * FRUSTUM_SHADE[k] // 32: faces are told apart without lighting
FRUSTUM_SHADE = (32, 31, 18, 17, 27, 26, 23, 22, 29, 28, 21, 20)
MESH_BIT = 0x80000000  # index: high bit set = a frustum triangle, low bits frame << 4 | triangle
WORKSPACE_BYTES = 64 << 20  # default budget of the z-buffer workspace (8 bytes per pixel and view of a chunk)


def mesh_colours() -> np.ndarray:
    """uint8 [12, 3]: the colour of each frustum triangle."""
    return (np.asarray(FRUSTUM_COLOUR_U8, dtype=np.int64)[None] * np.asarray(FRUSTUM_SHADE, dtype=np.int64)[:, None] // 32).astype(np.uint8)


def frusta_stride(frusta) -> int:
    """The ``stride`` of l4p_view_mesh for ``frusta``: "current" -> 0 (the frustum of the view's own frame), an int s >= 1 -> s (also
    every earlier frame f with f % s == 0: the camera path), "none" / None / False -> -1 (no frusta)."""
    if frusta is None or frusta is False or frusta == "none":
        return -1
    if frusta == "current":
        return 0
    if isinstance(frusta, (int, np.integer)) and not isinstance(frusta, bool) and frusta >= 1:
        return int(frusta)
    raise ValueError(f"frusta is 'current', 'none' or a stride >= 1, not {frusta!r}")


def render_4d_views(rec: Dict[str, torch.Tensor], T: int, hw: int, cam_T_world, intrinsics, size: Tuple[int, int], frames,
                    point_size: float = 0.02, max_half: int = 16, near: float = 1e-3, background=(0, 0, 0), tracks: bool = True,
                    frusta="current", workspace_bytes: int = WORKSPACE_BYTES) -> Dict[str, torch.Tensor]:
    """V views of the reconstruction ``rec`` (reconstruct_4d's result: T frames of hw pixels) as device tensors:

    image [V, Ho, Wo, 3] uint8, depth [V, Ho, Wo] float32 (camera z of what is seen, +inf where nothing is), index [V, Ho, Wo]
    int32 (the winner's local index: dense pixel i < hw, trail point hw + j, ``MESH_BIT | frame << 4 | triangle`` as a negative
    int for a frustum triangle, -1 where nothing is).

    cam_T_world [V, 4, 4] (anything torch.as_tensor takes; used in f32), intrinsics (fx, fy, cx, cy) shared or [V, 4],
    size = (Ho, Wo), frames [V] ints: view v shows frame frames[v].  point_size is in world units, max_half caps a splat at
    (2 max_half + 1)^2 pixels, points nearer than ``near`` are dropped.  tracks=False leaves the trail points out; frusta: see
    ``frusta_stride``.  Views are rendered in chunks whose 64-bit z-buffer stays within workspace_bytes (at least one view per
    chunk); the result does not depend on the chunking.  No host synchronisation: all sizes are static."""
    pts, col = rec["points"], rec["colors"]
    dev = pts.device
    assert dev.type == "cuda", "render_4d_views runs on the GPU"
    Ho, Wo = int(size[0]), int(size[1])
    if tuple(pts.shape) != (T * hw, 3) or tuple(col.shape) != (T * hw, 3) or pts.dtype != torch.float32 or col.dtype != torch.uint8:
        raise ValueError(f"render_4d_views: rec['points'] / rec['colors'] are {tuple(pts.shape)} {pts.dtype} / {tuple(col.shape)} "
                         f"{col.dtype}, expected [{T * hw}, 3] float32 / uint8")
    M = _f32(cam_T_world, dev)
    if M.dim() != 3 or tuple(M.shape[1:]) != (4, 4):
        raise ValueError(f"render_4d_views: cam_T_world is {tuple(M.shape)}, expected [V, 4, 4]")
    V = M.shape[0]
    K = _f32(intrinsics, dev)
    if K.numel() == 4:
        K = K.reshape(1, 4).expand(V, 4).contiguous()
    if tuple(K.shape) != (V, 4):
        raise ValueError(f"render_4d_views: intrinsics are {tuple(K.shape)}, expected (fx, fy, cx, cy) or [{V}, 4]")
    fr = torch.as_tensor(frames).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(fr.shape) != (V,):
        raise ValueError(f"render_4d_views: frames is {tuple(fr.shape)}, expected [{V}]")
    stride = frusta_stride(frusta)
    bg = [int(c) for c in background]
    txyz = tcol = off = None
    n_track = 0
    if tracks and "track_xyz" in rec and rec["track_xyz"].shape[0] > 0:
        txyz, tcol, off = rec["track_xyz"].contiguous(), rec["track_colors"].contiguous(), rec["track_offsets"].contiguous()
        n_track = txyz.shape[0]
        if (txyz.dtype, tcol.dtype, off.dtype) != (torch.float32, torch.uint8, torch.int64) or off.numel() < T + 1 or \
                tuple(tcol.shape) != (n_track, 3) or txyz.dim() != 2 or txyz.shape[1] != 3:
            raise ValueError("render_4d_views: rec['track_xyz'] [P, 3] float32, rec['track_colors'] [P, 3] uint8 and "
                             f"rec['track_offsets'] [>= {T + 1}] int64 are expected")
    frustum = rec["frustum"].contiguous() if stride >= 0 else None
    if frustum is not None and (tuple(frustum.shape) != (T, 8, 3) or frustum.dtype != torch.float32):
        raise ValueError(f"render_4d_views: rec['frustum'] is {tuple(frustum.shape)} {frustum.dtype}, expected [{T}, 8, 3] float32")
    pts, col = pts.contiguous(), col.contiguous()
    lib, st = _lib.load(), _stream()
    image = torch.empty(V, Ho, Wo, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(V, Ho, Wo, dtype=torch.float32, device=dev)
    index = torch.empty(V, Ho, Wo, dtype=torch.int32, device=dev)
    chunk = max(1, min(V, int(workspace_bytes) // (8 * Ho * Wo)))
    zbuf = torch.empty(chunk, Ho, Wo, dtype=torch.int64, device=dev)
    for a in range(0, V, chunk):
        n = min(chunk, V - a)
        Mc, Kc, fc = M[a:a + n], K[a:a + n], fr[a:a + n]
        _lib.check(lib.l4p_view_splat(st, _p(pts), _p(txyz), _p(off), T, hw, n_track, _p(Mc), _p(Kc), _p(fc), n, Ho, Wo,
                                      float(point_size), int(max_half), float(near), _p(zbuf)), "l4p_view_splat")
        if frustum is not None:
            _lib.check(lib.l4p_view_mesh(st, _p(frustum), T, _p(Mc), _p(Kc), _p(fc), n, Ho, Wo, stride, float(near), _p(zbuf)),
                       "l4p_view_mesh")
        _lib.check(lib.l4p_view_resolve(st, _p(zbuf), _p(col), _p(tcol), _p(off), T, hw, n_track, _p(fc), n, Ho, Wo, bg[0], bg[1],
                                        bg[2], _p(image[a:a + n]), _p(depth[a:a + n]), _p(index[a:a + n])), "l4p_view_resolve")
    return {"image": image, "depth": depth, "index": index}


def _tz(d: float) -> np.ndarray:
    m = np.eye(4)
    m[2, 3] = d
    return m


def _ry(a: float) -> np.ndarray:
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


def _rx(a: float) -> np.ndarray:
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    return m


def view_frames(T: int, n_views: int) -> np.ndarray:
    """The frame of each view: floor(v T / V)."""
    return (np.arange(n_views, dtype=np.int64) * T) // n_views


def orbit_path(world_T_cam: np.ndarray, d0: float, n_views: int, anchor: str = "first", yaw: float = 0.6, pitch: float = 0.25,
               pull_back: float = 0.5) -> Dict[str, np.ndarray]:
    """The camera path of ``orbit_views`` from host values: world_T_cam float64 [T, 4, 4], d0 the distance of the look-at point.

    View v of V shows frame f_v = floor(v T / V), from the pose (camera to world)
        world_T_cam[a_v] . Tz(d0) . Ry(phi_v) . Rx(psi_v) . Tz(-d0 (1 + pull_back)),
    a_v = 0 for anchor "first" (a static world camera: the estimated camera's frustum is seen moving, as one uses the viewer),
    a_v = f_v for "follow".  phi_v = yaw sin(2 pi v / V), psi_v = pitch sin(4 pi v / V): a figure of eight around the look-at point
    world_T_cam[a_v] . (0, 0, d0), which stays on the optical axis at distance d0 (1 + pull_back).  With yaw = pitch = pull_back
    = 0 the poses are the estimated cameras world_T_cam[a_v].  Returns cam_T_world [V, 4, 4] float64 (the inverses), frames [V]
    int64, look_at [V, 3] float64."""
    if anchor not in ("first", "follow"):
        raise ValueError(f"anchor is 'first' or 'follow', not {anchor!r}")
    W = np.asarray(world_T_cam, dtype=np.float64)
    T, V = W.shape[0], int(n_views)
    frames = view_frames(T, V)
    cams, look = np.empty((V, 4, 4)), np.empty((V, 3))
    for v in range(V):
        s = v / V
        base = W[0 if anchor == "first" else frames[v]]
        phi, psi = yaw * math.sin(2 * math.pi * s), pitch * math.sin(4 * math.pi * s)
        pose = base @ _tz(d0) @ _ry(phi) @ _rx(psi) @ _tz(-d0 * (1 + pull_back))
        cams[v] = np.linalg.inv(pose)
        look[v] = (base @ np.array([0.0, 0.0, d0, 1.0]))[:3]
    return {"cam_T_world": cams, "frames": frames, "look_at": look}


def orbit_views(rec: Dict[str, torch.Tensor], depth_est: torch.Tensor, T: int, n_views: int, anchor: str = "first", yaw: float = 0.6,
                pitch: float = 0.25, pull_back: float = 0.5) -> Dict[str, np.ndarray]:
    """A camera path around the scene, computed on the host in float64 (``orbit_path`` documents it) from rec["world_T_cam"] and
    d0 = the lower median (torch.median) of the finite positive depths of frame 0 of depth_est [1, 1, T, H, W]: one median on the
    device and one read-back (the T poses and d0 together).  Adds "d0" to orbit_path's result."""
    d = depth_est.reshape(-1, *depth_est.shape[-2:])[0].reshape(-1).to(torch.float32)
    good = d[torch.isfinite(d) & (d > 0)]
    if good.numel() == 0:
        raise ValueError("orbit_views: frame 0 has no finite positive depth")
    wtc = rec["world_T_cam"].to(torch.float32).reshape(16, T)
    host = torch.cat([wtc.reshape(-1), torch.median(good).reshape(1)]).cpu().numpy().astype(np.float64)
    W = host[:16 * T].reshape(4, 4, T).transpose(2, 0, 1)
    res = orbit_path(W, float(host[-1]), n_views, anchor, yaw, pitch, pull_back)
    res["d0"] = float(host[-1])
    return res


def scaled_intrinsics(K44: np.ndarray, hw_in: Tuple[int, int], size: Tuple[int, int]) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of a pinhole K (pixel index = integer coordinate) for an image resized from hw_in = (H, W) to size =
    (Ho, Wo): focal lengths scale with the size, pixel centres map to pixel centres (c + 0.5 scales)."""
    sy, sx = size[0] / hw_in[0], size[1] / hw_in[1]
    return (float(K44[0, 0]) * sx, float(K44[1, 1]) * sy, (float(K44[0, 2]) + 0.5) * sx - 0.5, (float(K44[1, 2]) + 0.5) * sy - 0.5)


def generate_4D_video(batch, out, tasks, out_path: Optional[str], n_views: Optional[int] = None, size: Tuple[int, int] = (480, 640),
                      intrinsics: Union[None, Sequence[float]] = None, anchor: str = "first", yaw: float = 0.6, pitch: float = 0.25,
                      pull_back: float = 0.5, **kw) -> Tuple[np.ndarray, Optional[str]]:
    """The viewer's replacement end to end: reconstruct_4d -> orbit_views -> render_4d_views -> vis2d.write_video.  n_views
    defaults to the number of frames; the output intrinsics default to the camray head's K of frame 0 resized to ``size``
    (``scaled_intrinsics``); further keywords go to render_4d_views.  Returns (frames uint8 [V, Ho, Wo, 3] on the host, the name
    of what was written: <out_path>/<seq_name>_4d.mp4 where mediapy is importable, else the directory <out_path>/<seq_name>_4d of
    PNG frames; None without out_path)."""
    _, _, T, H, W = batch["rgb_b3thw"].shape
    rec = reconstruct_4d(batch, out, tasks)
    path = orbit_views(rec, out["depth_est_b1thw"], T, T if n_views is None else int(n_views), anchor, yaw, pitch, pull_back)
    if intrinsics is None:
        K = out["traj3d_intrinsics_est_b16t"].reshape(4, 4, T)[:, :, 0].float().cpu().numpy().astype(np.float64)
        intrinsics = scaled_intrinsics(K, (H, W), size)
    res = render_4d_views(rec, T, H * W, path["cam_T_world"], intrinsics, size, path["frames"], tracks="track_2d" in tasks, **kw)
    frames_u8 = res["image"].cpu().numpy()
    name = vis2d.write_video(frames_u8, out_path, batch["seq_name"][0] + "_4d") if out_path is not None else None
    return frames_u8, name
