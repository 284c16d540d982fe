"""4D reconstruction on the GPU: the reference's generate_4D_visualization (l4p/utils/vis.py:107-221, traj3d branch) on the
engine's outputs — per-frame world point clouds of every pixel, 3D track trails and the camera path as frusta — with every
stage in csrc/recon4d.hip, and the reference's PLY files.

``reconstruct_4d`` returns device tensors; ``generate_4D_visualization`` has the reference's signature, assertions, side effect
(``batch["intrinsics_b44t"]`` is overwritten with the camray head's intrinsics), file names and return value, so the reference's
viser viewer can consume its list unchanged.  The module is not named ``vis``: ``l4p.utils.vis`` (the 2D visualisations, cv2 /
mediapy / open3d) stays out of the engine.
"""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream

VIS_THR = 0.75  # vis.py:147
TRACKS_LEAVE_TRACE = 16  # vis.py:177
SEGMENT_POINTS = 20  # np.linspace(0, 1, 20), vis.py:757
# create_camera_frustum() defaults (vis.py:529-618) and its colour
FRUSTUM_FOV, FRUSTUM_NEAR, FRUSTUM_FAR, FRUSTUM_COLOUR = 45.0, 0.01, 0.65, (1.0, 0.5, 0.5)
FRUSTUM_TRIANGLES = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 3, 7], [0, 7, 4],
                              [1, 5, 6], [1, 6, 2], [0, 4, 5], [0, 5, 1], [3, 2, 6], [3, 6, 7]], dtype=np.int32)

# matplotlib's "hsv" colormap: its published segment data (x, y0, y1) per channel
_HSV_DATA = {
    "red": ((0.0, 1.0, 1.0), (0.15873, 1.0, 1.0), (0.174603, 0.96875, 0.96875), (0.333333, 0.03125, 0.03125),
            (0.349206, 0.0, 0.0), (0.666667, 0.0, 0.0), (0.68254, 0.03125, 0.03125), (0.84127, 0.96875, 0.96875),
            (0.857143, 1.0, 1.0), (1.0, 1.0, 1.0)),
    "green": ((0.0, 0.0, 0.0), (0.15873, 0.9375, 0.9375), (0.174603, 1.0, 1.0), (0.507937, 1.0, 1.0),
              (0.666667, 0.0625, 0.0625), (0.68254, 0.0, 0.0), (1.0, 0.0, 0.0)),
    "blue": ((0.0, 0.0, 0.0), (0.333333, 0.0, 0.0), (0.349206, 0.0625, 0.0625), (0.507937, 1.0, 1.0),
             (0.84127, 1.0, 1.0), (0.857143, 0.9375, 0.9375), (1.0, 0.09375, 0.09375)),
}
HSV_N = 256


def _segment_lut(data, n: int) -> np.ndarray:
    """LinearSegmentedColormap's lookup table of one channel (matplotlib.colors._create_lookup_table, gamma 1), float64."""
    a = np.asarray(data, dtype=np.float64)
    x, y0, y1 = a[:, 0] * (n - 1), a[:, 1], a[:, 2]
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def hsv_table() -> np.ndarray:
    """float64 [256, 3]: matplotlib's hsv colours, entry k = cmap(k / 256)."""
    return np.stack([_segment_lut(_HSV_DATA[c], HSV_N) for c in ("red", "green", "blue")], axis=1)


def hsv_index(i, n: int) -> np.ndarray:
    """The table entry of track i of n under cmap(Normalize(0, n - 1)(i)): float64 i / (n - 1) (0 when n = 1), times 256,
    256 -> 255, truncated (matplotlib.colors.Colormap.__call__)."""
    f = np.asarray(i, dtype=np.float64) / (n - 1) if n > 1 else np.zeros_like(np.asarray(i, dtype=np.float64))
    f = f * HSV_N
    f[f == HSV_N] = HSV_N - 1
    return f.astype(np.int64)


def colour_bytes(c) -> np.ndarray:
    """Open3D's PLY colour rule: min(255, max(0, c * 255)) in float64, truncated to uchar."""
    return np.minimum(255.0, np.maximum(0.0, np.asarray(c, dtype=np.float64) * 255.0)).astype(np.uint8)


def frustum_camera_vertices() -> np.ndarray:
    """create_camera_frustum()'s 8 vertices in the camera frame, float64 [8, 3]."""
    t = np.tan(np.radians(FRUSTUM_FOV) / 2)
    nh, fh = 2 * FRUSTUM_NEAR * t, 2 * FRUSTUM_FAR * t
    s = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64)
    near = np.concatenate([s * nh / 2, np.full((4, 1), FRUSTUM_NEAR)], axis=1)
    far = np.concatenate([s * fh / 2, np.full((4, 1), FRUSTUM_FAR)], axis=1)
    return np.concatenate([near, far], axis=0)


def frustum_normals() -> np.ndarray:
    """compute_vertex_normals() of the camera-frame frustum (area-weighted triangle normals summed per vertex, normalised), float32
    [8, 3].  The reference computes them before it moves the vertices and never again, so every frame's file carries these."""
    v = frustum_camera_vertices()
    tri = FRUSTUM_TRIANGLES
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, tri[:, k], fn)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


_LUT_CACHE: Dict[torch.device, torch.Tensor] = {}


def _lut(device) -> torch.Tensor:
    if device not in _LUT_CACHE:
        _LUT_CACHE[device] = torch.from_numpy(colour_bytes(hsv_table())).contiguous().to(device)
    return _LUT_CACHE[device]


def _f32(x, device) -> torch.Tensor:
    return torch.as_tensor(x).to(device=device, dtype=torch.float32).contiguous()


def reconstruct_4d(batch: dict, out: dict, tasks: List[str]) -> Dict[str, torch.Tensor]:
    """The geometry of generate_4D_visualization as device tensors (csrc/recon4d.hip; f32 whatever dtype the engine returned):

    points [T*H*W, 3] f32 / colors [T*H*W, 3] uint8: every pixel of every frame in world space, frame-major (vis.py:143,
        geometry_utils.py:13-53), colour rgb * std + mean by Open3D's byte rule;
    cam_T_ref, world_T_cam [1, 4, 4, T]; frustum [T, 8, 3] (vis.py:138-141, 621-641);
    with "track_2d" in tasks: scale [1] (the lower median of vis.py:167, NaN when no pair is visible), track_order [N] (tracks by
    their y at frame 0, stable), track_points_bn3t [1, N, 3, T] (scaled, world, sorted order), track_counts [T] (visible tracks
    per frame), track_offsets [T + 1] int64 (trail points of frame t: [off[t], off[t + 1])), track_xyz [P, 3] f32 /
    track_colors [P, 3] uint8 (vis.py:738-766).

    The trail sizes depend on the visibility computed on the device: the call reads the per-frame offsets back once (one
    synchronisation) to size the trail outputs and the median's rank.  Nothing else leaves the device."""
    B, _, T, H, W = batch["rgb_b3thw"].shape
    assert "depth" in tasks and "camray" in tasks, "Tasks must include depth, camray"
    assert B == 1, "Current implementation supports only batch size 1"
    if "camray_est_b6thw" in out:
        raise ValueError("reconstruct_4d: the camray_est_b6thw branch of the reference is not supported; this engine's camray head "
                         "returns traj3d_est_b16t / traj3d_intrinsics_est_b16t")
    if "traj3d_est_b16t" not in out or "traj3d_intrinsics_est_b16t" not in out:
        raise ValueError("reconstruct_4d needs out['traj3d_est_b16t'] and out['traj3d_intrinsics_est_b16t'] (the camray task)")
    dev = out["depth_est_b1thw"].device
    assert dev.type == "cuda", "reconstruct_4d runs on the GPU"
    lib, st = _lib.load(), _stream()
    traj = _f32(out["traj3d_est_b16t"], dev)
    K = _f32(out["traj3d_intrinsics_est_b16t"], dev)
    assert tuple(traj.shape) == (1, 16, T) and K.numel() == 16 * T
    res: Dict[str, torch.Tensor] = {}
    cam_T_ref = torch.empty(1, 4, 4, T, dtype=torch.float32, device=dev)
    world_T_cam = torch.empty_like(cam_T_ref)
    frustum = torch.empty(T, 8, 3, dtype=torch.float32, device=dev)
    tan_half = float(np.tan(np.radians(FRUSTUM_FOV) / 2))
    _lib.check(lib.l4p_recon_cameras(st, _p(traj), 1, T, 0, 1, tan_half, FRUSTUM_NEAR, FRUSTUM_FAR, _p(cam_T_ref), _p(world_T_cam),
                                     _p(frustum)), "l4p_recon_cameras")
    depth = _f32(out["depth_est_b1thw"], dev)
    rgb = _f32(batch["rgb_b3thw"], dev)
    mean, std = _f32(batch["rgb_mean_b3111"], dev).reshape(3), _f32(batch["rgb_std_b3111"], dev).reshape(3)
    points = torch.empty(T * H * W, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(T * H * W, 3, dtype=torch.uint8, device=dev)
    _lib.check(lib.l4p_point_map(st, _p(depth), _p(K), _p(world_T_cam), 1, T, H, W, _p(points), 3, 1, 0, _p(rgb), _p(mean), _p(std),
                                 _p(colors)), "l4p_point_map")
    res.update(points=points, colors=colors, cam_T_ref=cam_T_ref, world_T_cam=world_T_cam, frustum=frustum)
    if "track_2d" not in tasks:
        return res
    tr = _f32(out["track_2d_traj_est_bn2t"], dev)
    vis = _f32(out["track_2d_vis_est_bn1t"], dev)
    tdepth = _f32(out["track_2d_depth_est_bn1t"], dev)
    N = tr.shape[1]
    i32 = dict(dtype=torch.int32, device=dev)
    order, counts = torch.empty(N, **i32), torch.empty(T, **i32)
    xyz = torch.empty(0, 3, dtype=torch.float32, device=dev)
    rgb_t = torch.empty(0, 3, dtype=torch.uint8, device=dev)
    scale = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    X = torch.empty(1, N, 3, T, dtype=torch.float32, device=dev)
    off = torch.zeros(T + 2, dtype=torch.int64, device=dev)
    if N == 0:  # no queries: no track work at all
        counts.zero_()
    else:
        slot = torch.empty(T, N, **i32)
        ratios = torch.empty(T, N, dtype=torch.float32, device=dev)
        flag = torch.empty(1, **i32)
        _lib.check(lib.l4p_recon_track_prep(st, _p(tr), _p(vis), _p(tdepth), _p(depth), N, T, H, W, VIS_THR, TRACKS_LEAVE_TRACE,
                                            SEGMENT_POINTS, _p(order), _p(slot), _p(ratios), _p(flag), _p(counts), _p(off)),
                   "l4p_recon_track_prep")
        off_h = off.cpu()  # the one host read-back: output sizes and the median's rank
        total, nvis = int(off_h[T]), int(off_h[T + 1])
        ws = torch.empty(_lib.L4P_QUANTILE_WS_UINTS, dtype=torch.int32, device=dev)
        sel = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(lib.l4p_recon_track_scale(st, _p(ratios), N * T, nvis, _p(flag), _p(ws), _p(sel), _p(scale)),
                   "l4p_recon_track_scale")
        _lib.check(lib.l4p_track_point_map(st, _p(tr), _p(tdepth), _p(K), _p(world_T_cam), _p(scale), _p(order), 1, N, T, _p(X)),
                   "l4p_track_point_map")
        xyz = torch.empty(total, 3, dtype=torch.float32, device=dev)
        rgb_t = torch.empty(total, 3, dtype=torch.uint8, device=dev)
        _lib.check(lib.l4p_recon_trails(st, _p(X), _p(slot), _p(off), _p(_lut(dev)), N, T, TRACKS_LEAVE_TRACE, SEGMENT_POINTS, total,
                                        _p(xyz), _p(rgb_t)), "l4p_recon_trails")
    res.update(scale=scale, track_order=order, track_points_bn3t=X, track_counts=counts, track_offsets=off[:T + 1],
               track_xyz=xyz, track_colors=rgb_t)
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# PLY (binary little-endian): float x, y, z [, float nx, ny, nz], uchar red, green, blue [, face: list uchar int vertex_indices]
# ------------------------------------------------------------------------------------------------------------------------------
def _vertex_dtype(normals: bool) -> np.dtype:
    f = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        f += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    return np.dtype(f + [("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(path: str, xyz: np.ndarray, rgb: np.ndarray, normals: np.ndarray = None, faces: np.ndarray = None) -> None:
    """One PLY file: xyz float [n, 3], rgb uint8 [n, 3], optional normals float [n, 3] and triangles int [m, 3]."""
    n = int(xyz.shape[0])
    v = np.empty(n, dtype=_vertex_dtype(normals is not None))
    for k, c in enumerate("xyz"):
        v[c] = xyz[:, k]
        if normals is not None:
            v["n" + c] = normals[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        v[c] = rgb[:, k]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y",
            "property float z"]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["property uchar red", "property uchar green", "property uchar blue"]
    body = [v.tobytes()]
    if faces is not None:
        f = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        f["n"], f["i"] = 3, faces
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        body.append(f.tobytes())
    with open(path, "wb") as fh:
        fh.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        for b in body:
            fh.write(b)


def read_ply(path: str) -> Dict[str, np.ndarray]:
    """Reader for the files write_ply produces: {"xyz", "rgb"[, "normals", "faces"]}."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0", path
    n = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    normals = "property float nx" in head
    v = np.frombuffer(data, dtype=_vertex_dtype(normals), count=n, offset=end)
    res = {"xyz": np.stack([v["x"], v["y"], v["z"]], axis=1), "rgb": np.stack([v["red"], v["green"], v["blue"]], axis=1)}
    if normals:
        res["normals"] = np.stack([v["nx"], v["ny"], v["nz"]], axis=1)
    faces = [h for h in head if h.startswith("element face")]
    if faces:
        m = int(faces[0].split()[-1])
        f = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=m, offset=end + v.nbytes)
        assert (f["n"] == 3).all(), path
        res["faces"] = f["i"].copy()
    return res


def generate_4D_visualization(batch, out, tasks, out_path):
    """vis.py:107-221 on the GPU: writes {t}_world_cam_mesh.ply (the frustum) and {t}_world_track_depth_pc.ply (dense cloud, then
    the frame's trail points; "track_2d" in tasks) or {t}_world.ply (dense cloud only) under out_path/seq_name/, and returns the
    reference's list of dicts.  As the reference does, batch["intrinsics_b44t"] is overwritten with the camray head's intrinsics
    out["traj3d_intrinsics_est_b16t"] reshaped to [1, 4, 4, T]."""
    B, _, T, H, W = batch["rgb_b3thw"].shape
    assert "depth" in tasks and "camray" in tasks, "Tasks must include depth, camray"
    assert B == 1, "Current implementation supports only batch size 1"
    seq_name = batch["seq_name"][0]
    out_path = os.path.join(out_path, seq_name)
    os.makedirs(out_path, exist_ok=True)
    if "traj3d_est_b16t" in out.keys():
        batch["intrinsics_b44t"] = out["traj3d_intrinsics_est_b16t"].reshape(1, 4, 4, T)
    rec = reconstruct_4d(batch, out, tasks)
    write_4d_files(rec, seq_name, out_path, T, H * W, "track_2d" in tasks)
    return ply_list(seq_name, out_path, T, "track_2d" in tasks)


def ply_list(seq_name: str, out_path: str, T: int, tracks: bool) -> List[dict]:
    """The return value of vis.py:190-221 for files under out_path (= the reference's out_path/seq_name)."""
    res = []
    for t in range(T):
        ply = os.path.join(out_path, f"{t}_world.ply")
        cam = ply.replace(".ply", "_cam_mesh.ply")
        if tracks:
            res.append({"name": f"{seq_name}_{t}", "pc_depth_track": ply.replace(".ply", "_track_depth_pc.ply"), "mesh_cam": cam})
        else:
            res.append({"name": f"{seq_name}_{t}", "pc_depth": ply, "mesh_cam": cam})
    return res


def write_4d_files(rec: Dict[str, torch.Tensor], seq_name: str, out_path: str, T: int, hw: int, tracks: bool) -> None:
    """Copy the reconstruction to the host and write the per-frame PLY files of ply_list()."""
    pts, col = rec["points"].cpu().numpy(), rec["colors"].cpu().numpy()
    fr = rec["frustum"].cpu().numpy()
    normals = frustum_normals()
    mesh_rgb = np.repeat(colour_bytes(FRUSTUM_COLOUR)[None], 8, axis=0)
    if tracks:
        txyz, trgb = rec["track_xyz"].cpu().numpy(), rec["track_colors"].cpu().numpy()
        off = rec["track_offsets"].cpu().numpy()
    for entry, t in zip(ply_list(seq_name, out_path, T, tracks), range(T)):
        write_ply(entry["mesh_cam"], fr[t], mesh_rgb, normals=normals, faces=FRUSTUM_TRIANGLES)
        a, b = t * hw, (t + 1) * hw
        if tracks:
            s, e = int(off[t]), int(off[t + 1])
            write_ply(entry["pc_depth_track"], np.concatenate([pts[a:b], txyz[s:e]]), np.concatenate([col[a:b], trgb[s:e]]))
        else:
            write_ply(entry["pc_depth"], pts[a:b], col[a:b])
