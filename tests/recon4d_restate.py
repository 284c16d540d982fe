"""Plain-torch restatement of the reference's 4D reconstruction (l4p/utils/vis.py:107-221 with vis.py:621-766 and
geometry_utils.py:13-143, traj3d branch), f32 as the reference computes on the device (float64 where it computes in numpy).
Used by tests/test_recon4d_cpu.py (against the reference's own output, tests/golden/recon4d_T24.npz) and by the GPU tests as
the yardstick of l4p_amd.utils.recon4d on inputs the fixture does not cover.

The synthetic scene of the fixture (make_scene) lives here too: tools/gen_golden_recon4d.py feeds it to the reference."""
from __future__ import annotations

import math

import numpy as np
import torch

from l4p_amd.utils.recon4d import (FRUSTUM_FAR, FRUSTUM_FOV, FRUSTUM_NEAR, SEGMENT_POINTS, TRACKS_LEAVE_TRACE, VIS_THR, colour_bytes,
                                   frustum_camera_vertices, hsv_index, hsv_table)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_scene(T=24, H=32, W=32, N=10, seed=0, depth_scale=2.0):
    """A small well-posed seeded scene: a camera moving along a smooth path with small rotations, pinhole K, smooth positive depth,
    N tracks (some invisible frames, one leaving the image), track depths off by 1 / depth_scale.  Every float is exactly
    representable from the stored integers, so the fixture needs only these numpy arrays."""
    g = np.random.default_rng(seed)
    rgb_u8 = g.integers(0, 256, size=(1, 3, T, H, W), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 64 + 40 * np.sin(xx / 7.0)[None] + 30 * np.cos(yy / 5.0 + np.arange(T)[:, None, None] / 9.0)
    depth_q = np.clip(np.round(base + g.integers(-8, 9, size=(T, H, W))), 1, 255).astype(np.uint8)  # depth = 1 + q / 64
    poses = np.zeros((16, T), dtype=np.float32)
    for t in range(T):
        a, b = 0.02 * t, 0.015 * math.sin(t / 4)
        ca, sa, cb, sb = math.cos(a), math.sin(a), math.cos(b), math.sin(b)
        R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, [0.05 * t, 0.02 * math.sin(t / 3), 0.03 * t]
        poses[:, t] = M.reshape(16)
    K = np.zeros((16, T), dtype=np.float32)
    K[0], K[5], K[2], K[6], K[10], K[15] = 30.0, 28.0, 15.5, 16.0, 1.0, 1.0
    # tracks: start at distinct y, drift; track 3 leaves the image to the right
    x0 = g.uniform(2, 29, N)
    y0 = np.sort(g.permutation(np.linspace(1.3, 30.1, N) + g.uniform(-0.4, 0.4, N)))[g.permutation(N)]
    ts = np.arange(T)
    tx = x0[:, None] + 0.35 * ts[None] * g.uniform(-1, 1, N)[:, None]
    ty = y0[:, None] + 0.25 * ts[None] * g.uniform(-1, 1, N)[:, None]
    if N > 3:
        tx[3] = x0[3] + 1.6 * ts
    traj = np.stack([tx, ty], axis=1).astype(np.float32)  # [N, 2, T]
    logit = g.normal(2.0, 2.5, size=(N, T)).astype(np.float32)
    logit[np.abs(logit - np.float32(math.log(3))) < 2e-3] += 0.01  # nothing within 1e-3 of the threshold
    if N > 5:
        logit[5, 4:9] = -4.0  # invisible stretch
    ix = np.clip(np.round(tx), 0, W - 1).astype(int)
    iy = np.clip(np.round(ty), 0, H - 1).astype(int)
    dtrue = 1.0 + depth_q[ts[None].repeat(N, 0), iy, ix].astype(np.float32) / 64
    tdepth = (dtrue / depth_scale * g.uniform(0.97, 1.03, size=(N, T))).astype(np.float32)
    return dict(rgb_u8=rgb_u8, depth_q=depth_q, poses=poses, K=K, traj=traj, vis_logit=logit, track_depth=tdepth)


def scene_tensors(sc, device="cpu"):
    """(batch, out) of the engine / the reference from make_scene's arrays."""
    T, H, W = sc["depth_q"].shape
    N = sc["traj"].shape[0]
    f = dict(dtype=torch.float32, device=device)
    rgb = (torch.from_numpy(sc["rgb_u8"]).to(**f) - 128) / 64  # exact
    batch = {"rgb_b3thw": rgb, "rgb_mean_b3111": torch.tensor(MEAN, **f).reshape(1, 3, 1, 1, 1),
             "rgb_std_b3111": torch.tensor(STD, **f).reshape(1, 3, 1, 1, 1), "seq_name": ["scene"],
             "intrinsics_b44t": torch.eye(4, **f)[None, :, :, None].repeat(1, 1, 1, T)}
    out = {"depth_est_b1thw": (1 + torch.from_numpy(sc["depth_q"]).to(**f) / 64).reshape(1, 1, T, H, W),
           "traj3d_est_b16t": torch.from_numpy(sc["poses"]).to(**f)[None],
           "traj3d_intrinsics_est_b16t": torch.from_numpy(sc["K"]).to(**f)[None],
           "track_2d_traj_est_bn2t": torch.from_numpy(sc["traj"]).to(**f)[None],
           "track_2d_vis_est_bn1t": torch.from_numpy(sc["vis_logit"]).to(**f).reshape(1, N, 1, T),
           "track_2d_depth_est_bn1t": torch.from_numpy(sc["track_depth"]).to(**f).reshape(1, N, 1, T)}
    return batch, out


def nearest_index(coord: torch.Tensor, size: int) -> torch.Tensor:
    """grid_sample(mode="nearest", align_corners=False) after the reference's normalisation by (size - 1): the source index
    ((g + 1) size - 1) / 2, g = c / (size - 1) * 2 - 1, each op rounded in f32, rounded half to even."""
    g = coord / (size - 1) * 2 - 1
    return torch.round(((g + 1) * size - 1) / 2)


def restate(batch, out, tasks):
    """The reference's geometry in plain torch on out's device (host numpy for the float64 parts).  Returns numpy arrays keyed as
    l4p_amd.utils.recon4d.reconstruct_4d's output."""
    _, _, T, H, W = batch["rgb_b3thw"].shape
    dev = out["depth_est_b1thw"].device
    f32 = lambda x: x.to(device=dev, dtype=torch.float32)  # noqa: E731
    M = f32(out["traj3d_est_b16t"]).permute(0, 2, 1).reshape(1, T, 4, 4)
    cam_T_world = torch.linalg.inv(M)
    cam_T_ref = torch.matmul(cam_T_world, torch.linalg.inv(cam_T_world[:, :1]))  # [1, T, 4, 4]
    world_T_cam = torch.linalg.inv(cam_T_ref)
    K = f32(out["traj3d_intrinsics_est_b16t"]).reshape(1, 4, 4, T).permute(0, 3, 1, 2)[0]  # [T, 4, 4]
    # dense
    depth = f32(out["depth_est_b1thw"])[0, 0]  # [T, H, W]
    j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    pix = torch.stack([i, j, torch.ones_like(i)], 0).reshape(3, H * W)
    cam = torch.matmul(torch.linalg.inv(K[:, :3, :3]), pix) * depth.reshape(T, 1, H * W)  # [T, 3, HW]
    P = world_T_cam[0]
    pts = torch.matmul(P[:, :3, :3], cam) + P[:, :3, 3:]
    rgb = f32(batch["rgb_b3thw"]) * f32(batch["rgb_std_b3111"]) + f32(batch["rgb_mean_b3111"])
    res = {"points": pts.permute(0, 2, 1).reshape(-1, 3).cpu().numpy(),
           "colors": colour_bytes(rgb[0].permute(1, 2, 3, 0).reshape(-1, 3).cpu().numpy()),
           "cam_T_ref": cam_T_ref.permute(0, 2, 3, 1).cpu().numpy(), "world_T_cam": world_T_cam.permute(0, 2, 3, 1).cpu().numpy()}
    wtc = np.linalg.inv(cam_T_ref[0].cpu().numpy().astype(np.float64))
    v = frustum_camera_vertices()
    res["frustum"] = (np.concatenate([v, np.ones((8, 1))], 1)[None] @ wtc.transpose(0, 2, 1))[..., :3]
    if "track_2d" not in tasks:
        return res
    tr = f32(out["track_2d_traj_est_bn2t"])[0]  # [N, 2, T]
    vis = torch.sigmoid(f32(out["track_2d_vis_est_bn1t"])[0, :, 0]) > VIS_THR  # [N, T]
    tdep = f32(out["track_2d_depth_est_bn1t"])[0, :, 0]
    N = tr.shape[0]
    ix, iy = nearest_index(tr[:, 0], W), nearest_index(tr[:, 1], H)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    tt = torch.arange(T, device=dev)[None].expand(N, T)
    samp = torch.where(inside, depth[tt, iy.clamp(0, H - 1).long(), ix.clamp(0, W - 1).long()], torch.zeros_like(tdep))
    ratios = (samp / tdep)[vis]
    scale = torch.median(ratios) if ratios.numel() else torch.tensor(float("nan"), device=dev)
    order = torch.argsort(tr[:, 1, 0], stable=True)
    Z = scale * tdep[order]
    trs = tr[order]
    X = (trs[:, 0] - K[:, 0, 2]) * Z / K[:, 0, 0]
    Y = (trs[:, 1] - K[:, 1, 2]) * Z / K[:, 1, 1]
    cam3 = torch.stack([X, Y, Z], 1)  # [N, 3, T]
    Xw = (torch.einsum("tij,njt->nit", P[:, :3, :3], cam3) + P[:, :3, 3].T[None]).cpu().numpy()  # [N, 3, T]
    vis_s = vis[order].cpu().numpy()
    lut = colour_bytes(hsv_table())[hsv_index(np.arange(N), N)]  # [N, 3]
    alpha = np.linspace(0, 1, SEGMENT_POINTS)
    xyz, col, counts, off = [], [], [], [0]
    for t in range(T):
        sel = np.nonzero(vis_s[:, t])[0]
        L = min(t, TRACKS_LEAVE_TRACE)
        Xt = Xw[sel].transpose(0, 2, 1)  # [nv, T, 3]
        if L == 0:
            p = Xt[:, t:t + 1].astype(np.float64)
        else:
            start, stop = Xt[:, t - L:t], Xt[:, t - L + 1:t + 1]
            p = start[:, :, None] + (stop - start)[:, :, None] * alpha[None, None, :, None]
        per = 1 if L == 0 else L * SEGMENT_POINTS
        xyz.append(p.reshape(-1, 3).astype(np.float32))
        col.append(np.repeat(lut[sel], per, axis=0))
        counts.append(len(sel))
        off.append(off[-1] + len(sel) * per)
    res.update(scale=scale.reshape(1).cpu().numpy(), track_order=order.cpu().numpy(), track_points_bn3t=Xw[None],
               track_counts=np.array(counts), track_offsets=np.array(off), track_xyz=np.concatenate(xyz),
               track_colors=np.concatenate(col))
    return res


def extent(a: np.ndarray) -> float:
    return float(np.abs(a).max())
