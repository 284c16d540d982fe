"""Plain torch / numpy restatement of the 2D result video (l4p_amd/utils/vis2d.py, csrc/vis2d.hip), always on the host.

The dense panels follow the reference's generate_video_visualizations (l4p/utils/vis.py:34-104 with :227-428) type by type: torch
f32 for RGB, depth and mask, numpy float64 for the flow panel from its clip on (NumPy 2 promotion: np.clip of a float32 array
with np.float64 bounds is float64).  The track panel follows the reference's ordering (vis.py:434-523) with the project's own
coverage rules in place of cv2's (stated at raster_segment / raster_disc).  ``expand_calls`` turns a display list into the
sequence of cv2 calls the reference makes, which tests/golden/vis2d_T24.npz records from the reference itself
(tools/gen_golden_vis2d.py).  The fixture's scene (make_scene) lives here too."""
from __future__ import annotations

import numpy as np
import torch

from l4p_amd.utils.recon4d import hsv_index, hsv_table
from l4p_amd.utils.vis2d import MASK_THR, MAX_FLOW_MAG, TRACK_VIS_THR, TRACKS_LEAVE_TRACE, colorwheel, panel_slots, turbo_table

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TASKS = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]
LINE, BLEND, CIRCLE = 0, 1, 2
F = np.float32


def make_scene(T=24, H=48, W=48, N=12, seed=0, ties=False):
    """A small seeded scene stored as small integers: rgb = (u8 - 128) / 64, depth = (u8 - 8) / 32 (some values <= 0, the smallest
    positive one below 0.05), flow = i16 / 8 (magnitudes on both sides of 25), mask logit = i8 / 16 (none within 1e-3 of
    logit(0.85) = 1.7346), visibility logit = i16 / 256 (never 0), estimated tracks = i32 / 4 (quarter pixels: exact .5 ties for the
    rounding), key_y = the batch trajectory's distinct y at frame 0 (pairwise tied with ties=True).  Track 3 leaves the image to the
    right, track 5 has an invisible stretch."""
    g = np.random.default_rng(seed)
    rgb_u8 = g.integers(0, 256, size=(3, T, H, W), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 90 + 70 * np.sin(xx / 7.0)[None] + 60 * np.cos(yy / 5.0 + np.arange(T)[:, None, None] / 9.0)
    depth_q = np.clip(np.round(base + g.integers(-8, 9, size=(T, H, W))), 0, 255).astype(np.uint8)
    ang = (xx / 9.0 + yy / 11.0)[None] + np.arange(T)[:, None, None] / 5.0
    mag = 170 + 150 * np.sin(yy / 6.0)[None] * np.cos(np.arange(T)[:, None, None] / 4.0)  # eighths of a pixel: 2.5 .. 40
    flow_q = np.stack([mag * np.cos(ang), mag * np.sin(ang)]) + g.integers(-6, 7, size=(2, T, H, W))
    flow_q = np.round(flow_q).astype(np.int16)
    flow_q[:, 0, :4, :4] = 0  # zero flow: the centre of the wheel
    mask_q = np.clip(np.round(40 * np.sin(xx / 5.0 + np.arange(T)[:, None, None] / 3.0) + g.integers(-20, 21, size=(T, H, W))), -127,
                     127).astype(np.int8)
    ts = np.arange(T)
    x0 = g.uniform(3, W - 4, N)
    y0 = np.linspace(2.3, H - 3.1, N)[g.permutation(N)]
    tx = x0[:, None] + 0.011 * W * ts[None] * g.uniform(-1, 1, N)[:, None] + g.uniform(-0.7, 0.7, (N, T))
    ty = y0[:, None] + 0.008 * H * ts[None] * g.uniform(-1, 1, N)[:, None] + g.uniform(-0.7, 0.7, (N, T))
    if N > 3:
        tx[3] = x0[3] + (W / 14.0) * ts  # leaves the image to the right
    traj_q = np.round(np.stack([tx, ty], axis=1) * 4).astype(np.int32)  # [N, 2, T]
    vis_q = np.round(g.normal(1.6, 2.2, size=(N, T)) * 256).astype(np.int16)
    vis_q[vis_q == 0] = 700
    if N > 5:
        vis_q[5, 4:9] = -1024  # invisible stretch
    key_y = g.permutation(N).astype(np.int32)
    if ties:
        key_y = key_y // 2
    return dict(rgb_u8=rgb_u8, depth_q=depth_q, flow_q=flow_q, mask_q=mask_q, traj_q=traj_q, vis_q=vis_q, key_y=key_y)


def scene_tensors(sc, device="cpu"):
    """(batch, out) of the engine / the reference from make_scene's arrays."""
    _, T, H, W = sc["rgb_u8"].shape
    N = sc["traj_q"].shape[0]
    f = dict(dtype=torch.float32, device=device)
    key = torch.zeros(1, N, 2, T, **f)  # VideoDataset fills the batch's trajectory with zeros; the scene gives frame 0 a height
    key[0, :, 1, 0] = torch.from_numpy(sc["key_y"]).to(**f)
    batch = {"rgb_b3thw": ((torch.from_numpy(sc["rgb_u8"]).to(**f) - 128) / 64)[None],
             "rgb_mean_b3111": torch.tensor(MEAN, **f).reshape(1, 3, 1, 1, 1), "rgb_std_b3111": torch.tensor(STD, **f).reshape(1, 3, 1, 1, 1),
             "seq_name": ["scene"], "track_2d_traj_bn2t": key}
    out = {"depth_est_b1thw": ((torch.from_numpy(sc["depth_q"]).to(**f) - 8) / 32).reshape(1, 1, T, H, W),
           "flow_2d_backward_est_b2thw": (torch.from_numpy(sc["flow_q"]).to(**f) / 8)[None],
           "dyn_mask_est_b1thw": (torch.from_numpy(sc["mask_q"]).to(**f) / 16).reshape(1, 1, T, H, W),
           "track_2d_traj_est_bn2t": (torch.from_numpy(sc["traj_q"]).to(**f) / 4)[None],
           "track_2d_vis_est_bn1t": (torch.from_numpy(sc["vis_q"]).to(**f) / 256).reshape(1, N, 1, T)}
    return batch, out


def _cpu32(x):
    return torch.as_tensor(x).detach().to(device="cpu", dtype=torch.float32)


def restate_dense(batch, out, tasks):
    """The dense panels in their integer forms: rgb [T, H, W, 3] f32, grey [T, H, W] f32 (the track panel's background), and per
    task depth_index [T, H, W] uint8 (entry of the flipped turbo table) with depth_range (2 Python floats), flow_level
    [T, H, W, 3] uint8 with flow_rad_max, mask_bit [T, H, W] bool."""
    rgb = (_cpu32(batch["rgb_b3thw"]) * _cpu32(batch["rgb_std_b3111"]) + _cpu32(batch["rgb_mean_b3111"]))[0]
    rgb_thw3 = rgb.permute(1, 2, 3, 0)
    res = {"rgb": rgb_thw3.numpy(), "grey": torch.mean(rgb_thw3, dim=-1).numpy()}
    if "depth" in tasks:
        d = _cpu32(out["depth_est_b1thw"])[0, 0]
        pos = d[d > 0]
        if pos.numel() == 0:
            res["depth_range"], res["depth_index"] = (float("nan"), float("nan")), None
        else:
            vmin, vmax = max(pos.min().item(), 0.05), min(pos.max().item(), 20.0)
            dc = torch.clamp(d, min=vmin, max=vmax)
            norm = (dc - vmin) / ((vmax - vmin) * 1.05)
            res["depth_range"], res["depth_index"] = (vmin, vmax), torch.clamp(norm * 255, 0, 255).byte().numpy()
    if "flow_2d_backward" in tasks:
        fl = _cpu32(out["flow_2d_backward_est_b2thw"])[0]
        rad_max = torch.max(torch.sqrt(torch.square(fl[0]) + torch.square(fl[1]))).item()
        rad_max = min(MAX_FLOW_MAG, rad_max)
        clip = rad_max / np.sqrt(2)  # np.float64
        uv = np.clip(fl.numpy(), -clip, clip).astype(np.float64)  # float64 under NumPy 2 promotion; stated, not relied on
        u, v = uv[0] / (rad_max + 1e-5), uv[1] / (rad_max + 1e-5)
        rad = np.sqrt(np.square(u) + np.square(v))
        fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
        k0 = np.floor(fk).astype(np.int32)
        k1 = k0 + 1
        k1[k1 == 55] = 0
        f = fk - k0
        wheel = colorwheel()
        level = np.zeros(u.shape + (3,), np.uint8)
        for c in range(3):
            col = (1 - f) * (wheel[k0, c] / 255.0) + f * (wheel[k1, c] / 255.0)
            col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
            level[..., c] = np.floor(255 * col)
        res["flow_rad_max"], res["flow_level"] = rad_max, level
    if "dyn_mask" in tasks:
        res["mask_bit"] = (torch.sigmoid(_cpu32(out["dyn_mask_est_b1thw"])[0, 0]) > MASK_THR).numpy()
    return res


def display_list(batch, out):
    """(order [N], xy [T, N, 2] int, vis [T, N] bool, colors float64 [N, 3]): tracks in the stable order of the batch trajectory's y
    at frame 0, estimates rounded half to even, sigmoid > 0.5 (and finite), matplotlib hsv of rank / (N - 1)."""
    order = torch.argsort(_cpu32(batch["track_2d_traj_bn2t"])[0, :, 1, 0], stable=True).numpy()
    traj = _cpu32(out["track_2d_traj_est_bn2t"])[0].numpy()[order]  # [N, 2, T]
    N = traj.shape[0]
    finite = np.isfinite(traj).all(axis=1)
    xy = np.clip(np.rint(np.where(np.isfinite(traj), traj, 0)), -2.0 ** 30, 2.0 ** 30).astype(np.int64).transpose(2, 0, 1)
    vis = (torch.sigmoid(_cpu32(out["track_2d_vis_est_bn1t"])[0, :, 0]) > TRACK_VIS_THR).numpy()[order] & finite
    colors = hsv_table()[hsv_index(np.arange(N), N)] if N else np.zeros((0, 3))
    return order, xy * finite.T[:, :, None], vis.T.copy(), colors


def expand_calls(xy, vis, colors, trail=TRACKS_LEAVE_TRACE):
    """The reference's cv2 call sequence for a display list (plot_2d_tracks, vis.py:489-521): kinds, points [K, 4], colours
    [K, 3], weights [K, 2]."""
    T, N = vis.shape
    kinds, pts, cols, wts = [], [], [], []
    for t in range(T):
        t0 = max(0, t - trail)
        for s in range(t - t0):
            for i in np.nonzero(vis[t0 + s] & vis[t0 + s + 1])[0]:
                kinds.append(LINE), pts.append([*xy[t0 + s, i], *xy[t0 + s + 1, i]]), cols.append(colors[i]), wts.append([0, 0])
            alpha = (s + 1) / (t - t0)
            kinds.append(BLEND), pts.append([0, 0, 0, 0]), cols.append([0, 0, 0]), wts.append([alpha, 1 - alpha])
        for i in np.nonzero(vis[t])[0]:
            kinds.append(CIRCLE), pts.append([*xy[t, i], 0, 0]), cols.append(colors[i]), wts.append([0, 0])
    return (np.array(kinds, np.int8), np.array(pts, np.int64).reshape(-1, 4), np.array(cols, np.float64).reshape(-1, 3),
            np.array(wts, np.float64).reshape(-1, 2))


def raster_segment(img, x1, y1, x2, y2, col):
    """The segment rule on img [H, W, 3] f32, in place: with d the Euclidean distance from the pixel centre to the segment,
    c = clamp(1 - d, 0, 1) and img = (1 - c) img + c col where c > 0.  f32, unfused, in this order: q = p - p1 and e = p2 - p1 as
    integers, then u = clamp((qx ex + qy ey) / (ex ex + ey ey), 0, 1) (0 for a zero-length segment), r = q - u e,
    d = sqrt(rx rx + ry ry).  Only the bounding box grown by one is visited: beyond it d >= 2."""
    H, W = img.shape[:2]
    xa, xb = max(min(x1, x2) - 1, 0), min(max(x1, x2) + 1, W - 1)
    ya, yb = max(min(y1, y2) - 1, 0), min(max(y1, y2) + 1, H - 1)
    if xa > xb or ya > yb:
        return
    qx = (np.arange(xa, xb + 1) - x1).astype(F)[None, :]
    qy = (np.arange(ya, yb + 1) - y1).astype(F)[:, None]
    ex, ey = F(x2 - x1), F(y2 - y1)
    len2 = ex * ex + ey * ey
    if len2 != 0:
        u = np.minimum(np.maximum((qx * ex + qy * ey) / len2, F(0)), F(1))
    else:
        u = np.zeros((qy.shape[0], qx.shape[1]), F)
    rx, ry = qx - u * ex, qy - u * ey
    c = np.minimum(np.maximum(F(1) - np.sqrt(rx * rx + ry * ry), F(0)), F(1))[..., None]
    sub = img[ya:yb + 1, xa:xb + 1]
    sub[...] = np.where(c > 0, (F(1) - c) * sub + c * col, sub)


def raster_disc(img, x, y, col):
    """The end point: pixels with dx^2 + dy^2 <= 5 take the colour (21 pixels in rows of 3, 5, 5, 5, 3), clipped to the frame."""
    H, W = img.shape[:2]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx * dx + dy * dy <= 5 and 0 <= x + dx < W and 0 <= y + dy < H:
                img[y + dy, x + dx] = col


def raster_frame(grey_hw, t, xy, vis, colors, trail=TRACKS_LEAVE_TRACE):
    """Frame t of the track panel [H, W, 3] f32 from its grey background and the display list: for each trail step s the segments
    in ascending rank, then img = f32(alpha) img + f32(1 - alpha) start-of-step (alpha = (s + 1) / (L - 1) in double); the discs
    last."""
    col32 = np.asarray(colors, np.float64).astype(F)
    img = np.repeat(np.asarray(grey_hw, F)[..., None], 3, axis=-1)
    t0 = max(0, t - trail)
    for s in range(t - t0):
        start = img.copy()
        for i in np.nonzero(vis[t0 + s] & vis[t0 + s + 1])[0]:
            raster_segment(img, int(xy[t0 + s, i, 0]), int(xy[t0 + s, i, 1]), int(xy[t0 + s + 1, i, 0]), int(xy[t0 + s + 1, i, 1]),
                           col32[i])
        alpha = (s + 1) / (t - t0)
        img = F(alpha) * img + F(1 - alpha) * start
    for i in np.nonzero(vis[t])[0]:
        raster_disc(img, int(xy[t, i, 0]), int(xy[t, i, 1]), col32[i])
    return img


def restate(batch, out, tasks, track_frames=None):
    """Everything render_video_panels returns, as numpy: video [T, H, P W, 3] f32 plus the scalars and the display list.
    track_frames: the frames of the track panel to rasterise (default all); the others keep the grey background."""
    dense = restate_dense(batch, out, tasks)
    T, H, W, _ = dense["rgb"].shape
    slots = panel_slots(tasks)
    video = np.zeros((T, H, (1 + len(slots)) * W, 3), F)
    video[:, :, :W] = dense["rgb"]
    res = {"video": video}
    for task, p in slots.items():
        panel = video[:, :, p * W:(p + 1) * W]
        if task == "depth":
            res["depth_range"] = np.array(dense["depth_range"], np.float64)
            if dense["depth_index"] is not None:
                panel[...] = turbo_table()[::-1].astype(F)[dense["depth_index"]]
            res["depth_index"] = dense["depth_index"]
        elif task == "flow_2d_backward":
            res["flow_rad_max"] = np.array([dense["flow_rad_max"]], np.float64)
            panel[...] = dense["flow_level"].astype(F) / F(255)
            res["flow_level"] = dense["flow_level"]
        elif task == "dyn_mask":
            panel[...] = dense["mask_bit"].astype(F)[..., None]
        else:
            order, xy, vis, colors = display_list(batch, out)
            res.update(track_order_n=order, track_xy_tn2=xy, track_vis_tn=vis, track_colors_n3=colors)
            panel[...] = dense["grey"][..., None]
            for t in (range(T) if track_frames is None else track_frames):
                panel[t] = raster_frame(dense["grey"][t], t, xy, vis, colors)
    return res
