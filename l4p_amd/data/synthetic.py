"""Seeded synthetic inputs of the benchmark and demo workloads: the 8x8 grid of track queries and a
deterministic uint8 "decoded video", plus seeded DAVIS / DyCheck directory trees (instance masks, a calibration file) for the
demo's --synthetic runs and the dataset tests.  Lives in the package so that bench.py and demo/demo.py do not depend on tests/."""
import torch


def grid_queries(nq: int) -> torch.Tensor:
    """The benchmark's track queries (bench.py): an 8x8 grid x, y in {14 + 28 i} + 0.5 at t = 0.5 -> [1,nq,3]."""
    q = torch.zeros(1, nq, 3)
    for i in range(nq):
        q[0, i] = torch.tensor([0.5, 14.0 + 28.0 * (i % 8) + 0.5, 14.0 + 28.0 * ((i // 8) % 8) + 0.5])
    return q


def synthetic_video(seed: int, T: int, H: int, W: int):
    """uint8 frames [T,H,W,3]: smooth moving gradients + blocks + noise, so every filter tap matters."""
    import numpy as np

    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None, None]
    y = np.arange(H)[None, :, None, None]
    x = np.arange(W)[None, None, :, None]
    c = np.arange(3)[None, None, None, :]
    v = 127 + 90 * np.sin(0.07 * x + 0.3 * t + c) * np.cos(0.05 * y - 0.2 * t) + 40 * (((x // 8 + y // 8 + t) % 2) - 0.5)
    v = v + rng.normal(0, 12, size=(T, H, W, 3))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


MASK_KINDS = ("blob", "thin", "border")


def synthetic_masks(seed: int, T: int, H: int, W: int, kind: str = "blob"):
    """uint8 instance labels [T,H,W] (0 = background): "blob" = two moving ellipses with noisy rims (labels 1, 2); "thin" = a
    one-pixel line (a 3x3 erosion empties it); "border" = a block that touches the top-left image border."""
    import numpy as np

    assert kind in MASK_KINDS, kind
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    m = np.zeros((T, H, W), dtype=np.uint8)
    if kind == "blob":
        for label, (cy, cx, ry, rx) in enumerate(((0.45, 0.35, 0.28, 0.2), (0.6, 0.72, 0.2, 0.16)), start=1):
            d = ((y - (cy + 0.002 * t) * H) / (ry * H)) ** 2 + ((x - (cx + 0.004 * t) * W) / (rx * W)) ** 2
            m[d + rng.normal(0, 0.05, size=(T, H, W)) < 1.0] = label
    elif kind == "thin":
        m[(y == H // 2 + 0 * t) & (x > W // 8) & (x < W - W // 8)] = 1
    else:
        m[(y < H // 2 + t) & (x < W // 3 + 2 * t)] = 1
    return m


_PALETTE = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0]  # the first entries of the DAVIS-2017 palette


def write_davis_tree(root: str, seq: str, frames, masks=None, mode: str = "P") -> str:
    """A DAVIS tree under ``root``: JPEGImages/480p/<seq>/%05d.jpg and (``masks`` given) Annotations/480p/<seq>/%05d.png.  The
    ".jpg" files hold PNG bytes: PIL detects the format from the content, so the decoded frames are exactly ``frames`` on any
    libjpeg.  ``mode``: "P" palette labels (DAVIS-2017), "L" / "RGB" 0/255 masks (DAVIS-2016 style).  Returns ``root``."""
    import os

    import numpy as np
    from PIL import Image

    jd = os.path.join(root, "JPEGImages", "480p", seq)
    os.makedirs(jd, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f)).save(os.path.join(jd, "%05d.jpg" % i), format="PNG")
    if masks is not None:
        ad = os.path.join(root, "Annotations", "480p", seq)
        os.makedirs(ad, exist_ok=True)
        for i, m in enumerate(masks):
            if m is None:
                continue
            if mode == "P":
                im = Image.fromarray(np.ascontiguousarray(m), mode="P")
                im.putpalette(_PALETTE)
            elif mode == "L":
                im = Image.fromarray(((m > 0) * 255).astype(np.uint8))
            elif mode == "RGB":
                im = Image.fromarray(np.repeat(((m > 0) * 255).astype(np.uint8)[..., None], 3, axis=-1))
            else:
                raise ValueError(mode)
            im.save(os.path.join(ad, "%05d.png" % i), format="PNG")
    return root


def write_dycheck_tree(root: str, seq: str, frames, calibration) -> str:
    """A DyCheck tree under ``root``: <seq>/dense/images/%05d.png and <seq>/calibration.txt ("fx fy cx cy").  Returns ``root``."""
    import os

    import numpy as np
    from PIL import Image

    d = os.path.join(root, seq, "dense", "images")
    os.makedirs(d, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f)).save(os.path.join(d, "%05d.png" % i), format="PNG")
    with open(os.path.join(root, seq, "calibration.txt"), "w") as fh:
        fh.write(" ".join(repr(float(v)) for v in calibration) + "\n")
    return root


def synthetic_ground_truth(seed: int, T: int, H: int, W: int, N: int):
    """A raw ground-truth clip as a dataset decodes it, under the L4PData field names (numpy, no batch dimension): rgb in [0, 1];
    depth with some inf, nan and 0 entries and its valid mask; both flow directions and their valid masks; a blob motion mask, its
    valid mask and an instance mask; N tracks (some leave the image) with visibility, validity and depth; one query per track placed
    on the track at a frame centre; point labels; intrinsics, extrinsics and relative poses."""
    import numpy as np

    rng = np.random.default_rng(seed)
    f32 = np.float32
    out = {"rgb_b3thw": np.ascontiguousarray(synthetic_video(seed, T, H, W).transpose(3, 0, 1, 2)).astype(f32) / f32(255)}
    t = np.arange(T)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    depth = (2.0 + 0.5 * np.sin(0.4 * x + 0.3 * t) + 0.1 * y + rng.uniform(0, 0.2, size=(T, H, W))).astype(f32)
    kind = rng.integers(0, 12, size=(T, H, W))
    depth[kind == 0] = np.inf
    depth[kind == 1] = np.nan
    depth[kind == 2] = 0
    out["depth_b1thw"] = depth[None]
    out["depth_valid_b1thw"] = (np.isfinite(depth) & (depth > 0)).astype(f32)[None]
    for name in ("backward", "forward"):
        out[f"flow_2d_{name}_b2thw"] = rng.normal(0, 1.5, size=(2, T, H, W)).astype(f32)
        out[f"flow_2d_{name}_valid_b2thw"] = np.repeat((rng.uniform(size=(1, T, H, W)) > 0.2).astype(f32), 2, axis=0)
    blob = synthetic_masks(seed + 1, T, H, W, "blob")
    out["dyn_mask_b1thw"] = (blob == 1).astype(f32)[None]
    out["dyn_mask_valid_b1thw"] = (rng.uniform(size=(1, T, H, W)) > 0.1).astype(f32)
    out["instanceseg_b1thw"] = (blob > 0).astype(f32)[None]
    # tracks: a random walk from a start inside (or just outside) the image
    start = np.stack([rng.uniform(-1.5, W + 1.5, size=N), rng.uniform(-1.5, H + 1.5, size=N)], axis=1)
    traj = (start[:, :, None] + np.cumsum(rng.normal(0, 0.8, size=(N, 2, T)), axis=2)).astype(f32)
    out["track_2d_traj_bn2t"] = traj
    out["track_2d_vis_bn1t"] = rng.uniform(size=(N, 1, T)) > 0.25
    out["track_2d_valid_bn1t"] = rng.uniform(size=(N, 1, T)) > 0.15
    out["track_2d_depth_bn1t"] = rng.uniform(1, 5, size=(N, 1, T)).astype(f32)
    qt = rng.integers(0, T, size=N)
    n = np.arange(N)
    out["track_2d_pointquerries_bn3"] = np.stack([qt.astype(f32) + f32(0.5), traj[n, 0, qt], traj[n, 1, qt]], axis=1).astype(f32)
    out["track_2d_pointlabels_bn"] = np.ones(N, dtype=f32)
    K = np.eye(4, dtype=f32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 1.1 * W, 1.3 * W, W / 2 - 0.25, H / 2 + 0.75
    out["intrinsics_b44t"] = np.repeat(K[:, :, None], T, axis=2) + (0.01 * np.arange(T, dtype=f32))[None, None, :] * (K > 1)[:, :, None]
    E = np.repeat(np.eye(4, dtype=f32)[:, :, None], T, axis=2)
    E[:3, 3, :] = rng.normal(0, 0.3, size=(3, T)).astype(f32)
    out["extrinsics_b44t"] = E
    out["rel_pose_b6t"] = rng.normal(0, 0.2, size=(6, T)).astype(f32)
    out["intrinsics_b44t"] = out["intrinsics_b44t"].astype(f32)
    return out
