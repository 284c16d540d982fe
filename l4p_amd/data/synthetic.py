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
