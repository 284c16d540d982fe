"""Timing of the ground-truth clip preparation (l4p_amd/data/l4p_dataset_mini.py, csrc/gt_prep.hip) at a DAVIS-sized raw clip:
64 frames of 480 x 854 with every dense field (rgb, depth, both flows, masks, all valid masks: 14 channels, 1.47 GB of float32)
and 1024 tracks with user queries, resized to 256 x 455 and randomly cropped to (64, 224, 224), one estimation direction;
seeded tensors already on the device, no file decoding, no model.

Two paths are timed, alternating, after 3 warm-up calls each:
  fused    ds[0] of an L4PDataset subclass (three launches, one 4-byte read-back)
  torch    the same steps written with torch operations on the same device tensors - F.interpolate, slicing, indexing, boolean
           masks: what a user would write without these kernels
Times are host-clock milliseconds around one call that ends in a device synchronise.  Prints one JSON line with the median, the
minimum and the maximum of --iters calls of each path, and the largest difference between the two paths' outputs.

  python tools/gt_prep_time.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from l4p_amd.data.l4p_dataset_mini import DENSE_KEYS, L4PData, L4PDataset, draw_crop_offsets  # noqa: E402

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def device_clip(seed, T, H, W, N, dev):
    g = torch.Generator(device=dev).manual_seed(seed)

    def rand(*shape):
        return torch.rand(shape, generator=g, device=dev)

    x = {"rgb_b3thw": rand(3, T, H, W), "depth_b1thw": rand(1, T, H, W) * 5 + 0.5, "depth_valid_b1thw": (rand(1, T, H, W) > 0.2).float(),
         "instanceseg_b1thw": (rand(1, T, H, W) > 0.5).float(), "dyn_mask_b1thw": (rand(1, T, H, W) > 0.5).float(),
         "dyn_mask_valid_b1thw": (rand(1, T, H, W) > 0.1).float()}
    for d in ("backward", "forward"):
        x[f"flow_2d_{d}_b2thw"] = rand(2, T, H, W) * 4 - 2
        x[f"flow_2d_{d}_valid_b2thw"] = (rand(1, T, H, W) > 0.2).float().repeat(2, 1, 1, 1)
    traj = torch.stack([rand(N, T) * (W + 40) - 20, rand(N, T) * (H + 40) - 20], dim=1)
    qt = torch.randint(0, T, (N,), generator=g, device=dev)
    n = torch.arange(N, device=dev)
    x.update({"track_2d_traj_bn2t": traj, "track_2d_vis_bn1t": rand(N, 1, T) > 0.25, "track_2d_valid_bn1t": rand(N, 1, T) > 0.15,
              "track_2d_depth_bn1t": rand(N, 1, T) + 1,
              "track_2d_pointquerries_bn3": torch.stack([qt.float() + 0.5, traj[n, 0, qt], traj[n, 1, qt]], dim=1),
              "track_2d_pointlabels_bn": torch.ones(N, device=dev),
              "intrinsics_b44t": torch.eye(4, device=dev)[:, :, None].repeat(1, 1, T)})
    return x


class Clip(L4PDataset):
    def getitem_helper(self, index):
        return L4PData(seq_name="clip", **self.tensors)


def torch_prepare(x, res, crop, direction):
    """The reference's steps (l4p_dataset_mini.py:237-395, 499-519, 576-580) with torch operations on device tensors; the clip
    needs no mirror padding at this size."""
    _, T, H, W = x["rgb_b3thw"].shape
    fh, fw = res[0] / H, res[1] / W
    Tn, Hn, Wn = crop
    t0, i0, j0 = draw_crop_offsets((T - Tn, res[0] - Hn, res[1] - Wn), False, False)
    out = {}
    for k in DENSE_KEYS:
        v = F.interpolate(x[k][None], (T, res[0], res[1]), mode="trilinear" if k == "rgb_b3thw" else "nearest")[0]
        if k in ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw"):
            v[0] = v[0] * fw
            v[1] = v[1] * fh
        out[k] = v[:, t0:t0 + Tn, i0:i0 + Hn, j0:j0 + Wn]
    traj = x["track_2d_traj_bn2t"].clone()
    traj[:, 0] = traj[:, 0] * fw
    traj[:, 1] = traj[:, 1] * fh
    q = x["track_2d_pointquerries_bn3"].clone()
    q[:, 1] = q[:, 1] * fw
    q[:, 2] = q[:, 2] * fh
    keep = (q[:, 0] > t0) & (q[:, 0] < t0 + Tn) & (q[:, 1] > j0) & (q[:, 1] < j0 + Wn) & (q[:, 2] > i0) & (q[:, 2] < i0 + Hn)
    q = q[keep]
    traj = traj[..., t0:t0 + Tn][keep]
    vis = x["track_2d_vis_bn1t"][..., t0:t0 + Tn][keep]
    valid = x["track_2d_valid_bn1t"][..., t0:t0 + Tn][keep]
    out["track_2d_depth_bn1t"] = x["track_2d_depth_bn1t"][..., t0:t0 + Tn][keep]
    out["track_2d_pointlabels_bn"] = x["track_2d_pointlabels_bn"][keep]
    traj[:, 0] = traj[:, 0] - j0
    traj[:, 1] = traj[:, 1] - i0
    vis = vis & ~((traj[:, 0] >= Wn) | (traj[:, 0] < 0) | (traj[:, 1] >= Hn) | (traj[:, 1] < 0))[:, None]
    q = q - torch.tensor([t0, j0, i0], dtype=torch.float32, device=q.device)
    time_nt = 0.5 + torch.arange(Tn, device=q.device)[None, :]
    ok = time_nt >= q[:, :1] if direction == 1 else time_nt <= q[:, :1]
    out.update({"track_2d_traj_bn2t": traj, "track_2d_vis_bn1t": vis, "track_2d_valid_bn1t": valid & ok[:, None, :],
                "track_2d_pointquerries_bn3": q})
    k = x["intrinsics_b44t"][..., t0:t0 + Tn].clone()
    k[0, 0], k[1, 1] = k[0, 0] * fw, k[1, 1] * fh
    k[0, 2], k[1, 2] = (k[0, 2] + 0.5) * fw - 0.5 - j0, (k[1, 2] + 0.5) * fh - 0.5 - i0
    out["intrinsics_b44t"] = k
    mean = torch.tensor(MEAN, device=q.device)[:, None, None, None]
    std = torch.tensor(STD, device=q.device)[:, None, None, None]
    out["rgb_b3thw"] = (out["rgb_b3thw"] - mean) / std
    return {k: v.contiguous() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, nargs=3, default=(64, 480, 854), metavar=("T", "H", "W"))
    ap.add_argument("--tracks", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    T, H, W = args.size
    res, crop = (256, 455), (T, 224, 224)
    x = device_clip(0, T, H, W, args.tracks, dev)
    ds = Clip(crop_size=crop, resize_size=res, estimation_directions=[1], scale_queries_on_resize=True)
    ds.tensors = x

    def fused():
        return ds[0]

    def plain():
        return torch_prepare(x, res, crop, 1)

    # same seed, same crop: the two paths agree
    torch.manual_seed(1)
    a = fused()
    torch.manual_seed(1)
    b = plain()
    diff = {}
    for k, v in b.items():
        assert a[k].shape == v.shape, (k, a[k].shape, v.shape)
        d = float((a[k].float() - v.float()).abs().max()) if v.numel() else 0.0
        if d:
            diff[k] = d
    for fn in (fused, plain):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {"fused": [], "torch": []}
    for i in range(args.iters):
        for name, fn in (("fused", fused), ("torch", plain)):
            torch.manual_seed(100 + i)
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3)
    out = {"raw": [T, H, W], "resize": list(res), "crop": list(crop), "tracks": args.tracks, "kept_queries_first_call": int(a["track_2d_pointquerries_bn3"].shape[0]),
           "iters": args.iters, "max_abs_difference": diff}
    for name, v in ms.items():
        out[name + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
