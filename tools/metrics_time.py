"""Timing of the evaluation metrics (l4p_amd/metrics.py) at the demo size: 64 frames of 224 x 224, 625 queries, all five tasks,
median depth alignment, seeded tensors, no model.  Prints one JSON line:

  forward_ms                  device-event time of one L4PMetrics.forward after warm-up (median of --iters; _min: the fastest)
  depth_ms / flow_ms / mask_ms / tracks_ms / cameras_ms   each entry on its own (depth with the median alignment)
  depth_none_ms               the depth error pass alone (no alignment)
  *_gbs                       bytes read by the dense pass / its time: depth_none 3 arrays, flow 6, mask 3 of n floats

Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py` (separate run).

  python tools/metrics_time.py [--iters 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l4p_amd import metrics as M  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    T, H, W, N = 64, 224, 224, 625
    n = T * H * W
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape):
        return torch.rand(*shape, generator=g, device="cuda")

    gt = 0.5 + 9.5 * rnd(1, 1, T, H, W)
    batch = {
        "rgb_b3thw": torch.zeros(1, 3, T, H, W, device="cuda"),
        "depth_b1thw": gt, "depth_valid_b1thw": (rnd(1, 1, T, H, W) > 0.3).float(),
        "flow_2d_backward_b2thw": 10 * rnd(1, 2, T, H, W) - 5, "flow_2d_backward_valid_b2thw": (rnd(1, 2, T, H, W) > 0.15).float(),
        "dyn_mask_b1thw": (rnd(1, 1, T, H, W) > 0.6).float(), "dyn_mask_valid_b1thw": (rnd(1, 1, T, H, W) > 0.3).float(),
        "track_2d_traj_bn2t": 224 * rnd(1, N, 2, T), "track_2d_vis_bn1t": rnd(1, N, 1, T) > 0.3,
        "track_2d_valid_bn1t": rnd(1, N, 1, T) > 0.1,
        "track_2d_pointquerries_bn3": torch.cat([torch.floor(T * rnd(1, N, 1)) + 0.5, 224 * rnd(1, N, 2)], 2),
        "extrinsics_b44t": torch.eye(4, device="cuda")[None, :, :, None].repeat(1, 1, 1, T).contiguous(),
    }
    pose = torch.eye(4, device="cuda").reshape(1, 16, 1).repeat(1, 1, T)
    pose[:, 3] = rnd(1, T)
    pose[:, 7] = rnd(1, T)
    pose[:, 11] = rnd(1, T)
    batch["extrinsics_b44t"][:, 0, 3] = -pose[:, 3] * 2 + 0.01 * rnd(1, T)
    batch["extrinsics_b44t"][:, 1, 3] = -pose[:, 7] * 2
    batch["extrinsics_b44t"][:, 2, 3] = -pose[:, 11] * 2
    out = {
        "depth_est_b1thw": gt * (0.6 + 1.3 * rnd(1, 1, T, H, W)), "flow_2d_backward_est_b2thw": 10 * rnd(1, 2, T, H, W) - 5,
        "dyn_mask_est_b1thw": rnd(1, 1, T, H, W) - 0.5,
        "track_2d_traj_est_bn2t": batch["track_2d_traj_bn2t"] + 8 * rnd(1, N, 2, T) - 4, "track_2d_vis_est_bn1t": rnd(1, N, 1, T) - 0.4,
        "traj3d_est_b16t": pose.contiguous(),
    }
    mod = M.L4PMetrics()
    res = {"frames": T, "hw": [H, W], "queries": N, "iters": args.iters}
    res["forward_ms"], res["forward_ms_min"] = timed(lambda: mod(batch, out), args.iters)
    d = (out["depth_est_b1thw"], batch["depth_b1thw"], batch["depth_valid_b1thw"])
    f = (out["flow_2d_backward_est_b2thw"], batch["flow_2d_backward_b2thw"], batch["flow_2d_backward_valid_b2thw"])
    k = (out["dyn_mask_est_b1thw"], batch["dyn_mask_b1thw"], batch["dyn_mask_valid_b1thw"])
    res["depth_ms"], _ = timed(lambda: M.depth_metrics(*d, "median"), args.iters)
    res["depth_lstsq_ms"], _ = timed(lambda: M.depth_metrics(*d, "lstsq"), args.iters)
    res["depth_none_ms"], _ = timed(lambda: M.depth_metrics(*d, "none"), args.iters)
    res["flow_ms"], _ = timed(lambda: M.flow_metrics(*f), args.iters)
    res["mask_ms"], _ = timed(lambda: M.mask_metrics(*k), args.iters)
    res["tracks_ms"], _ = timed(lambda: M.track_metrics(out["track_2d_traj_est_bn2t"], batch["track_2d_traj_bn2t"],
                                                        out["track_2d_vis_est_bn1t"], batch["track_2d_vis_bn1t"],
                                                        batch["track_2d_valid_bn1t"], batch["track_2d_pointquerries_bn3"], (H, W)),
                                args.iters)
    res["cameras_ms"], _ = timed(lambda: M.camera_metrics(out["traj3d_est_b16t"], batch["extrinsics_b44t"]), args.iters)
    for name, arrays in (("depth_none", 3), ("flow", 6), ("mask", 3)):
        res[name + "_gbs"] = round(arrays * n * 4 / (res[name + "_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
