"""Timing of the 4D reconstruction (l4p_amd/utils/recon4d.py) at the demo size: 64 frames of 224 x 224, 625 tracks (a 25 x 25
query grid, ~85 % of track-frames visible), seeded tensors, no model.  Prints one JSON line:

  reconstruct_4d_ms    device-event time of one reconstruct_4d call after warm-up (median of --iters), the one read-back included
  readback_ms          a (T + 2)-int64 device-to-host copy after a synchronisation, timed alone (what the call's read-back costs)
  ply_write_ms         write_4d_files of the result (2 T files) into a temporary directory
  host_restated_s      the same geometry through the plain-torch / numpy restatement (tests/recon4d_restate.py) on the host CPU
  points               dense + trail points

Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/recon4d_time.py --no-host` (separate run).

  python tools/recon4d_time.py [--iters 20] [--no-host]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l4p_amd.utils import recon4d as R  # noqa: E402
from tests import recon4d_restate as RS  # noqa: E402

TASKS = ["depth", "camray", "track_2d"]


def demo_inputs(T=64, H=224, W=224, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = 25
    gy, gx = torch.meshgrid(torch.linspace(4.48, 219.52, n), torch.linspace(4.48, 219.52, n), indexing="ij")
    xy0 = torch.stack([gx.reshape(-1), gy.reshape(-1)], 1)
    N = xy0.shape[0]
    traj = xy0[:, :, None] + torch.randn(N, 2, 1, generator=g) * torch.arange(T).float()[None, None] * 0.3
    sc = {"rgb_u8": torch.randint(0, 256, (1, 3, T, H, W), generator=g, dtype=torch.uint8).numpy(),
          "depth_q": torch.randint(1, 256, (T, H, W), generator=g, dtype=torch.uint8).numpy(), "traj": traj.numpy(),
          "vis_logit": (torch.randn(N, T, generator=g) + 2.1).numpy(), "track_depth": (torch.rand(N, T, generator=g) + 0.5).numpy()}
    s = RS.make_scene(T=T, H=8, W=8, N=4)
    K = s["K"].copy()
    K[0], K[5], K[2], K[6] = 200.0, 200.0, 111.5, 111.5
    sc.update(poses=s["poses"], K=K)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (e.g. under the profiler)")
    args = ap.parse_args()
    sc = demo_inputs()
    T = sc["depth_q"].shape[0]
    batch, out = RS.scene_tensors(sc, "cuda")
    for _ in range(3):
        rec = R.reconstruct_4d(batch, out, TASKS)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rec = R.reconstruct_4d(batch, out, TASKS)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    off = torch.zeros(T + 2, dtype=torch.int64, device="cuda")
    rb = []
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off.cpu()
        rb.append((time.perf_counter() - t0) * 1e3)
    d = tempfile.mkdtemp()
    try:
        t0 = time.perf_counter()
        R.write_4d_files(rec, "demo", d, T, 224 * 224, True)
        ply_ms = (time.perf_counter() - t0) * 1e3
    finally:
        shutil.rmtree(d)
    res = {"reconstruct_4d_ms": round(float(np.median(ms)), 3), "reconstruct_4d_ms_min": round(float(np.min(ms)), 3),
           "readback_ms": round(float(np.median(rb)), 3), "ply_write_ms": round(ply_ms, 1),
           "points": int(rec["points"].shape[0] + rec["track_xyz"].shape[0]), "trail_points": int(rec["track_xyz"].shape[0]),
           "frames": T, "tracks": int(sc["traj"].shape[0])}
    if not args.no_host:
        hb, ho = RS.scene_tensors(sc, "cpu")
        t0 = time.perf_counter()
        RS.restate(hb, ho, TASKS)
        res["host_restated_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
