"""Timing of the free-viewpoint 4D renderer (l4p_amd/utils/view4d.py) at the demo size: 64 frames of 224 x 224, 625 tracks (the
seeded tensors of tools/recon4d_time.py, no model), 64 views of 480 x 640 along the default orbit path, default point size.
Prints one JSON line:

  render_4d_views_ms   device-event time of one render_4d_views call after warm-up (median of --iters; no host synchronisation inside)
  reconstruct_4d_ms    the same for reconstruct_4d in the same run, for scale (its one read-back included)
  splat_only_ms        render_4d_views with frusta="none" (what the triangles add is the difference)
  one_chunk_ms         render_4d_views with a workspace budget that holds all views at once
  covered              fraction of the 64 x 480 x 640 pixels that show something
  points               dense + trail points of the reconstruction

Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/view4d_time.py` (separate run).

  python tools/view4d_time.py [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l4p_amd.utils import recon4d as R  # noqa: E402
from l4p_amd.utils import view4d as V4  # noqa: E402
from recon4d_time import TASKS, demo_inputs  # noqa: E402
from tests import recon4d_restate as RS  # noqa: E402


def event_ms(fn, iters):
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
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sc = demo_inputs()
    T, H, W = sc["depth_q"].shape
    size, views = (480, 640), 64
    batch, out = RS.scene_tensors(sc, "cuda")
    rec = R.reconstruct_4d(batch, out, TASKS)
    path = V4.orbit_views(rec, out["depth_est_b1thw"], T, views)
    K = sc["K"].reshape(4, 4, T)[:, :, 0].astype(np.float64)
    intr = V4.scaled_intrinsics(K, (H, W), size)
    cams = torch.from_numpy(path["cam_T_world"]).float().cuda()
    frames = torch.from_numpy(path["frames"]).int().cuda()
    render = lambda **kw: V4.render_4d_views(rec, T, H * W, cams, intr, size, frames, **kw)  # noqa: E731
    res = {"frames": T, "tracks": int(sc["traj"].shape[0]), "views": views, "size": list(size), "point_size": 0.02,
           "points": int(rec["points"].shape[0] + rec["track_xyz"].shape[0]), "look_at_distance": round(path["d0"], 4)}
    res["render_4d_views_ms"], res["render_4d_views_ms_min"] = event_ms(render, args.iters)
    res["reconstruct_4d_ms"], _ = event_ms(lambda: R.reconstruct_4d(batch, out, TASKS), args.iters)
    res["splat_only_ms"], _ = event_ms(lambda: render(frusta="none"), args.iters)
    res["one_chunk_ms"], _ = event_ms(lambda: render(workspace_bytes=views * size[0] * size[1] * 8), args.iters)
    res["covered"] = round(float((render()["index"] != -1).float().mean()), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
