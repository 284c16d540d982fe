"""Timing of the 2D result video (l4p_amd/utils/vis2d.py) at the demo size: 64 frames of 224 x 224, five panels, 600 tracks
(tests/vis2d_restate.make_scene at that size), seeded tensors, no model.  Prints one JSON line:

  render_f32_ms / render_u8_ms   device-event time of one render_video_panels call after warm-up (median of --iters)
  dense_only_ms                  the same without the track panel
  to_host_ms                     the single device-to-host copy of the f32 video
  png_write_ms                   write_png_frames of the uint8 video into a temporary directory
  host_restated_s                the same video through the numpy / torch restatement (tests/vis2d_restate.py) on the host CPU

Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/vis2d_time.py --no-host` (separate run).

  python tools/vis2d_time.py [--iters 20] [--no-host]
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

from l4p_amd.utils import vis2d as V  # noqa: E402
from tests import vis2d_restate as RS  # noqa: E402


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
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement and the file writing (e.g. under the profiler)")
    args = ap.parse_args()
    sc = RS.make_scene(T=64, H=224, W=224, N=600, seed=7, ties=True)
    batch, out = RS.scene_tensors(sc, "cuda")
    res = {"frames": 64, "tracks": 600, "panels": 5}
    res["render_f32_ms"], res["render_f32_ms_min"] = timed(lambda: V.render_video_panels(batch, out, RS.TASKS), args.iters)
    res["render_u8_ms"], _ = timed(lambda: V.render_video_panels(batch, out, RS.TASKS, out_dtype=torch.uint8), args.iters)
    res["dense_only_ms"], _ = timed(lambda: V.render_video_panels(batch, out, RS.TASKS[:3]), args.iters)
    vid = V.render_video_panels(batch, out, RS.TASKS)["video"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = vid.cpu().numpy()
    res["to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    if not args.no_host:
        d = tempfile.mkdtemp()
        try:
            t0 = time.perf_counter()
            V.write_png_frames(V.to_uint8(host), d)
            res["png_write_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        finally:
            shutil.rmtree(d)
        hb, ho = RS.scene_tensors(sc, "cpu")
        t0 = time.perf_counter()
        RS.restate(hb, ho, RS.TASKS)
        res["host_restated_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
