"""Timing of guided up-sampling to the video's own resolution (l4p_amd/utils/native_res.py, csrc/upsample.hip) at the demo size: one
call on a 64-frame clip of 480 x 854 from 224 x 224, C = 4 fields (depth, flow x / y, mask), radius 2; the seeded video of the demo
through VideoDataset, seeded fields, no model.  Prints one JSON line:

  upsample_ms                 device-event time of one guided_upsample after warm-up (median of --iters; _min: the fastest)
  upsample_tbs                compulsory traffic / time: 3 (guide) + 4 C (fields) + 1 (valid) bytes per full-resolution pixel
  upsample_c8_r3_ms           the same call with the largest C and window (8 fields, radius 3)
  bilinear_ms                 context only: F.interpolate(bilinear) of the same four channels - less work and a different function

Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python tools/native_time.py` (separate run).

  python tools/native_time.py [--iters 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l4p_amd.data import VideoDataset  # noqa: E402
from l4p_amd.data.synthetic import synthetic_video  # noqa: E402
from l4p_amd.utils import native_res as NR  # noqa: E402


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
    T, H, W, Cn = 64, 480, 854, 4
    path = "synthetic/480p.mp4"
    ds = VideoDataset(video_paths=[path], crop_size=(T, 224, 224), frames={path: synthetic_video(1, T, H, W)}, device="cuda")
    rgb = ds[0]["rgb_b3thw"][None]
    frames, geometry = ds.source_clip(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    src8 = torch.randn(1, 8, T, 224, 224, generator=g, device="cuda")
    src = src8[:, :Cn].contiguous()
    res = {"frames": T, "src_hw": [H, W], "lo_hw": [224, 224], "channels": Cn, "radius": 2, "iters": args.iters}
    res["upsample_ms"], res["upsample_ms_min"] = timed(lambda: NR.guided_upsample(frames, rgb, src, geometry), args.iters)
    res["upsample_tbs"] = round(T * H * W * (3 + 4 * Cn + 1) / (res["upsample_ms"] * 1e-3) / 1e12, 3)
    res["upsample_c8_r3_ms"], _ = timed(lambda: NR.guided_upsample(frames, rgb, src8, geometry, radius=3), args.iters)
    planes = src.reshape(Cn * T, 1, 224, 224)
    res["bilinear_ms"], _ = timed(lambda: torch.nn.functional.interpolate(planes, size=(H, W), mode="bilinear", align_corners=False),
                                  args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
