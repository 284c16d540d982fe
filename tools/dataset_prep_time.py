"""Timing of the DAVIS clip preparation (l4p_amd/data/davis.py -> prepare_clip) at the dataset's size: 50 frames of 480 x 854 with
palette annotations, crop (56, 224, 224), query spacing 0.02 (2500 candidates); seeded arrays already on the device, no file
decoding, no model.  Prints one JSON line:

  prepare_ms                 device-event time of one prepare_clip call (RGB + mask + selection, the count read-back included), warm,
                             median of --iters
  rgb_only_ms                the same without annotations and with "uniform" sampling (VideoDataset's path)
  mask_ms / select_ms        l4p_instance_mask_clip alone / l4p_seg_query_select + the 4-byte read-back alone
  mask_share                 (prepare_ms - rgb_only_ms) / prepare_ms
  host_restated_s            the same sample through the numpy / torch restatement (tests/datasets_restate.py) on the host CPU
  host_restated_mask_s       its mask + selection part alone

  python tools/dataset_prep_time.py [--iters 20] [--no-host]
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

from l4p_amd.data import video_dataset as vd  # noqa: E402
from l4p_amd.data.synthetic import synthetic_masks, synthetic_video  # noqa: E402
from tests import datasets_restate as dr  # noqa: E402


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
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (e.g. under the profiler)")
    args = ap.parse_args()
    T, H, W, crop, res, spacing = 50, 480, 854, (56, 224, 224), (224, 224), 0.02
    frames, masks = synthetic_video(41, T, H, W), synthetic_masks(42, T, H, W, "blob")
    fd, md = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda()

    def full():
        return vd.prepare_clip(fd, crop, res, None, 1, spacing, annotations=md, annotation_mode="P", sampling="uniform_over_seg")

    s = full()
    out = {"frames": T, "size": [H, W], "crop": list(crop), "candidates": int(vd.seg_cells(spacing).shape[0]),
           "queries": int(s["track_2d_pointquerries_bn3"].shape[0])}
    out["prepare_ms"], out["prepare_ms_min"] = timed(full, args.iters)
    out["rgb_only_ms"], _ = timed(lambda: vd.prepare_clip(fd, crop, res, None, 1, spacing), args.iters)
    fidx = torch.tensor(vd.mirror_pad_indices(T, crop[0])[: crop[0]], dtype=torch.int32, device="cuda")
    out["mask_ms"], _ = timed(lambda: vd.instance_mask_clip(md, "P", res, fidx, res[0], res[1], 0, 0, *crop), args.iters)
    seg0 = s["instanceseg_b1thw"][0, 0]
    out["select_ms"], _ = timed(lambda: vd.select_queries_over_seg(seg0, spacing), args.iters)
    out["mask_share"] = round((out["prepare_ms"] - out["rgb_only_ms"]) / out["prepare_ms"], 3)
    if not args.no_host:
        out["host_threads"] = torch.get_num_threads()
        t0 = time.perf_counter()
        o = dr.davis_sample(frames, masks, "P", crop, res, 1, spacing, rgb=False)
        out["host_restated_mask_s"] = round(time.perf_counter() - t0, 2)
        t0 = time.perf_counter()
        o = dr.davis_sample(frames, masks, "P", crop, res, 1, spacing)
        out["host_restated_s"] = round(time.perf_counter() - t0, 2)
        assert np.array_equal(o["instanceseg_b1thw"], s["instanceseg_b1thw"].cpu().numpy())
        assert np.array_equal(o["track_2d_pointquerries_bn3"], s["track_2d_pointquerries_bn3"].cpu().numpy())
        assert np.array_equal(o["rgb_b3thw"], s["rgb_b3thw"].cpu().numpy())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
