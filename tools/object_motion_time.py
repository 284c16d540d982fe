"""Timing of the object-motion stage (csrc/object_motion.hip: l4p_objects_motion + l4p_objects_canonical, then one
static_map.fuse_points per object and l4p_objects_place) on the seeded synthetic clip of tools/objects_time.py (moving discs, the
backward flow of their motion, world points on a smooth surface), at the demo's shape (16, 224, 224) and at the native shape
(16, 480, 854).  Prints one JSON line per shape with:

  motion_us, canonical_us, place_us   device-event time per call of the native entries on preallocated buffers, warm, median over
                       --repeats rounds of --iters calls, with [min, max] over the rounds beside each; the rounds alternate between
                       the shapes.  motion = the 2 + n_refits pixel passes, the solves and the composition (n_refits = 1).
  models_ms            object_models through the Python wrapper, wall clock around a synchronisation: K fuse_points calls with
                       their allocations and one host read-back each (median and [min, max] over the rounds)
  wrappers_ms          rigid_motion through the Python wrapper, wall clock, with its allocations (no read-back)
  min_bytes, gb_per_s  the least the three pixel passes can read: object_id once per pixel and pass (4 bytes), and per object pixel
                       of a frame t >= 1 its flow (8), its predecessor's id (4) and the two point rows (24); divided by motion_us,
                       which also holds the memsets, the solves and the composition: a lower bound on the passes' rate
  K, n_object_pixels, n_pairs, n_valid_rows, n_vertices   of the clip;  same_bits: the preallocated calls give what the wrapper gave

  python tools/object_motion_time.py [--iters 10] [--repeats 7] [--frames 16] [--shapes 224x224 480x854]
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

from l4p_amd import _lib  # noqa: E402
from l4p_amd.ops import _p, _stream  # noqa: E402
from l4p_amd.utils import moving_objects as MO  # noqa: E402
from l4p_amd.utils import object_motion as OM  # noqa: E402
from tools.objects_time import disc_clip, window  # noqa: E402

N_REFITS, INLIER_VOXELS, MIN_PAIRS = 1, 2.0, 16


class Native:
    """The entries on preallocated buffers."""

    def __init__(self, ids, K, points, grid, flow, models, pose):
        self.lib = _lib.load()
        self.a = (ids, points, grid, flow)
        self.T, self.H, self.W = (int(v) for v in ids.shape)
        self.K, dev = K, ids.device
        T = self.T
        i32, f32, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(1, int(self.lib.l4p_objects_motion_ws_bytes(K, T))), dtype=torch.uint8, device=dev)
        self.o = dict(motion=torch.empty(K, T, 12, **f32), n_pairs=torch.empty(K, T, **i32), n_inliers=torch.empty(K, T, **i32),
                      n_far=torch.empty(K, T, **i32), rms=torch.empty(K, T, **f32), valid=torch.empty(K, T, **u8),
                      pose=torch.empty(K, T, 12, **f32), pose_valid=torch.empty(K, T, **u8),
                      canonical=torch.empty(T * self.H * self.W, 3, **f32))
        self.models, self.pose, self.placed = models, pose, torch.empty_like(models["xyz"])

    def motion(self):
        ids, points, grid, flow = self.a
        o = self.o
        _lib.check(self.lib.l4p_objects_motion(_stream(), _p(ids), _p(points), _p(flow), _p(grid), self.T, self.H, self.W, self.K, N_REFITS,
                                               INLIER_VOXELS, MIN_PAIRS, _p(self.ws), _p(o["motion"]), _p(o["n_pairs"]), _p(o["n_inliers"]),
                                               _p(o["n_far"]), _p(o["rms"]), _p(o["valid"]), None, _p(o["pose"]), _p(o["pose_valid"])))

    def canonical(self):
        ids, points, _, _ = self.a
        _lib.check(self.lib.l4p_objects_canonical(_stream(), _p(ids), _p(points), _p(self.ws), self.T, self.H, self.W, self.K,
                                                  _p(self.o["canonical"])))

    def place(self):
        m = self.models
        if m["xyz"].shape[0]:
            _lib.check(self.lib.l4p_objects_place(_stream(), _p(m["xyz"]), _p(m["object"]), _p(self.pose), int(m["xyz"].shape[0]), self.K,
                                                  self.T, self.T - 1, _p(self.placed)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--shapes", nargs="*", default=["224x224", "480x854"])
    args = ap.parse_args()
    cands, info, clips = {}, {}, {}
    for shape in args.shapes:
        H, W = (int(v) for v in shape.split("x"))
        T = args.frames
        mask, depth, flow, points, grid = disc_clip(0, T, H, W)
        res = MO.label_components(mask, depth, flow, min_pixels=64, min_frames=2)
        res["grid"] = grid
        colors = torch.randint(0, 256, (T * H * W, 3), dtype=torch.uint8, device="cuda")
        ids, K = res["object_id"], res["K"]
        kw = dict(n_refits=N_REFITS, inlier_voxels=INLIER_VOXELS, min_pairs=MIN_PAIRS)
        ref = OM.rigid_motion(ids, K, points, grid, flow, **kw)
        models = OM.object_models(res, ref, colors, T)
        n = Native(ids, K, points, grid, flow, models, ref["pose"])
        for _ in range(2):  # warm-up, and the bits
            n.motion(), n.canonical(), n.place()
        same = all(torch.equal(n.o[k].reshape(-1).view(torch.uint8), ref[k].reshape(-1).view(torch.uint8)) for k in n.o)
        same = same and torch.equal(n.placed.view(torch.int32), OM.place_models(models, ref["pose"], T - 1).view(torch.int32))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        OM.rigid_motion(ids, K, points, grid, flow, **kw)
        torch.cuda.synchronize()
        on = (ids[1:] >= 0).sum().item()
        cands[shape], clips[shape] = n, (res, ref, colors, T)
        info[shape] = dict(shape=[T, H, W], iters=args.iters, repeats=args.repeats, n_refits=N_REFITS, K=K,
                           n_object_pixels=int((ids >= 0).sum()), n_pairs=int(ref["n_pairs"].sum()), n_valid_rows=int(ref["valid"].sum()),
                           n_vertices=int(models["offsets"][-1]), same_bits=bool(same), wrappers_ms=round((time.perf_counter() - t0) * 1e3, 2),
                           min_bytes=(2 + N_REFITS) * (4 * T * H * W + 36 * int(on)))
    times = {}
    for _ in range(args.repeats):  # alternated rounds
        for shape, n in cands.items():
            for part in ("motion", "canonical", "place"):
                times.setdefault((shape, part), []).append(window(getattr(n, part), args.iters))
            res, ref, colors, T = clips[shape]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            OM.object_models(res, ref, colors, T)
            torch.cuda.synchronize()
            times.setdefault((shape, "models"), []).append((time.perf_counter() - t0) * 1e3)
    for shape, res in info.items():
        for part, unit, nd in (("motion", "us", 1), ("canonical", "us", 1), ("place", "us", 1), ("models", "ms", 2)):
            v = times[(shape, part)]
            key = f"{part}_{unit}"
            res[key], res[key + "_min_max"] = round(float(np.median(v)), nd), [round(min(v), nd), round(max(v), nd)]
        res["gb_per_s"] = round(res["min_bytes"] / (res["motion_us"] * 1e-6) / 1e9, 1)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
