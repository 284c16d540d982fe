"""Timing of the moving-object stage (csrc/objects.hip: l4p_objects_label + l4p_objects_roots + l4p_objects_tables) on a seeded
synthetic clip of moving discs (no model: a motion mask of discs that cross the view at constant velocities, the backward flow of
that motion on their pixels, a smooth depth, world points on a plane), at the demo's shape (64, 224, 224) and at the native shape
(64, 480, 854), with and without the flow.  Prints one JSON line per (shape, flow) with:

  label_us, roots_us, tables_us, total_us   device-event time per call of the native entries on preallocated buffers, median over
                       --repeats rounds of --iters calls (after a warm-up); the rounds alternate between the configurations
  wrappers_ms          label_components + object_tracks through the Python wrappers, wall clock, with their allocation and the one
                       host read-back
  bytes, gb_per_s      one read of the mask plus one write of object_id (8 bytes per pixel), divided by label_us: how far the
                       labelling's passes are from a single streaming pass
  counters, K          of the clip;  same_bits: the preallocated calls give what the wrappers gave

  python tools/objects_time.py [--iters 10] [--repeats 7] [--frames 64] [--shapes 224x224 480x854]
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


def disc_clip(seed, T, H, W, n_discs=6):
    """(mask, depth, flow, points, grid) on the device: discs of radius 0.05 .. 0.12 H moving by up to 1.5 % of the frame per frame."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
    t = torch.arange(T, device="cuda").float().view(T, 1, 1)
    mask = torch.full((T, H, W), -2.0, device="cuda")
    flow = torch.zeros(2, T, H, W, device="cuda")
    for _ in range(n_discs):
        cx, cy = float(torch.rand(1, generator=g)) * W, float(torch.rand(1, generator=g)) * H
        vx, vy = (float(torch.rand(1, generator=g)) - 0.5) * 0.03 * W, (float(torch.rand(1, generator=g)) - 0.5) * 0.03 * H
        r = (0.05 + 0.07 * float(torch.rand(1, generator=g))) * H
        on = (xx - (cx + vx * t)) ** 2 + (yy - (cy + vy * t)) ** 2 < r * r
        mask = torch.where(on, torch.full_like(mask, 2.0), mask)
        flow[0] = torch.where(on, torch.full_like(mask, -vx), flow[0])
        flow[1] = torch.where(on, torch.full_like(mask, -vy), flow[1])
    mask = mask + 0.5 * (torch.rand(T, H, W, generator=g) - 0.5).cuda()
    depth = 2.5 + torch.sin(xx / 40) * torch.cos(yy / 35) + 0.0 * t
    points = torch.stack([(xx - W / 2) * depth / W, (yy - H / 2) * depth / W, depth], dim=-1).reshape(-1, 3).contiguous()
    grid = torch.tensor([0.0, 0.0, 0.0, 2.0 * 2.5 / W], device="cuda")
    return mask.contiguous(), depth.contiguous(), flow.contiguous(), points, grid


class Native:
    """The three entries on preallocated buffers (the sizes of a first, sizing run through the wrappers)."""

    def __init__(self, mask, depth, flow, points, grid, K):
        self.lib = _lib.load()
        self.a = (mask, depth, flow, points, grid)
        self.T, self.H, self.W = (int(v) for v in mask.shape)
        self.K, dev = K, mask.device
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        self.ws = torch.empty(int(self.lib.l4p_objects_ws_bytes(self.T, self.H, self.W)), dtype=torch.uint8, device=dev)
        self.tws = torch.empty(max(1, int(self.lib.l4p_objects_tables_ws_bytes(K, self.T))), dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(6, dtype=torch.int64, device=dev)
        T = self.T
        self.o = dict(label=torch.empty(mask.shape, **i32), object_id=torch.empty(mask.shape, **i32), root=torch.empty(K, **i32),
                      n_pixels=torch.empty(K, **i32), first_frame=torch.empty(K, **i32), last_frame=torch.empty(K, **i32),
                      count=torch.empty(K, T, **i32), bbox=torch.empty(K, T, 4, **i32), centroid_px=torch.empty(K, T, 2, **f32),
                      count3d=torch.empty(K, T, **i32), centroid_xyz=torch.empty(K, T, 3, **f32), box3d=torch.empty(K, T, 6, **f32),
                      step=torch.empty(K, T, 3, **f32), speed=torch.empty(K, T, **f32))

    def label(self):
        mask, depth, flow, _, _ = self.a
        _lib.check(self.lib.l4p_objects_label(_stream(), _p(mask), _p(depth), _p(flow), None, self.T, self.H, self.W, 8, 0.0, 64, 2,
                                              _p(self.ws), _p(self.o["label"]), _p(self.o["object_id"]), _p(self.counters)))

    def roots(self):
        o = self.o
        _lib.check(self.lib.l4p_objects_roots(_stream(), _p(self.ws), _p(o["label"]), _p(o["object_id"]), self.T, self.H, self.W, self.K,
                                              _p(o["root"]), _p(o["n_pixels"]), _p(o["first_frame"]), _p(o["last_frame"])))

    def tables(self):
        o = self.o
        _lib.check(self.lib.l4p_objects_tables(_stream(), _p(o["object_id"]), _p(self.a[3]), _p(self.a[4]), self.T, self.H, self.W, self.K,
                                               _p(self.tws), _p(o["count"]), _p(o["bbox"]), _p(o["centroid_px"]), _p(o["count3d"]),
                                               _p(o["centroid_xyz"]), _p(o["box3d"]), _p(o["step"]), _p(o["speed"])))

    def all(self):
        self.label(), self.roots(), self.tables()


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", nargs="*", default=["224x224", "480x854"])
    args = ap.parse_args()
    cands, info = {}, {}
    for shape in args.shapes:
        H, W = (int(v) for v in shape.split("x"))
        mask, depth, flow, points, grid = disc_clip(0, args.frames, H, W)
        for with_flow in (True, False):
            f = flow if with_flow else None
            tag = f"{shape} {'flow' if with_flow else 'no flow'}"
            ref = MO.label_components(mask, depth, f, min_pixels=64, min_frames=2)
            ref.update(MO.object_tracks(ref["object_id"], ref["K"], points, grid))
            n = Native(mask, depth, f, points, grid, ref["K"])
            for _ in range(2):  # warm-up, and the bits
                n.all()
            same = all(torch.equal(n.o[k], ref[k]) for k in n.o) and [int(v) for v in n.counters.tolist()] == list(ref["counters"].values())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = MO.label_components(mask, depth, f, min_pixels=64, min_frames=2)
            MO.object_tracks(r["object_id"], r["K"], points, grid)
            torch.cuda.synchronize()
            cands[tag] = n
            info[tag] = dict(shape=[args.frames, H, W], flow=with_flow, iters=args.iters, repeats=args.repeats, counters=ref["counters"],
                             K=ref["K"], same_bits=bool(same), wrappers_ms=round((time.perf_counter() - t0) * 1e3, 2))
    times = {}
    for _ in range(args.repeats):  # alternated rounds
        for tag, n in cands.items():
            n.label()  # roots and tables need a labelled clip
            for part in ("label", "roots", "tables", "all"):
                times.setdefault((tag, part), []).append(window(getattr(n, part), args.iters))
    for tag, res in info.items():
        for part in ("label", "roots", "tables", "all"):
            v = times[(tag, part)]
            key = part.replace("all", "total") + "_us"
            res[key], res[key + "_min_max"] = round(float(np.median(v)), 1), [round(min(v), 1), round(max(v), 1)]
        res["bytes"] = int(np.prod(res["shape"])) * 8
        res["gb_per_s"] = round(res["bytes"] / (res["label_us"] * 1e-6) / 1e9, 1)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
