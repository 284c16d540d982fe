"""Timing of the static scene map (csrc/static_map.hip: l4p_static_map_insert + _count + _emit) at the demo's shape (64, 224, 224) on
seeded synthetic outputs (no model: a depth field over a slowly moving camera through recon4d.reconstruct_4d, a motion mask over a
moving disc), with the default voxel (2 px at the median depth of frame 0), against the plain-torch composition of the same map
(torch.unique(keys, return_inverse=True) + index_add_ / scatter_reduce_) on the same GPU.  Prints one JSON line:

  insert_us, count_us, emit_us, total_us   device-event time per call, median over --repeats rounds; the rounds alternate between
                       the candidates (native, --alt-lib if given, torch), as the measuring guide asks
  torch_us             the torch composition, same rounds
  alt_*                the same three entries of a second build of the library (--alt-lib: a variant under trial, built with
                       make VARIANT=<name> into l4p_amd/lib/libl4p_hip_<name>.so), checked to give the same bits
  bytes                compulsory traffic of one map: per point 12 B xyz + 3 B colour + 4 B mask read, 4 B slot index written and
                       read twice, 4 B voxel_id written; the 64-byte slots cleared once (capacity x 64 B); per voxel one slot read
  counters             of the map;  same_as_torch: the torch composition gives the same voxels, counts and colours

  python tools/static_map_time.py [--iters 20] [--repeats 9] [--alt-lib l4p_amd/lib/libl4p_hip_<name>.so]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l4p_amd import _lib  # noqa: E402
from l4p_amd.ops import _p, _stream  # noqa: E402
from l4p_amd.utils import recon4d, static_map as SM  # noqa: E402


def demo_outputs(seed, T=64, H=224, W=224):
    """(batch, out): a smooth depth field, a camera that turns and moves a little per frame, a disc that crosses the view."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
    t = torch.arange(T, device="cuda").float().view(1, 1, T, 1, 1)
    depth = 2.5 + torch.sin(xx / 40 + 0.02 * t) * torch.cos(yy / 35) + 0.01 * torch.rand(1, 1, T, H, W, generator=g, device="cuda")
    K = torch.eye(4, device="cuda").view(1, 4, 4, 1).repeat(1, 1, 1, T).clone()
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 200.0, 205.0, 111.5, 111.0
    P = torch.eye(4, device="cuda").view(1, 4, 4, 1).repeat(1, 1, 1, T).clone()
    a = 0.004 * torch.arange(T, device="cuda").float()
    P[:, 0, 0], P[:, 0, 2], P[:, 2, 0], P[:, 2, 2] = torch.cos(a), torch.sin(a), -torch.sin(a), torch.cos(a)
    P[:, 0, 3], P[:, 2, 3] = 0.01 * torch.arange(T, device="cuda").float(), 0.004 * torch.arange(T, device="cuda").float()
    cx = (20 + (W - 40) * torch.arange(T, device="cuda").float() / (T - 1)).view(1, 1, T, 1, 1)
    mask = torch.where((xx - cx) ** 2 + (yy - H / 2) ** 2 < 30.0 ** 2, 2.0, -2.0) + 0.5 * torch.randn(1, 1, T, H, W, generator=g, device="cuda")
    batch = {"rgb_b3thw": torch.rand(1, 3, T, H, W, generator=g, device="cuda") * 4 - 2,
             "rgb_mean_b3111": torch.tensor((0.485, 0.456, 0.406), device="cuda").reshape(1, 3, 1, 1, 1),
             "rgb_std_b3111": torch.tensor((0.229, 0.224, 0.225), device="cuda").reshape(1, 3, 1, 1, 1), "seq_name": ["clip"]}
    out = {"depth_est_b1thw": depth.contiguous(), "dyn_mask_est_b1thw": mask.contiguous(),
           "traj3d_est_b16t": P.reshape(1, 16, T).contiguous(), "traj3d_intrinsics_est_b16t": K.reshape(1, 16, T).contiguous()}
    return batch, out


def torch_composition(points, colors, mask, grid, T, min_frames=2):
    """The same map with torch ops: keys in f32 as the kernel forms them, torch.unique for the voxels, index_add_ / scatter_reduce_ for
    the per-voxel state, a sort of the kept voxels' first points for the output order."""
    M = points.shape[0]
    HW = M // T
    q = (points - grid[:3]) / grid[3]
    i = torch.floor(q)
    ok = torch.isfinite(points).all(1) & ~(mask > 0) & ((i >= -(1 << 20)) & (i <= (1 << 20) - 1)).all(1)
    used = torch.nonzero(ok)[:, 0]
    f = torch.floor((q[used] - i[used]) * 65536.0).long()
    ii = i[used].long() + (1 << 20)
    keys = ii[:, 0] | (ii[:, 1] << 21) | (ii[:, 2] << 42)
    uk, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
    nv = uk.shape[0]
    sum_f = torch.zeros(nv, 3, dtype=torch.long, device=points.device).index_add_(0, inv, f)
    sum_c = torch.zeros(nv, 3, dtype=torch.long, device=points.device).index_add_(0, inv, colors[used].long())
    first = torch.full((nv,), M, dtype=torch.long, device=points.device).scatter_reduce_(0, inv, used, "amin")
    frame = used // HW
    last = torch.zeros(nv, dtype=torch.long, device=points.device).scatter_reduce_(0, inv, frame, "amax")
    pairs = torch.unique(inv * T + frame)
    n_frames = torch.bincount(pairs // T, minlength=nv)
    kept = torch.nonzero(n_frames >= min_frames)[:, 0]
    kept = kept[torch.argsort(first[kept])]
    c = cnt[kept].double()[:, None]
    idx = torch.stack([((uk[kept] >> s) & 0x1FFFFF) - (1 << 20) for s in (0, 21, 42)], dim=1).double()
    xyz = (grid[:3].double() + (idx + (sum_f[kept].double() + 0.5 * c) / (c * 65536.0)) * grid[3].double()).float()
    rgb = ((2 * sum_c[kept] + cnt[kept][:, None]) // (2 * cnt[kept][:, None])).to(torch.uint8)
    out_idx = torch.full((nv,), -1, dtype=torch.int32, device=points.device)
    out_idx[kept] = torch.arange(kept.shape[0], dtype=torch.int32, device=points.device)
    voxel_id = torch.full((M,), -1, dtype=torch.int32, device=points.device)
    voxel_id[used] = out_idx[inv]
    return dict(xyz=xyz, colors=rgb, count=cnt[kept].int(), n_frames=n_frames[kept].int(), last_frame=last[kept].int(),
                first_point=first[kept].int(), key=uk[kept], voxel_id=voxel_id)


def bind(path):
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Native:
    """The three entries on preallocated buffers (the sizes of the first, sizing run)."""

    def __init__(self, lib, pts, col, mask, grid, T, cap, V):
        self.lib, self.a = lib, (pts, col, mask, grid)
        self.T, self.HW, self.cap, self.V = T, pts.shape[0] // T, cap, V
        M, dev = pts.shape[0], pts.device
        self.ws = torch.empty(int(lib.l4p_static_map_ws_bytes(cap, M)), dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(8, dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.o = dict(xyz=torch.empty(V, 3, device=dev), colors=torch.empty(V, 3, dtype=torch.uint8, device=dev), count=torch.empty(V, **i32),
                      n_frames=torch.empty(V, **i32), first_frame=torch.empty(V, **i32), last_frame=torch.empty(V, **i32),
                      first_point=torch.empty(V, **i32), key=torch.empty(V, dtype=torch.int64, device=dev), voxel_id=torch.empty(M, **i32))

    def insert(self):
        pts, col, mask, grid = self.a
        _lib.check(self.lib.l4p_static_map_insert(_stream(), _p(pts), _p(col), _p(mask), None, _p(grid), self.T, self.HW, self.cap, _p(self.ws)))

    def count(self):
        _lib.check(self.lib.l4p_static_map_count(_stream(), _p(self.ws), self.T, self.HW, self.cap, 2, 1, _p(self.counters)))

    def emit(self):
        o = self.o
        _lib.check(self.lib.l4p_static_map_emit(_stream(), _p(self.ws), _p(self.a[3]), self.T, self.HW, self.cap, self.V, _p(o["xyz"]),
                                                _p(o["colors"]), _p(o["count"]), _p(o["n_frames"]), _p(o["first_frame"]), _p(o["last_frame"]),
                                                _p(o["first_point"]), _p(o["key"]), _p(o["voxel_id"])))

    def all(self):
        self.insert(), self.count(), self.emit()


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--alt-lib", default=None)
    args = ap.parse_args()
    T, H, W = args.frames, 224, 224
    batch, out = demo_outputs(0, T, H, W)
    rec = recon4d.reconstruct_4d(batch, out, ["depth", "camray"])
    pts, col = rec["points"], rec["colors"]
    mask = out["dyn_mask_est_b1thw"].reshape(-1).contiguous()
    grid = SM.default_grid(out)
    ref = SM.fuse_points(pts, col, T, grid=grid, dyn_mask=mask)
    k = ref["counters"]
    M, cap, V = pts.shape[0], SM.default_capacity(pts.shape[0]), k["n_kept"]
    cands = {"": Native(_lib.load(), pts, col, mask, grid, T, cap, V)}
    if args.alt_lib:
        cands["alt_"] = Native(bind(args.alt_lib), pts, col, mask, grid, T, cap, V)
    res = {"shape": [T, H, W], "iters": args.iters, "repeats": args.repeats, "voxel_size": float(grid[3]), "table_capacity": cap,
           "counters": k}
    for tag, n in cands.items():  # warm-up, and the bits
        for _ in range(3):
            n.all()
        res[tag + "same_bits"] = all(torch.equal(n.o[f], ref[f]) for f in n.o) and [int(v) for v in n.counters.tolist()] == list(k.values())
    tm = torch_composition(pts, col, mask, grid, T)
    res["same_as_torch"] = all(torch.equal(tm[f], ref[f]) for f in tm)
    for _ in range(2):
        torch_composition(pts, col, mask, grid, T)
    torch.cuda.synchronize()
    times = {}
    for _ in range(args.repeats):  # alternated rounds
        for tag, n in cands.items():
            for part in ("insert", "count", "emit", "all"):
                if part != "insert":
                    n.insert()  # count and emit need a filled table; emit a counted one
                if part == "emit":
                    n.count()
                times.setdefault(tag + part, []).append(window(getattr(n, part), args.iters))
        times.setdefault("torch", []).append(window(lambda: torch_composition(pts, col, mask, grid, T), max(2, args.iters // 5)))
    for name, v in times.items():
        key = name.replace("all", "total") + "_us"
        res[key], res[key + "_min_max"] = round(float(np.median(v)), 1), [round(min(v), 1), round(max(v), 1)]
    res["bytes"] = M * (12 + 3 + 4 + 4 * 3 + 4) + cap * 64 + k["n_voxels"] * 64
    res["tb_per_s"] = round(res["bytes"] / (res["total_us"] * 1e-6) / 1e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
