"""Timing of the scene-flow kernel (csrc/sceneflow.hip, l4p_scene_flow alone) at the demo's shape (1, 64, 224, 224), seeded
tensors, no model, against the plain-torch composition of the same arithmetic on the same GPU.  Prints one JSON line:

  scene_flow_us        device-event time per l4p_scene_flow call (median over --repeats windows of --iters calls each); the calls
                       rotate over --sets independent input / output sets so that the working set (sets x 144 MB) exceeds the
                       256 MiB Infinity Cache and the traffic is HBM traffic
  bytes_per_call       45 B per pixel: 12 read (depth, flow), 4 gathered (the previous depth plane, once), 29 written
  tb_per_s, hbm_share  bytes_per_call / scene_flow_us, and that over the 6.3 TB/s a streaming kernel achieves on an MI355X
  summary_us, colors_us  l4p_scene_flow_summary and l4p_scene_flow_colors, timed the same way
  torch_us             the plain-torch composition (torch.linalg.inv, matmul, grid_sample, where), same rotation
  max_diff_3d / _2d    largest difference between the two on pixels both call valid (sanity only; the tests hold the kernel to
                       the float64 restatement)

  python tools/scene_flow_time.py [--iters 500] [--repeats 7] [--sets 4]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from l4p_amd import _lib  # noqa: E402
from l4p_amd.ops import _p, _stream  # noqa: E402
from l4p_amd.utils import scene_flow as SF  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # B/s, a streaming copy on an MI355X


def demo_inputs(seed, B=1, T=64, H=224, W=224):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
    t = torch.arange(T, device="cuda").float().view(1, 1, T, 1, 1)
    depth = 2.5 + torch.sin(xx / 40 + 0.1 * t) * torch.cos(yy / 35) + 0.3 * torch.rand(B, 1, T, H, W, generator=g, device="cuda")
    flow = 3.0 * (torch.rand(B, 2, T, H, W, generator=g, device="cuda") - 0.5) + torch.tensor([1.5, -0.75], device="cuda").view(1, 2, 1, 1, 1)
    K = torch.eye(4, device="cuda").view(1, 4, 4, 1).repeat(B, 1, 1, T).clone()
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 200.0, 205.0, 111.5, 111.0
    P = torch.eye(4, device="cuda").view(1, 4, 4, 1).repeat(B, 1, 1, T).clone()
    a = 0.01 * torch.arange(T, device="cuda").float()
    P[:, 0, 0], P[:, 0, 2], P[:, 2, 0], P[:, 2, 2] = torch.cos(a), torch.sin(a), -torch.sin(a), torch.cos(a)
    P[:, 0, 3], P[:, 2, 3] = 0.05 * torch.arange(T, device="cuda").float(), 0.02 * torch.arange(T, device="cuda").float()
    mask = torch.randn(B, 1, T, H, W, generator=g, device="cuda")
    return depth.contiguous(), flow.contiguous(), P.contiguous(), K.contiguous(), mask


def torch_composition(depth, flow, P, K):
    """The definitions with torch ops (f32): returns scene [B,3,T,H,W], rigid, comp [B,2,T,H,W], valid [B,1,T,H,W] bool."""
    B, _, T, H, W = depth.shape
    HW = H * W
    Kt, Pt = K.permute(0, 3, 1, 2)[:, :, :3, :3], P.permute(0, 3, 1, 2)
    Kinv, Pinv = torch.linalg.inv(Kt), torch.linalg.inv(Pt)
    jj, ii = torch.meshgrid(torch.arange(H, device=depth.device).float(), torch.arange(W, device=depth.device).float(), indexing="ij")
    pix = torch.stack([ii, jj, torch.ones_like(ii)]).reshape(3, HW)
    X = Pt[:, :, :3, :3] @ ((Kinv @ pix) * depth.reshape(B, T, 1, HW)) + Pt[:, :, :3, 3:]  # [B, T, 3, HW]
    Xc, f = X[:, 1:], flow.permute(0, 2, 1, 3, 4).reshape(B, T, 2, HW)[:, 1:]
    q = pix[:2] + f
    inside = (q[:, :, 0] >= 0) & (q[:, :, 0] <= W - 1) & (q[:, :, 1] >= 0) & (q[:, :, 1] <= H - 1)
    grid = torch.stack([q[:, :, 0] / (W - 1) * 2 - 1, q[:, :, 1] / (H - 1) * 2 - 1], dim=-1).reshape(B * (T - 1), 1, HW, 2)
    dp = F.grid_sample(depth[:, 0, :-1].reshape(B * (T - 1), 1, H, W), grid, mode="bilinear", padding_mode="border",
                       align_corners=True).reshape(B, T - 1, 1, HW)
    qh = torch.cat([q, torch.ones_like(q[:, :, :1])], dim=2)
    Xp = Pt[:, :-1, :3, :3] @ ((Kinv[:, :-1] @ qh) * dp) + Pt[:, :-1, :3, 3:]
    S = Xp - Xc
    xc = Pinv[:, :-1, :3, :3] @ Xc + Pinv[:, :-1, :3, 3:]
    front = xc[:, :, 2] > 1e-6
    Rf = (Kt[:, :-1, :2] @ xc) / xc[:, :, 2:3] - pix[:2]
    C = f - Rf
    ok = inside & (depth.reshape(B, T, HW)[:, 1:] > 0) & (dp[:, :, 0] > 0) & front & torch.isfinite(S).all(2) & torch.isfinite(Rf).all(2) & \
        torch.isfinite(C).all(2)
    z = torch.zeros((), device=depth.device)

    def full(x, c):  # [B, T-1, c, HW] -> [B, c, T, H, W] with frame 0 zero
        x = torch.where(ok[:, :, None], x, z)
        return torch.cat([torch.zeros_like(x[:, :1]), x], dim=1).permute(0, 2, 1, 3).reshape(B, c, T, H, W)

    valid = torch.cat([torch.zeros_like(ok[:, :1]), ok], dim=1).reshape(B, 1, T, H, W)
    return full(S, 3), full(Rf, 2), full(C, 2), valid


def timed(fn, sets, iters, repeats):
    """Median over `repeats` event windows of the time per call, in microseconds; call k uses set k % sets."""
    for k in range(max(sets, 3)):
        fn(k % sets)
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(iters):
            fn(k % sets)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(us)), float(np.min(us)), float(np.max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    B, T, H, W = 1, 64, 224, 224
    lib, st = _lib.load(), _stream()
    ins = [demo_inputs(s) for s in range(args.sets)]
    f32 = dict(dtype=torch.float32, device="cuda")
    outs = [(torch.empty(B, 3, T, H, W, **f32), torch.empty(B, 2, T, H, W, **f32), torch.empty(B, 2, T, H, W, **f32),
             torch.empty(B, 1, T, H, W, dtype=torch.uint8, device="cuda")) for _ in range(args.sets)]
    ws = torch.empty(B * T * ((H * W + SF.SUMMARY_CHUNK - 1) // SF.SUMMARY_CHUNK) * 8, dtype=torch.float64, device="cuda")
    rows = torch.empty(B, T, 8, dtype=torch.float64, device="cuda")
    colors = torch.empty(B, T * H * W, 3, dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(SF.motion_lut()).cuda()
    s_max = torch.full((1,), 0.1, **f32)

    def fields(k):
        d, f, P, K, m = ins[k]
        s, r, c, v = outs[k]
        _lib.check(lib.l4p_scene_flow(st, _p(d), _p(f), _p(P), _p(K), _p(m), B, T, H, W, _p(s), _p(r), _p(c), _p(v)), "l4p_scene_flow")

    def summary(k):
        s, r, c, v = outs[k]
        _lib.check(lib.l4p_scene_flow_summary(st, _p(s), _p(c), _p(v), _p(ins[k][4]), B, T, H, W, 1.0, _p(ws), _p(rows)),
                   "l4p_scene_flow_summary")

    def colours(k):
        s, r, c, v = outs[k]
        _lib.check(lib.l4p_scene_flow_colors(st, _p(s), _p(v), _p(lut), B, T, H, W, _p(s_max), _p(colors)), "l4p_scene_flow_colors")

    res = {"shape": [B, T, H, W], "sets": args.sets, "iters": args.iters, "repeats": args.repeats}
    for name, fn in (("scene_flow", fields), ("summary", summary), ("colors", colours),
                     ("torch", lambda k: torch_composition(*ins[k][:4]))):
        med, lo, hi = timed(fn, args.sets, args.iters if name != "torch" else max(10, args.iters // 10), args.repeats)
        res[name + "_us"], res[name + "_us_min_max"] = round(med, 2), [round(lo, 2), round(hi, 2)]
    nbytes = 45 * B * T * H * W
    res["bytes_per_call"] = nbytes
    res["tb_per_s"] = round(nbytes / (res["scene_flow_us"] * 1e-6) / 1e12, 3)
    res["hbm_share"] = round(nbytes / (res["scene_flow_us"] * 1e-6) / HBM_ACHIEVABLE, 3)
    S, R, C, V = torch_composition(*ins[0][:4])
    s, r, c, v = outs[0]
    both = V & (v != 0)
    res["valid_fraction"] = round(float((v != 0).float().mean()), 4)
    res["valid_disagree"] = int((V != (v != 0)).sum())
    res["max_diff_3d"] = float(((S - s).abs() * both).max())
    res["max_diff_2d"] = float(torch.maximum(((R - r).abs() * both).max(), ((C - c).abs() * both).max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
