"""Tracking in both time directions, restated in NumPy / torch on the CPU: the definition the kernels of csrc/track_bidir.hip and
L4P_VideoMAE.forward are held to (DESIGN.md "Tracking in both time directions").

The reference's tracker is causal - a frame is estimated iff frame centre - query time >= 0 (sparse_heads.py:306-316) - and its
assert names the recipe for the other frames (sparse_heads.py:242-245): "Run twice, with and without video flipping, and then combine
outputs".  For a clip of T frames and a query (tq, x, y):
  * the forward pass is the causal pass on the clip as it is;
  * the reversed pass is the causal pass on the time-flipped clip - its frame f' is frame T-1-f' of the input - with the query
    ((float)T - tq, x, y), one f32 subtraction, the point labels unchanged;
  * output frame g of track n is the forward pass's iff ((float)g + 0.5f) - tq[n] >= 0 in f32 (the expression of
    track_prepare_kernel), else the reversed pass's at frame T-1-g; traj (both channels), vis and depth alike.
Everything here is float32 arithmetic, operation by operation, so the kernels can be compared bit for bit."""
import numpy as np
import torch

KEYS = ("track_2d_traj_est_bn2t", "track_2d_vis_est_bn1t", "track_2d_depth_est_bn1t")
FILL = {"track_2d_traj_est_bn2t": 0.0, "track_2d_vis_est_bn1t": -10.0, "track_2d_depth_est_bn1t": 0.0}


def edge_times(T: int):
    """Query times at the edges of the rule for a clip of T frames: on the first frame's centre, one f32 step to either side of it,
    between two frames, on the last frame's centre, past the end, not a number."""
    return [0.5, 0.49999997, 0.50000006, 1.0, T - 0.5, T + 0.5, float("nan")]


def time_reverse(x: np.ndarray) -> np.ndarray:
    """[outer][T][inner] with the T axis reversed."""
    return np.ascontiguousarray(x[:, ::-1])


def flip_queries(q, T: int):
    """[..., 3] float32 -> the queries of the reversed pass: ((float)T - tq, x, y)."""
    if torch.is_tensor(q):
        out = q.to(torch.float32).clone()
        out[..., 0] = torch.tensor(float(T), dtype=torch.float32) - out[..., 0]
        return out
    out = np.array(q, dtype=np.float32, copy=True)
    out[..., 0] = np.float32(T) - out[..., 0]
    return out


def forward_owned(tq, T: int) -> np.ndarray:
    """tq [...] float32 -> bool [..., T]: frame g is the forward pass's.  ((float)g + 0.5f) - tq >= 0, NaN compares false."""
    tq = np.asarray(tq, dtype=np.float32)
    centre = np.arange(T, dtype=np.float32) + np.float32(0.5)
    with np.errstate(invalid="ignore"):
        return (centre - tq[..., None]).astype(np.float32) >= np.float32(0)


def reversed_pass_valid(tq, T: int) -> np.ndarray:
    """bool [..., T], indexed by the frame g of the INPUT clip: the reversed pass estimates that frame (its causal rule on its
    own frame T-1-g and the flipped query time)."""
    tq_rev = np.float32(T) - np.asarray(tq, dtype=np.float32)
    return forward_owned(tq_rev, T)[..., ::-1]


def need_count(tq) -> int:
    """Queries with at least one frame before them: (0.5f - tq) < 0."""
    tq = np.asarray(tq, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return int(((np.float32(0.5) - tq).astype(np.float32) < np.float32(0)).sum())


def merge(q_bn3, fwd, rev, mode: int = 0):
    """q [B, N, 3]; fwd / rev: (traj [B, N, 2, T], vis [B, N, 1, T], depth [B, N, 1, T]) as arrays or CPU tensors, the reversed ones
    in the reversed clip's own frame order.  mode 1: no forward pass (fwd may be None), forward-owned frames get the fill values.
    -> the three merged arrays."""
    rev = [np.asarray(t, dtype=np.float32) for t in rev]
    T = rev[0].shape[-1]
    own = forward_owned(np.asarray(q_bn3, dtype=np.float32)[..., 0], T)[:, :, None, :]  # [B, N, 1, T]
    out = []
    for i, (key, r) in enumerate(zip(KEYS, rev)):
        f = np.asarray(fwd[i], dtype=np.float32) if mode == 0 else np.full_like(r, FILL[key])
        out.append(np.where(own, f, r[..., ::-1]).astype(np.float32))
    return out


def flip_batch(batch: dict) -> dict:
    """The batch of the reversed pass: clip flipped in time, queries mapped, everything else as it is."""
    T = batch["rgb_b3thw"].shape[2]
    out = dict(batch)
    out["rgb_b3thw"] = batch["rgb_b3thw"].flip(2).contiguous()
    out["track_2d_pointquerries_bn3"] = flip_queries(batch["track_2d_pointquerries_bn3"], T)
    return out


def compose(run_forward, batch: dict, mode: int = 0) -> dict:
    """The merged result from ANY runner of the causal pass: ``run_forward(batch) -> {key: tensor}`` (estimation_directions [1])."""
    rev = run_forward(flip_batch(batch))
    fwd = run_forward(batch) if mode == 0 else None
    cpu = lambda o: [o[k].detach().float().cpu().numpy() for k in KEYS]  # noqa: E731
    merged = merge(batch["track_2d_pointquerries_bn3"].detach().float().cpu().numpy(), cpu(fwd) if fwd is not None else None, cpu(rev), mode)
    return {k: torch.from_numpy(m) for k, m in zip(KEYS, merged)}
