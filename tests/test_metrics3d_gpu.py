"""GPU: l4p_metric_tracks3d, l4p_metric_depth_full and the opt-in arguments of L4PMetrics against the numpy restatement
(tests/metrics3d_restate.py).  Counts, count-ratio metrics and the median / query scales are EQUAL; the f64-summed columns are
within a relative 1e-9 (the same terms added in another order: n <= 2^20 terms bound the difference by n 2^-53 = 1.2e-10, and the
f64 log of the two math libraries differs by a few 1e-16 per term); silog, a difference of two moments, within 1e-8 where the
variance is at least 0.3 of the second moment."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics3d_restate as R3
from tests import metrics_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
THR = (1, 2, 4, 8, 16)
SMALL, LARGE = (2, 3 * 5 * 7), (1, 16 * 224 * 224)
SUM_RTOL = 1e-9
TRACK_SHAPES = [(2, 3, 5, (224, 224)), (1, 70, 24, (180, 320)), (1, 17, 130, (224, 224))]
TRACK_IDS = ["B2N3T5", "B1N70T24_HneW", "B1N17T130"]


def M():
    import l4p_amd.metrics as m

    return m


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def same(a, b):
    """equal, NaN == NaN"""
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def close(got, want, rtol=SUM_RTOL):
    return same(got, want) or abs(got - want) <= rtol * abs(want)


@functools.lru_cache(maxsize=None)
def track_case(B, N, T, hw, per_track):
    return R3.make_track3d_case(B, N, T, seed=7 + N, hw=hw, per_track=per_track)


@functools.lru_cache(maxsize=None)
def track_want(B, N, T, hw, per_track, scale, with_valid=True):
    c = track_case(B, N, T, hw, per_track)
    return [R3.tracks3d_of_case(c, b, scale, "case" if with_valid else None) for b in range(B)]


@functools.lru_cache(maxsize=None)
def dense_case(B, n):
    return R.make_dense_case(B, n, seed=100 + B + n % 97)


def run_tracks3d(c, scale, valid="case"):
    return M().track3d_metrics(dev(c["traj_est"]), dev(c["depth_est"]), dev(c["traj_gt"]), dev(c["depth_gt"]), dev(c["vis_logit"]),
                               dev(c["vis_gt"]), dev(c["valid"]) if valid == "case" else None, dev(c["queries"]), dev(c["intrinsics"]),
                               c["hw"], scale)


def check_track_rows(rows, want_list, tag=""):
    m = M()
    rows = rows.cpu().numpy()
    for b, want in enumerate(want_list):
        for name, col in {**m.TRACK_RAW, **m.TRACK_METRICS, "scale": 31}.items():
            got, w = float(rows[b, col]), float(want[name])
            print(f"{tag} clip {b} {name}: kernel {got!r} restatement {w!r}")
            assert same(got, w), (b, name, got, w)


@pytest.mark.parametrize("B,N,T,hw", TRACK_SHAPES, ids=TRACK_IDS)
@pytest.mark.parametrize("scale", R3.SCALES)
def test_tracks3d_match_restatement(B, N, T, hw, scale):
    per_track = scale in ("track_median", "query")  # the hidden scale is one per track where the mode can recover that
    c = track_case(B, N, T, hw, per_track)
    want = track_want(B, N, T, hw, per_track, scale)
    # what makes a pass mean something, on the restatement alone
    clip = track_want(B, N, T, hw, False, "median")
    for w in clip:
        par = set(int(x) % 2 for x in w["eligible_per_track"] if x > 0)
        assert par == {0, 1} or N == 3  # even and odd eligible counts: both lower-median ranks
        assert (w["eligible_per_track"] == 0).any()  # a track with no eligible frame
        assert w["eligible"][0, 1] and w["eligible"][0, 3] and w["ratios"][0, 1] == w["ratios"][0, 3]  # a tie
        if N > 3:
            assert 0 < w["count_within_1"] < w["count_within_2"] < w["count_within_4"] < w["count_within_8"] < w["count_within_16"] \
                < w["count_gt_visible"]
    if N > 3:
        assert all(w["count_within_16"] == 0 for w in track_want(B, N, T, hw, False, "none"))  # the scale is what earns the score
    assert all(np.isnan(w["track_scales"]).any() for w in track_want(B, N, T, hw, True, "query"))
    check_track_rows(run_tracks3d(c, scale), want, scale)
    if scale in ("track_median", "query"):
        assert all(0 < w["scale"] < N for w in want)


@pytest.mark.parametrize("scale", R3.SCALES)
def test_tracks3d_without_valid_and_same_bits_twice(scale):
    B, N, T, hw = TRACK_SHAPES[1]
    c = track_case(B, N, T, hw, True)
    want = track_want(B, N, T, hw, True, scale, False)
    zg = c["depth_gt"].reshape(B, N, T)
    ok_z = np.isfinite(zg) & (zg > 0)
    ok_z[0, np.arange(N), np.floor(c["queries"][0, :, 0]).astype(int)] = False
    assert want[0]["count"] == int(ok_z.sum()) < N * (T - 1)  # every frame but the query frame and the bad gt depths
    rows = run_tracks3d(c, scale, None)
    check_track_rows(rows, want, scale + " valid=None")
    again = run_tracks3d(c, scale, None)
    assert torch.equal(rows.view(torch.int64), again.view(torch.int64))


def test_refusals():
    from l4p_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")  # stands in for every pointer: a refused call launches nothing
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    big = 1 << 31

    def refused(name, rc):
        msg = lib.l4p_last_error().decode()
        assert rc == -1 and name in msg, (name, rc, msg)

    # l4p_metric_tracks3d_ws_bytes: 0 for what the entry refuses
    wsb = lib.l4p_metric_tracks3d_ws_bytes
    need = {k: int(wsb(1, 3, 5, k)) for k in range(4)}
    assert all(v > 0 for v in need.values()) and need[1] > need[0] and need[2] > need[0]
    for args in [(0, 3, 5, 1), (1, 0, 5, 1), (1, 3, 0, 1), (1, 3, 5, -1), (1, 3, 5, 4), (4, 1 << 15, 1 << 14, 0), (1 << 11, 1 << 10, 1 << 10, 0)]:
        assert wsb(*args) == 0, args
    assert wsb(1, 1 << 15, (1 << 16) - 1, 0) > 0  # B N T = 2^31 - 2^15 is in range
    t3d = lib.l4p_metric_tracks3d

    def call(ptrs=None, shape=(1, 3, 5, 8, 8), scale=1, ws_bytes=1 << 19):
        a = [p] * 12 if ptrs is None else ptrs  # nine inputs, ws, counts, out
        return t3d(st, *a[:9], *shape, scale, a[9], ws_bytes, a[10], a[11])

    for shape in [(0, 3, 5, 8, 8), (1, 0, 5, 8, 8), (1, 3, 0, 8, 8), (1, 3, 5, 0, 8), (1, 3, 5, 8, 0), (4, 1 << 15, 1 << 14, 8, 8)]:
        refused("l4p_metric_tracks3d", call(shape=shape, ws_bytes=1 << 62))
    for scale in (-1, 4):
        refused("l4p_metric_tracks3d", call(scale=scale))
    for k in range(12):
        ptrs = [p] * 12
        ptrs[k] = None
        if k == 6:
            continue  # valid may be NULL
        refused("l4p_metric_tracks3d", call(ptrs))
    for k in range(4):
        refused("l4p_metric_tracks3d", call(scale=k, ws_bytes=need[k] - 1))
    # l4p_metric_depth_full and its workspace size
    dwb = lib.l4p_metric_depth_full_ws_bytes
    ws = int(dwb(1, 105, 1))
    assert ws > 0 and dwb(1, 105, 3) > 0 and dwb(0, 105, 1) == 0 and dwb(1, 0, 1) == 0 and dwb(1, 105, 4) == 0 and dwb(1, 105, -1) == 0
    assert dwb(1, big, 0) == 0 and dwb(2, 1 << 30, 0) == 0
    full = lib.l4p_metric_depth_full
    for args in [(0, 105, 1), (1, 0, 1), (1, big, 1), (2, 1 << 30, 0)]:
        refused("l4p_metric_depth_full", full(st, p, p, p, args[0], args[1], args[2], 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, 4, 1e-3, 80.0, p, 1 << 19, p))  # unknown alignment
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, -1, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, 3, 0.0, 80.0, p, 1 << 19, p))  # dmin
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, 3, 2.0, 1.0, p, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, None, p, p, 1, 105, 3, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, p, None, p, 1, 105, 3, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, 3, 1e-3, 80.0, None, 1 << 19, p))
    refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, 3, 1e-3, 80.0, p, 1 << 19, None))
    for k in range(4):
        refused("l4p_metric_depth_full", full(st, p, p, p, 1, 105, k, 1e-3, 80.0, p, int(dwb(1, 105, k)) - 1, p))
    # the 16-column entry still refuses the new alignment
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 3, 1e-3, 80.0, p, 1 << 19, p))
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0  # nothing was launched
    m = M()
    z = torch.zeros(1, 3, 2, 5, device="cuda")
    with pytest.raises(ValueError, match="intrinsics"):
        m.track3d_metrics(z, z[:, :, :1], z, z[:, :, :1], z[:, :, :1], z[:, :, :1], None, z[:, :, 0, :3], torch.zeros(1, 3, 3, 5), (8, 8))
    with pytest.raises(ValueError, match="depth_est"):
        m.track3d_metrics(z, z[:, :, :1, :4], z, z[:, :, :1], z[:, :, :1], z[:, :, :1], None, z[:, :, 0, :3], torch.zeros(1, 4, 4, 5), (8, 8))


DEPTH_SUMMED = ("sum_abs_rel", "sum_sq", "abs_rel", "rmse", "sum_sq_rel", "sum_log", "sum_log_sq", "sum_abs_log", "sq_rel", "rmse_log",
                "log10")


def check_depth_full(rows, c, B, mode, valid="case", dmin=1e-3, dmax=80.0):
    """rows [B, 24] against the restatement under the kernel's own (s, t); returns the restated clips"""
    m = M()
    host = rows.cpu().numpy()
    cols = {**m.DEPTH_RAW, **m.DEPTH_METRICS, **m.DEPTH_FULL_RAW, **m.DEPTH_FULL_METRICS}
    wants = []
    for b in range(B):
        v = c["depth_valid"][b] if valid == "case" else valid
        s_ref, t_ref = R3.depth_full_align(c["depth_est"][b], c["depth_gt"][b], v, mode, dmin, dmax)
        s, t = host[b, 11], host[b, 12]
        print(f"clip {b} {mode}: (s, t) kernel ({s!r}, {t!r}) restatement ({float(s_ref)!r}, {float(t_ref)!r})")
        if mode in ("lstsq", "lstsq_inv"):  # normal equations in f64 against numpy's SVD: they meet at the f32 rounding
            assert abs(s - float(s_ref)) <= 1e-6 * abs(float(s_ref)) and abs(t - float(t_ref)) <= 1e-6 * abs(float(t_ref))
        else:
            assert s == float(s_ref) and t == float(t_ref)
        assert F(s) == s and F(t) == t  # f32 values
        w = R3.depth_full_errors(c["depth_est"][b], c["depth_gt"][b], v, F(s), F(t), mode == "lstsq_inv", dmin, dmax)
        wants.append(w)
        for name, col in cols.items():
            if name == "silog":
                continue  # a difference of two moments: below
            got = float(host[b, col])
            print(f"clip {b} {mode} {name}: kernel {got!r} restatement {float(w[name])!r}")
            if name in DEPTH_SUMMED:
                assert close(got, float(w[name])), (b, name, got, w[name])
            else:
                assert same(got, float(w[name])), (b, name, got, w[name])
        print(f"clip {b} {mode} silog: kernel {float(host[b, 20])!r} restatement {w['silog']!r}")
        assert close(float(host[b, 20]), w["silog"], 1e-8)
        assert np.isnan(host[b, 21:24]).all()
    return wants


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["n105", "n802816"])
@pytest.mark.parametrize("mode", ["none", "median", "lstsq", "lstsq_inv"])
def test_depth_full_matches_restatement(shape, mode):
    B, n = shape
    c = dense_case(B, n)
    m = M()
    est, gt, valid = dev(c["depth_est"]), dev(c["depth_gt"]), dev(c["depth_valid"])
    rows = m.depth_metrics_full(est, gt, valid, mode)
    assert rows.shape == (B, 24) and rows.dtype == torch.float64
    if mode != "lstsq_inv":  # the first 13 columns are the depth entry's, bit for bit
        old = m.depth_metrics(est, gt, valid, mode)
        assert torch.equal(rows[:, :13].view(torch.int64), old[:, :13].view(torch.int64))
    wants = check_depth_full(rows, c, B, mode)
    for w in wants:
        assert 0.5 * n < w["count"] < 0.8 * n
        mean_abs_l, mean_ll = w["sum_abs_log"] / w["count"], w["sum_log_sq"] / w["count"]
        print(f"{mode}: mean |l| {mean_abs_l!r}, var / mean l*l {w['log_var'] / mean_ll!r}")
        assert mean_abs_l > 1e-3  # the log sums are not rounding noise
        assert w["log_var"] >= 0.3 * mean_ll  # silog's difference of moments keeps its digits
    again = m.depth_metrics_full(est, gt, valid, mode)
    assert torch.equal(rows.view(torch.int64), again.view(torch.int64))


def test_depth_full_clamped_in_disparity_and_empty_clips():
    B, n = SMALL
    c = dense_case(B, n)
    m = M()
    est, gt = dev(c["depth_est"]), dev(c["depth_gt"])
    # no valid array, another range.  (1.5, 6.0), not (1.0, 6.0): a fit with a shift pulls towards the mean, and in (1.0, 6.0) the
    # restatement finds no element of this case beyond either end in inverse depth; in (1.5, 6.0) each clip has one
    rows = m.depth_metrics_full(est, gt, None, "lstsq_inv", 1.5, 6.0)
    wants = check_depth_full(rows, c, B, "lstsq_inv", None, 1.5, 6.0)
    assert all(w["clamped_inv"] >= 1 for w in wants)  # the clamp in inverse depth is reached
    # a clip with no valid element: count 0, sums 0, NaN metrics and alignment; the other clip is untouched
    valid = c["depth_valid"].copy()
    valid[1] = 0
    for mode in ("none", "median", "lstsq", "lstsq_inv"):
        rows = m.depth_metrics_full(est, gt, dev(valid), mode).cpu().numpy()
        ref = m.depth_metrics_full(est, gt, dev(c["depth_valid"]), mode).cpu().numpy()
        assert np.array_equal(rows[0], ref[0], equal_nan=True)
        assert rows[1, 0] == 0 and (rows[1, 1:6] == 0).all() and (rows[1, 13:17] == 0).all()
        assert np.isnan(rows[1, 6:11]).all() and np.isnan(rows[1, 17:24]).all()
        assert mode == "none" or np.isnan(rows[1, 11])
    # one valid element: the least squares in inverse depth has no solution and scores nothing
    valid[:] = 0
    ok = np.flatnonzero(R.depth_valid(c["depth_est"][0], c["depth_gt"][0], None, 1e-3, 80.0))
    valid[0, ok[0]] = 1
    row = m.depth_metrics_full(est, gt, dev(valid), "lstsq_inv").cpu().numpy()[0]
    assert row[0] == 0 and math.isnan(row[11]) and math.isnan(row[12]) and math.isnan(row[18])


def five_task_inputs_3d(B=2, T=5, H=6, W=9, N=4, seed=3):
    """a small batch / out pair with all five tasks on the device, as tests/test_metrics_gpu.py builds it, plus the track depths of
    both sides and per-frame intrinsics"""
    n = T * H * W
    c = R.make_dense_case(B, n, seed)
    tr = R3.make_track3d_case(B, N, T, seed, hw=(H, W))
    cams = [R.make_camera_case(T, seed + b) for b in range(B)]
    batch = {
        "rgb_b3thw": torch.zeros(B, 3, T, H, W, device="cuda"),
        "depth_b1thw": dev(c["depth_gt"]).reshape(B, 1, T, H, W), "depth_valid_b1thw": dev(c["depth_valid"]).reshape(B, 1, T, H, W) > 0.5,
        "flow_2d_backward_b2thw": dev(c["flow_gt"]).reshape(B, 2, T, H, W),
        "flow_2d_backward_valid_b2thw": dev(c["flow_valid"]).reshape(B, 2, T, H, W),
        "dyn_mask_b1thw": dev(c["mask_gt"]).reshape(B, 1, T, H, W), "dyn_mask_valid_b1thw": dev(c["mask_valid"]).reshape(B, 1, T, H, W),
        "track_2d_traj_bn2t": dev(tr["traj_gt"]), "track_2d_vis_bn1t": dev(tr["vis_gt"]), "track_2d_valid_bn1t": dev(tr["valid"]),
        "track_2d_pointquerries_bn3": dev(tr["queries"]), "track_2d_depth_bn1t": dev(tr["depth_gt"]),
        "intrinsics_b44t": dev(tr["intrinsics"]),
        "extrinsics_b44t": dev(np.stack([x[1] for x in cams])),
    }
    out = {
        "depth_est_b1thw": dev(c["depth_est"]).reshape(B, 1, T, H, W),
        "flow_2d_backward_est_b2thw": dev(c["flow_est"]).reshape(B, 2, T, H, W),
        "dyn_mask_est_b1thw": dev(c["mask_logit"]).reshape(B, 1, T, H, W),
        "track_2d_traj_est_bn2t": dev(tr["traj_est"]), "track_2d_vis_est_bn1t": dev(tr["vis_logit"]),
        "track_2d_depth_est_bn1t": dev(tr["depth_est"]).to(torch.float64),
        "traj3d_est_b16t": dev(np.stack([x[0] for x in cams])),
    }
    return batch, out, c, tr


def test_module_opt_in_keys_values_and_no_host_sync():
    m = M()
    B = 2
    batch, out, c, tr = five_task_inputs_3d()
    old_keys = {f"depth_{k}" for k in m.DEPTH_METRICS} | {f"flow_{k}" for k in m.FLOW_METRICS} | \
        {f"dyn_mask_{k}" for k in m.MASK_METRICS} | {f"track_2d_{k}" for k in m.TRACK_METRICS} | {f"camray_{k}" for k in m.CAM_METRICS}
    # default arguments: exactly the old keys, although the batch now carries track depths and intrinsics
    met0, ex0 = m.L4PMetrics()(batch, out)
    assert set(met0) == old_keys and not any(k.startswith("track_3d") or "log" in k or "sq_rel" in k for k in ex0)
    mod = m.L4PMetrics(track_3d="median", depth_log_errors=True, depth_align="lstsq_inv")
    met, ex = mod(batch, out)
    new_keys = {f"depth_{k}" for k in m.DEPTH_FULL_METRICS} | {f"track_3d_{k}" for k in m.TRACK_METRICS}
    assert set(met) == old_keys | new_keys
    for k, v in met.items():
        assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda, k
    new_extras = {k + "_per_clip" for k in new_keys} | {f"depth_{k}" for k in m.DEPTH_FULL_RAW} | {f"track_3d_{k}" for k in m.TRACK_RAW} | \
        {"track_3d_scale"}
    assert set(ex) == set(ex0) | new_extras
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (B,) for v in ex.values())
    # everything that does not depend on the depth alignment is what the default module gives
    for k in ex0:
        if not k.startswith("depth_"):
            assert torch.equal(ex[k].view(torch.int64), ex0[k].view(torch.int64)), k
    # values: 3D tracks equal, depth under the kernel's own (s, t)
    wt = [R3.tracks3d_of_case(tr, b, "median") for b in range(B)]
    for name in list(m.TRACK_METRICS) + list(m.TRACK_RAW):
        key = f"track_3d_{name}_per_clip" if name in m.TRACK_METRICS else f"track_3d_{name}"
        assert all(same(float(ex[key][b]), float(wt[b][name])) for b in range(B)), name
    assert [float(x) for x in ex["track_3d_scale"].cpu()] == [w["scale"] for w in wt]
    assert same(float(met["track_3d_average_jaccard"]), float(torch.nanmean(ex["track_3d_average_jaccard_per_clip"]).to(torch.float32)))
    for b in range(B):
        s, t = float(ex["depth_align_scale"][b]), float(ex["depth_align_shift"][b])
        s_ref, t_ref = R3.depth_full_align(c["depth_est"][b], c["depth_gt"][b], c["depth_valid"][b], "lstsq_inv")
        assert abs(s - float(s_ref)) <= 1e-6 * abs(float(s_ref)) and abs(t - float(t_ref)) <= 1e-6 * abs(float(t_ref))
        w = R3.depth_full_errors(c["depth_est"][b], c["depth_gt"][b], c["depth_valid"][b], F(s), F(t), True)
        assert float(ex["depth_count"][b]) == w["count"] and float(ex["depth_delta1_per_clip"][b]) == w["delta1"]
        for name in ("abs_rel", "sq_rel", "rmse_log", "log10"):
            assert close(float(ex[f"depth_{name}_per_clip"][b]), w[name]), name
        assert close(float(ex["depth_silog_per_clip"][b]), w["silog"], 1e-8)
    # track_3d follows the tasks filter of track_2d; a missing side skips it silently; depth_log_errors alone keeps the alignment
    met2, _ = m.L4PMetrics(tasks=["flow", "camray"], track_3d="median")(batch, out)
    assert {k.split("_")[0] for k in met2} == {"flow", "camray"}
    met3, _ = mod({k: v for k, v in batch.items() if k != "intrinsics_b44t"}, out)
    assert set(met3) == old_keys | {f"depth_{k}" for k in m.DEPTH_FULL_METRICS}
    met4, ex4 = m.L4PMetrics(depth_log_errors=True)(batch, out)
    assert set(met4) == old_keys | {f"depth_{k}" for k in m.DEPTH_FULL_METRICS}
    assert torch.equal(ex4["depth_abs_rel_per_clip"].view(torch.int64), ex0["depth_abs_rel_per_clip"].view(torch.int64))
    # no host synchronisation
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device="cuda").item()
            implemented = False
        except RuntimeError:
            implemented = True
        if implemented:
            _, ex5 = mod(batch, out)
            m.L4PMetrics(track_3d="track_median")(batch, out)
            m.L4PMetrics(track_3d="query", depth_log_errors=True)(batch, out)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not implemented:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a synchronising call in this torch build on ROCm")
    for k in ex:
        assert torch.equal(ex5[k].view(torch.int64), ex[k].view(torch.int64)), k


def test_end_to_end_mini_test_step_track_3d():
    from l4p_amd.models.utils import build_model
    from l4p_amd.weights import ModelCfg, seeded_state_dict
    from tests.golden_utils import make_batch

    m = M()
    cfg = ModelCfg.mini()
    model = build_model(os.path.join(ROOT, "configs", "model.yaml"), max_queries=8, precision="32-true", model_cfg=cfg)
    for h in model.l4p_model.task_heads.values():
        if hasattr(h, "hooks_idx"):
            h.hooks_idx = list(cfg.hooks)
    model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(cfg).items()})
    model = model.eval()
    T, N = 24, 8
    batch = make_batch(T, N)
    rng = np.random.default_rng(5)
    q = batch["track_2d_pointquerries_bn3"]
    batch["track_2d_traj_bn2t"] = q[:, :, 1:, None].repeat(1, 1, 1, T) + torch.from_numpy(rng.uniform(-3, 3, (1, N, 2, T)).astype(F))
    batch["track_2d_vis_bn1t"] = torch.from_numpy(rng.uniform(size=(1, N, 1, T)) > 0.3)
    batch["track_2d_valid_bn1t"] = torch.arange(T)[None, None, None, :] >= torch.floor(q[:, :, 0])[:, :, None, None]
    batch["track_2d_depth_bn1t"] = torch.from_numpy(rng.uniform(1.0, 8.0, (1, N, 1, T)).astype(F))
    K = batch["intrinsics_b44t"].clone()  # per-frame intrinsics: the focal length drifts by up to 5 %
    K[:, 0, 0] *= torch.from_numpy(1.0 + rng.uniform(-0.05, 0.05, (1, T)).astype(F))
    K[:, 1, 1] = 1.1 * K[:, 0, 0]
    batch["intrinsics_b44t"] = K
    gt = {k: batch[k][0].clone().numpy() for k in ("track_2d_traj_bn2t", "track_2d_depth_bn1t", "track_2d_vis_bn1t", "track_2d_valid_bn1t",
                                                   "track_2d_pointquerries_bn3", "intrinsics_b44t")}
    model.metrics_module = m.L4PMetrics(track_3d="track_median")
    with torch.no_grad():
        res = model.test_step(batch, 0)
    out = {k: v.float().cpu().numpy() for k, v in res["out"].items() if k.startswith("track_2d_") and torch.is_tensor(v)}
    want = R3.tracks3d(out["track_2d_traj_est_bn2t"][0], out["track_2d_depth_est_bn1t"][0], gt["track_2d_traj_bn2t"],
                       gt["track_2d_depth_bn1t"], out["track_2d_vis_est_bn1t"][0], gt["track_2d_vis_bn1t"], gt["track_2d_valid_bn1t"],
                       gt["track_2d_pointquerries_bn3"], gt["intrinsics_b44t"], (224, 224), "track_median")
    log = model.last_log
    assert want["count"] > 0 and want["count_gt_visible"] > 0
    for name in m.TRACK_METRICS:
        v = log[f"scalars/val/track_3d_{name}"]
        print(name, float(v), want[name])
        assert v.dtype == torch.float32 and v.dim() == 0 and same(float(v), float(F(want[name]))), name
    assert "scalars/val/track_2d_average_jaccard" in log and not any("sq_rel" in k for k in log)
    # seeded weights track nothing, so the step above compares zeros wherever a distance counts.  A second step whose ground truth
    # is made FROM the estimate: depth 1.25 x the estimate (a per-track scale to recover), positions 0.3 .. 30 px off
    ze = out["track_2d_depth_est_bn1t"]
    usable = np.isfinite(ze) & (ze > 0)
    zg = np.where(usable, F(1.25) * np.where(usable, ze, F(1)), F(2)).astype(F)
    off = np.asarray([0.3, 1.5, 3.0, 6.0, 12.0, 30.0], F)[rng.integers(0, 6, (1, N, 1, T))]
    tg = (np.nan_to_num(out["track_2d_traj_est_bn2t"], nan=0.0, posinf=0.0, neginf=0.0) + off * np.asarray([1.0, 0.0], F)[None, None, :, None])
    batch2 = dict(batch)
    batch2["track_2d_depth_bn1t"], batch2["track_2d_traj_bn2t"] = torch.from_numpy(zg), torch.from_numpy(tg.astype(F))
    with torch.no_grad():
        res = model.test_step(batch2, 1)
    out = {k: v.float().cpu().numpy() for k, v in res["out"].items() if k.startswith("track_2d_") and torch.is_tensor(v)}
    want = R3.tracks3d(out["track_2d_traj_est_bn2t"][0], out["track_2d_depth_est_bn1t"][0], tg[0].astype(F), zg[0],
                       out["track_2d_vis_est_bn1t"][0], gt["track_2d_vis_bn1t"], gt["track_2d_valid_bn1t"],
                       gt["track_2d_pointquerries_bn3"], gt["intrinsics_b44t"], (224, 224), "track_median")
    print("second step:", [want[f"count_within_{t}"] for t in THR], want["count_gt_visible"], want["track_scales"])
    assert want["count_within_1"] < want["count_within_16"] < want["count_gt_visible"] and want["count_within_16"] > 0
    for name in m.TRACK_METRICS:
        v = model.last_log[f"scalars/val/track_3d_{name}"]
        assert same(float(v), float(F(want[name]))), (name, float(v), want[name])
