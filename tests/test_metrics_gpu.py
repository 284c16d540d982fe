"""GPU: the evaluation-metric kernels (csrc/metrics.hip) and L4PMetrics (l4p_amd/metrics.py) against the numpy restatement
(tests/metrics_restate.py).  Counts, count-ratio metrics and the median scale are EQUAL; the f64-summed metrics are within a
relative 1e-9 (both sides add the same f32 terms in f64 in another order: n <= 2^20 terms bound the difference by n 2^-53 =
1.2e-10 of the sum of magnitudes); the camera metrics are f64 on both sides (relative 1e-9 + absolute 1e-12)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SMALL, LARGE = (2, 3 * 5 * 7), (1, 16 * 224 * 224)  # (B, n): n = 105 is under one workgroup, odd, clip 1 starts off a 16-byte line
SUM_RTOL = 1e-9


def M():
    import l4p_amd.metrics as m

    return m


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def dense_case(B, n):
    return R.make_dense_case(B, n, seed=100 + B + n % 97)


def same(a, b):
    """equal, NaN == NaN"""
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def close(got, want, rtol=SUM_RTOL):
    return same(got, want) or abs(got - want) <= rtol * abs(want)


def check_rows(rows, want_list, raw_cols, metric_cols, summed=()):
    rows = rows.cpu().numpy()
    for b, want in enumerate(want_list):
        for name, col in {**raw_cols, **metric_cols}.items():
            if name not in want:
                continue
            got, w = float(rows[b, col]), float(want[name])
            print(f"clip {b} {name}: kernel {got!r} restatement {w!r}")
            if name in summed:
                assert close(got, w), (b, name, got, w)
            else:
                assert same(got, w), (b, name, got, w)


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["n105", "n802816"])
@pytest.mark.parametrize("mode", ["median", "none", "lstsq"])
def test_depth_matches_restatement(shape, mode):
    B, n = shape
    c = dense_case(B, n)
    m = M()
    rows = m.depth_metrics(dev(c["depth_est"]), dev(c["depth_gt"]), dev(c["depth_valid"]), mode)
    host = rows.cpu().numpy()
    want = []
    for b in range(B):
        s_ref, t_ref = R.depth_align(c["depth_est"][b], c["depth_gt"][b], c["depth_valid"][b], mode)
        s, t = host[b, 11], host[b, 12]
        print(f"clip {b} {mode}: (s, t) kernel ({s!r}, {t!r}) restatement ({float(s_ref)!r}, {float(t_ref)!r})")
        if mode == "lstsq":  # the kernel solves the normal equations in f64, numpy by SVD: they meet at the f32 rounding
            assert abs(s - float(s_ref)) <= 1e-6 * abs(float(s_ref)) and abs(t - float(t_ref)) <= 1e-6 * abs(float(t_ref))
        else:
            assert s == float(s_ref) and t == float(t_ref)
        assert F(s) == s and F(t) == t  # f32 values
        want.append(R.depth_errors(c["depth_est"][b], c["depth_gt"][b], c["depth_valid"][b], F(s), F(t)))
        assert 0.5 * n < want[-1]["count"] < 0.8 * n  # about 30 % invalid
    check_rows(rows, want, m.DEPTH_RAW, m.DEPTH_METRICS, summed=("sum_abs_rel", "sum_sq", "abs_rel", "rmse"))


def test_depth_without_valid_and_other_range():
    B, n = SMALL
    c = dense_case(B, n)
    m = M()
    rows = m.depth_metrics(dev(c["depth_est"]), dev(c["depth_gt"]), None, "median", 1.0, 6.0)
    want = [R.depth(c["depth_est"][b], c["depth_gt"][b], None, "median", 1.0, 6.0) for b in range(B)]
    check_rows(rows, want, m.DEPTH_RAW, m.DEPTH_METRICS, summed=("sum_abs_rel", "sum_sq", "abs_rel", "rmse"))
    assert [float(x) for x in rows[:, 11].cpu()] == [w["align_scale"] for w in want]


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["n105", "n802816"])
def test_flow_and_mask_match_restatement(shape):
    B, n = shape
    c = dense_case(B, n)
    m = M()
    rows = m.flow_metrics(dev(c["flow_est"]), dev(c["flow_gt"]), dev(c["flow_valid"]))
    want = [R.flow(c["flow_est"][b], c["flow_gt"][b], c["flow_valid"][b]) for b in range(B)]
    assert all(0.5 * n < w["count"] < 0.8 * n for w in want)
    check_rows(rows, want, m.FLOW_RAW, m.FLOW_METRICS, summed=("sum_epe", "epe"))
    rows = m.mask_metrics(dev(c["mask_logit"]), dev(c["mask_gt"]), dev(c["mask_valid"]))
    want = [R.mask(c["mask_logit"][b], c["mask_gt"][b], c["mask_valid"][b]) for b in range(B)]
    check_rows(rows, want, m.MASK_RAW, m.MASK_METRICS)
    if shape == SMALL:  # no valid arrays: all valid
        rows = m.flow_metrics(dev(c["flow_est"]), dev(c["flow_gt"]), None)
        check_rows(rows, [R.flow(c["flow_est"][b], c["flow_gt"][b]) for b in range(B)], m.FLOW_RAW, m.FLOW_METRICS, summed=("sum_epe", "epe"))
        rows = m.mask_metrics(dev(c["mask_logit"]), dev(c["mask_gt"]), None)
        check_rows(rows, [R.mask(c["mask_logit"][b], c["mask_gt"][b]) for b in range(B)], m.MASK_RAW, m.MASK_METRICS)


def test_dense_unaligned_views_take_the_scalar_path():
    """arrays of one clip at different offsets inside a 16-byte line: same numbers as the aligned copy"""
    B, n = 1, 1000
    c = dense_case(B, n)
    m = M()

    def off(a, k):  # a contiguous view that starts k floats into a fresh buffer
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
        buf[k:k + a.size] = dev(a).reshape(-1)
        return buf[k:k + a.size].reshape(a.shape)

    want = m.depth_metrics(dev(c["depth_est"]), dev(c["depth_gt"]), dev(c["depth_valid"]), "none")
    got = m.depth_metrics(off(c["depth_est"], 1), off(c["depth_gt"], 2), off(c["depth_valid"], 0), "none")
    assert torch.equal(got[:, [0, 3, 4, 5, 8, 9, 10]], want[:, [0, 3, 4, 5, 8, 9, 10]])
    assert torch.allclose(got[:, [1, 2, 6, 7]], want[:, [1, 2, 6, 7]], rtol=SUM_RTOL, atol=0)
    got = m.depth_metrics(off(c["depth_est"], 3), off(c["depth_gt"], 3), off(c["depth_valid"], 3), "none")  # head of one element
    assert torch.equal(got[:, [0, 3, 4, 5]], want[:, [0, 3, 4, 5]])


def test_empty_clips_and_median_ranks():
    B, n = SMALL
    c = dense_case(B, n)
    m = M()
    est, gt = c["depth_est"], c["depth_gt"]
    ok = [np.flatnonzero(R.depth_valid(est[b], gt[b], None, 1e-3, 80.0)) for b in range(B)]
    valid = np.zeros((B, n), F)
    valid[0, ok[0][:1]] = 1  # one valid element: rank 0
    valid[1, ok[1][:4]] = 1  # an even count: the LOWER median, rank 1
    rows = m.depth_metrics(dev(est), dev(gt), dev(valid), "median")
    want = [R.depth(est[b], gt[b], valid[b], "median") for b in range(B)]
    assert [w["count"] for w in want] == [1, 4]
    check_rows(rows, want, m.DEPTH_RAW, m.DEPTH_METRICS, summed=("sum_abs_rel", "sum_sq", "abs_rel", "rmse"))
    assert [float(x) for x in rows[:, 11].cpu()] == [w["align_scale"] for w in want]
    # least squares of one element: no alignment, nothing scored
    row = m.depth_metrics(dev(est), dev(gt), dev(valid), "lstsq").cpu().numpy()
    assert math.isnan(row[0, 11]) and row[0, 0] == 0 and math.isnan(row[0, 6]) and not math.isnan(row[1, 6])
    # a clip with no valid element is NaN per clip and left out of the batch mean
    valid[:] = c["depth_valid"]
    valid[1] = 0
    mod = m.L4PMetrics()
    batch = {"depth_b1thw": dev(gt).reshape(B, 1, 3, 5, 7), "depth_valid_b1thw": dev(valid).reshape(B, 1, 3, 5, 7)}
    out = {"depth_est_b1thw": dev(est).reshape(B, 1, 3, 5, 7)}
    met, ex = mod(batch, out)
    per = ex["depth_abs_rel_per_clip"].cpu().numpy()
    w0 = R.depth(est[0], gt[0], valid[0], "median")
    assert close(float(per[0]), w0["abs_rel"]) and math.isnan(per[1]) and math.isnan(float(ex["depth_align_scale"][1]))
    assert met["depth_abs_rel"].dtype == torch.float32 and met["depth_abs_rel"].dim() == 0
    assert float(met["depth_abs_rel"]) == float(F(per[0]))
    assert float(ex["depth_count"][1]) == 0 and float(met["depth_delta1"]) == float(F(w0["delta1"]))
    # a batch of only such clips: NaN scalars
    batch["depth_valid_b1thw"] = torch.zeros_like(batch["depth_valid_b1thw"])
    met, ex = mod(batch, out)
    assert all(math.isnan(float(met[k])) for k in ("depth_abs_rel", "depth_rmse", "depth_delta1"))
    # flow and mask with nothing valid
    z = torch.zeros(B, 2, n, device="cuda")
    assert torch.isnan(m.flow_metrics(dev(c["flow_est"]), dev(c["flow_gt"]), z)[:, 5:9]).all()
    assert torch.isnan(m.mask_metrics(dev(c["mask_logit"]), dev(c["mask_gt"]), z[:, 0])[:, 4:9]).all()


@pytest.mark.parametrize("B,N,T,hw", [(2, 3, 5, (224, 224)), (1, 70, 24, (180, 320))], ids=["B2N3T5", "B1N70T24_HneW"])
def test_tracks_match_restatement(B, N, T, hw):
    c = R.make_track_case(B, N, T, seed=7 + N, hw=hw)
    m = M()
    rows = m.track_metrics(dev(c["traj_est"]), dev(c["traj_gt"]), dev(c["vis_logit"]), dev(c["vis_gt"]), dev(c["valid"]),
                           dev(c["queries"]), hw)
    want = [R.tracks(c["traj_est"][b], c["traj_gt"][b], c["vis_logit"][b], c["vis_gt"][b], c["valid"][b], c["queries"][b], hw)
            for b in range(B)]
    check_rows(rows, want, m.TRACK_RAW, m.TRACK_METRICS)
    for w in want:  # the planted distances reach both sides of every threshold
        assert 0 < w["count_within_1"] < w["count_within_2"] < w["count_within_4"] < w["count_within_8"] < w["count_within_16"] \
            < w["count_gt_visible"] or N == 3
    # a track queried in the last frame (everything before it cleared) scores no frame
    last = [i for i in range(N) if int(c["queries"][0, i, 0]) == T - 1]
    assert last
    only = np.zeros_like(c["valid"])
    only[:, last] = c["valid"][:, last]
    rows = m.track_metrics(dev(c["traj_est"]), dev(c["traj_gt"]), dev(c["vis_logit"]), dev(c["vis_gt"]), dev(only), dev(c["queries"]), hw)
    assert float(rows[0, 0]) == 0 and torch.isnan(rows[0, 18:31]).all()
    # no valid array: every frame but the query frame
    rows = m.track_metrics(dev(c["traj_est"]), dev(c["traj_gt"]), dev(c["vis_logit"]), dev(c["vis_gt"]), None, dev(c["queries"]), hw)
    want = [R.tracks(c["traj_est"][b], c["traj_gt"][b], c["vis_logit"][b], c["vis_gt"][b], None, c["queries"][b], hw) for b in range(B)]
    assert want[0]["count"] == N * (T - 1)
    check_rows(rows, want, m.TRACK_RAW, m.TRACK_METRICS)


@pytest.mark.parametrize("T", [3, 24])
def test_cameras_match_restatement(T):
    cases = [R.make_camera_case(T, seed=11), R.make_camera_case(T, seed=12, reflect=True)]  # clip 1: the reflection branch
    pose = np.stack([c[0] for c in cases])
    extr = np.stack([c[1] for c in cases])
    m = M()
    rows = m.camera_metrics(dev(pose), dev(extr)).cpu().numpy()
    for b in range(2):
        want = R.cameras(pose[b], extr[b])
        for name, col in {**m.CAM_METRICS, **m.CAM_RAW}.items():
            got, w = float(rows[b, col]), float(want[name])
            print(f"T={T} clip {b} {name}: kernel {got!r} restatement {w!r}")
            assert abs(got - w) <= 1e-9 * abs(w) + 1e-12, (b, name, got, w)
        assert want["ate"] > 0 and want["rpe_rot"] > 0
    if T > 3:
        P = pose[1].astype(np.float64).reshape(4, 4, T).transpose(2, 0, 1)
        G = np.linalg.inv(extr[1].astype(np.float64).transpose(2, 0, 1))
        assert np.linalg.det(R.umeyama(P[:, :3, 3], G[:, :3, 3])[3]) < 0


def test_refusals():
    from l4p_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")  # stands in for every pointer: a refused call launches nothing
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    big = 1 << 31

    def refused(name, rc):
        msg = lib.l4p_last_error().decode()
        assert rc == -1 and name in msg, (name, rc, msg)

    ws = int(lib.l4p_metric_ws_bytes(1, 105, 1))
    assert ws > 0 and lib.l4p_metric_ws_bytes(0, 105, 1) == 0 and lib.l4p_metric_ws_bytes(1, 105, 3) == 0
    assert lib.l4p_metric_ws_bytes(1, big, 0) == 0
    for args in [(0, 105, 1), (1, 0, 1), (1, big, 1), (2, 1 << 30, 0)]:
        refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, args[0], args[1], args[2], 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 3, 1e-3, 80.0, p, 1 << 19, p))  # unknown mode
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, -1, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 1, 0.0, 80.0, p, 1 << 19, p))  # dmin
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 1, 2.0, 1.0, p, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, None, p, p, 1, 105, 1, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, None, p, 1, 105, 1, 1e-3, 80.0, p, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 1, 1e-3, 80.0, None, 1 << 19, p))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 1, 1e-3, 80.0, p, 1 << 19, None))
    refused("l4p_metric_depth", lib.l4p_metric_depth(st, p, p, p, 1, 105, 1, 1e-3, 80.0, p, ws - 1, p))  # workspace too small
    for name in ("l4p_metric_flow", "l4p_metric_mask"):
        fn = getattr(lib, name)
        for B, n in [(0, 105), (1, 0), (1, big), (1, 1 << 30)]:
            if name == "l4p_metric_mask" and (B, n) == (1, 1 << 30):
                continue  # (a legal mask size; the flow entry indexes 2 B n elements)
            refused(name, fn(st, p, p, p, B, n, p, 1 << 19, p))
        refused(name, fn(st, None, p, p, 1, 105, p, 1 << 19, p))
        refused(name, fn(st, p, None, p, 1, 105, p, 1 << 19, p))
        refused(name, fn(st, p, p, p, 1, 105, None, 1 << 19, p))
        refused(name, fn(st, p, p, p, 1, 105, p, 1 << 19, None))
        refused(name, fn(st, p, p, p, 1, 105, p, 16, p))
    trk = lib.l4p_metric_tracks
    for B, N, T, H, W in [(0, 3, 5, 8, 8), (1, 0, 5, 8, 8), (1, 3, 0, 8, 8), (1, 3, 5, 0, 8), (1, 3, 5, 8, 0), (4, 1 << 15, 1 << 14, 8, 8)]:
        refused("l4p_metric_tracks", trk(st, p, p, p, p, p, p, B, N, T, H, W, p, p))
    for k in (0, 1, 2, 3, 5, 6, 7):  # every pointer but valid
        ptrs = [p] * 8
        ptrs[k] = None
        refused("l4p_metric_tracks", trk(st, *ptrs[:6], 1, 3, 5, 8, 8, *ptrs[6:]))
    cam = lib.l4p_metric_cameras
    for B, T in [(1, 2), (0, 5), (1, 0), (1, 1 << 28)]:
        refused("l4p_metric_cameras", cam(st, p, p, B, T, p))
    refused("l4p_metric_cameras", cam(st, None, p, 1, 5, p))
    refused("l4p_metric_cameras", cam(st, p, None, 1, 5, p))
    refused("l4p_metric_cameras", cam(st, p, p, 1, 5, None))
    sel = lib.l4p_select_median_dev
    for B, n in [(0, 5), (1, 0), (1, big)]:
        refused("l4p_select_median_dev", sel(st, p, n, B, p, 1, p, p, 1))
    refused("l4p_select_median_dev", sel(st, None, 5, 1, p, 1, p, p, 1))
    refused("l4p_select_median_dev", sel(st, p, 5, 1, None, 1, p, p, 1))
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0  # nothing was launched
    with pytest.raises(_lib.L4PHipError, match="l4p_metric_cameras"):
        M().camera_metrics(torch.zeros(1, 16, 2, device="cuda"), torch.zeros(1, 4, 4, 2, device="cuda"))
    with pytest.raises(AssertionError):
        M().depth_metrics(torch.zeros(1, 8), torch.zeros(1, 8))  # host tensors never reach a kernel


def five_task_inputs(B=2, T=5, H=6, W=9, N=4, seed=3):
    """a small batch / out pair with all five tasks on the device"""
    n = T * H * W
    c = R.make_dense_case(B, n, seed)
    tr = R.make_track_case(B, N, T, seed, hw=(H, W))
    cams = [R.make_camera_case(T, seed + b) for b in range(B)]
    batch = {
        "rgb_b3thw": torch.zeros(B, 3, T, H, W, device="cuda"),
        "depth_b1thw": dev(c["depth_gt"]).reshape(B, 1, T, H, W), "depth_valid_b1thw": dev(c["depth_valid"]).reshape(B, 1, T, H, W) > 0.5,
        "flow_2d_backward_b2thw": dev(c["flow_gt"]).reshape(B, 2, T, H, W),
        "flow_2d_backward_valid_b2thw": dev(c["flow_valid"]).reshape(B, 2, T, H, W),
        "dyn_mask_b1thw": dev(c["mask_gt"]).reshape(B, 1, T, H, W), "dyn_mask_valid_b1thw": dev(c["mask_valid"]).reshape(B, 1, T, H, W),
        "track_2d_traj_bn2t": dev(tr["traj_gt"]), "track_2d_vis_bn1t": dev(tr["vis_gt"]), "track_2d_valid_bn1t": dev(tr["valid"]),
        "track_2d_pointquerries_bn3": dev(tr["queries"]),
        "extrinsics_b44t": dev(np.stack([x[1] for x in cams])),
    }
    out = {
        "depth_est_b1thw": dev(c["depth_est"]).reshape(B, 1, T, H, W).to(torch.float16).to(torch.float32).to(torch.float64),
        "flow_2d_backward_est_b2thw": dev(c["flow_est"]).reshape(B, 2, T, H, W),
        "dyn_mask_est_b1thw": dev(c["mask_logit"]).reshape(B, 1, T, H, W),
        "track_2d_traj_est_bn2t": dev(tr["traj_est"]), "track_2d_vis_est_bn1t": dev(tr["vis_logit"]),
        "traj3d_est_b16t": dev(np.stack([x[0] for x in cams])),
    }
    return batch, out, c, tr, cams


def test_module_keys_reproducibility_and_no_host_sync():
    m = M()
    batch, out, c, tr, cams = five_task_inputs()
    mod = m.L4PMetrics()
    met, ex = mod(batch, out)
    want_keys = {f"depth_{k}" for k in m.DEPTH_METRICS} | {f"flow_{k}" for k in m.FLOW_METRICS} | \
        {f"dyn_mask_{k}" for k in m.MASK_METRICS} | {f"track_2d_{k}" for k in m.TRACK_METRICS} | {f"camray_{k}" for k in m.CAM_METRICS}
    assert set(met) == want_keys
    for k, v in met.items():
        assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda and math.isfinite(float(v)), k
    assert {k + "_per_clip" for k in want_keys} <= set(ex) and {"depth_align_scale", "depth_align_shift", "depth_count"} <= set(ex)
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (2,) for v in ex.values())
    # the module against the restatement, through its dtype handling (a float64 estimate, bool masks)
    est = out["depth_est_b1thw"].to(torch.float32).cpu().numpy().reshape(2, -1)
    w = [R.depth(est[b], c["depth_gt"][b], c["depth_valid"][b], "median") for b in range(2)]
    assert [float(x) for x in ex["depth_delta1_per_clip"].cpu()] == [x["delta1"] for x in w]
    assert float(met["depth_delta1"]) == float(F((w[0]["delta1"] + w[1]["delta1"]) / 2))
    wt = [R.tracks(tr["traj_est"][b], tr["traj_gt"][b], tr["vis_logit"][b], tr["vis_gt"][b], tr["valid"][b], tr["queries"][b], (6, 9))
          for b in range(2)]
    assert [float(x) for x in ex["track_2d_average_jaccard_per_clip"].cpu()] == [x["average_jaccard"] for x in wt]
    wc = R.cameras(cams[1][0], cams[1][1])
    assert close(float(ex["camray_ate_per_clip"][1]), wc["ate"])
    # tasks=: only these; a task with a missing side is skipped silently
    met2, _ = m.L4PMetrics(tasks=["flow", "camray"])(batch, out)
    assert {k.split("_")[0] for k in met2} == {"flow", "camray"}
    met3, _ = mod({k: v for k, v in batch.items() if k != "depth_b1thw"}, {k: v for k, v in out.items() if k != "traj3d_est_b16t"})
    assert not any(k.startswith(("depth_", "camray_")) for k in met3) and "flow_epe" in met3
    # two calls on the same inputs: the same bits
    _, ex2 = mod(batch, out)
    for k in ex:
        assert torch.equal(ex[k].view(torch.int64), ex2[k].view(torch.int64)), k
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
            met4, ex4 = mod(batch, out)
            met5, _ = m.L4PMetrics(depth_align="lstsq")(batch, out)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not implemented:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a synchronising call in this torch build on ROCm")
    assert torch.equal(ex4["flow_epe_per_clip"].view(torch.int64), ex["flow_epe_per_clip"].view(torch.int64))
    assert math.isfinite(float(met5["depth_abs_rel"]))


def test_end_to_end_mini_test_step():
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
    # synthetic ground truth (host tensors: step() brings the batch to the model's device)
    batch["depth_b1thw"] = torch.from_numpy(rng.uniform(0.5, 10.0, (1, 1, T, 224, 224)).astype(F))
    batch["depth_valid_b1thw"] = torch.from_numpy(rng.uniform(size=(1, 1, T, 224, 224)) > 0.3)
    batch["flow_2d_backward_b2thw"] = torch.from_numpy(rng.uniform(-2, 2, (1, 2, T, 224, 224)).astype(F))
    batch["dyn_mask_b1thw"] = torch.from_numpy((rng.uniform(size=(1, 1, T, 224, 224)) > 0.5).astype(F))
    q = batch["track_2d_pointquerries_bn3"]
    traj = q[:, :, 1:, None].repeat(1, 1, 1, T) + torch.from_numpy(rng.uniform(-3, 3, (1, N, 2, T)).astype(F))
    batch["track_2d_traj_bn2t"] = traj
    batch["track_2d_vis_bn1t"] = torch.from_numpy(rng.uniform(size=(1, N, 1, T)) > 0.3)
    batch["track_2d_valid_bn1t"] = torch.arange(T)[None, None, None, :] >= torch.floor(q[:, :, 0])[:, :, None, None]
    _, extr = R.make_camera_case(T, seed=9)
    batch["extrinsics_b44t"] = torch.from_numpy(extr)[None]
    model.metrics_module = m.L4PMetrics()
    with torch.no_grad():
        res = model.test_step(batch, 0)
    assert set(res) == {"loss", "out"} and res["loss"] == 0 and "depth_est_b1thw" in res["out"]
    log = model.last_log
    for key in ("depth_abs_rel", "depth_rmse", "depth_delta1", "flow_epe", "flow_1px", "dyn_mask_iou", "dyn_mask_f1",
                "track_2d_average_jaccard", "track_2d_occlusion_accuracy", "track_2d_average_pts_within_thresh", "camray_ate",
                "camray_rpe_trans", "camray_rpe_rot"):
        v = log[f"scalars/val/{key}"]
        print(key, float(v))
        assert v.dtype == torch.float32 and v.dim() == 0 and math.isfinite(float(v)), key
    assert log["scalars/val/loss"] == 0
    with torch.no_grad():
        out = model.predict_step(batch, 0)  # unchanged: the outputs, nothing scored
    assert isinstance(out, dict) and "depth_est_b1thw" in out
