"""GPU: the two callers of csrc/umeyama_moments.hpp and the similarity's application, through the C ABI, at the inputs where a closed
form goes wrong (its arithmetic alone is covered on the host by tests/test_umeyama_moments_cpu.py):

  l4p_metric_cameras     == tests/metrics_restate.py:cameras (float64, np.linalg.svd) within 1e-9 on degenerate trajectories - gt
                            centres exactly along x, y, z (identity gt rotations: a dolly shot; the covariance has two rows of exact
                            zeros) and along an oblique line, collinear estimates, planar gt, static gt (s = 0), static estimate
                            (s = 1), a mirrored clip - at T = 3 and 24; the curved path at T = 255, 256, 257, 600 (the 256-stride frame
                            loops and the t + 1 < T neighbour load wrap); three different clips in one call into a sentinel-filled
                            buffer.  The lines are exact in float32, so the rank is 1 exactly and the ATE does not depend on the free
                            rotation about the line: the 1e-9 bound applies as it stands.
  l4p_similarity_ransac  == the float64 closed form on PLANTED inliers (noise <= thr / 10, outliers >= 10 thr) within 1e-5 max|T|, the
                            inlier count exactly, at n = 3 .. 1000, trials = 1 and 100, min_samples = 3 and 32; a planar and a mirrored
                            cloud; the branch that keeps the trial model; the refusals.
  l4p_similarity_apply   == oracle/joint_oracle.py:similarity_apply in float64 within 1e-6 of the maximum at T = 1, 63, 64, 65, 130.
"""
import functools

import numpy as np
import pytest
import torch

from l4p_amd import _lib
from oracle import joint_oracle as jo
from tests import metrics_restate as MR

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = -777.0
SKEW = [0.3, -1.0, 0.45]
CAM_COLS = {"ate": 0, "rpe_trans": 1, "rpe_rot": 2, "align_scale": 3, "sum_sq_ate": 4, "sum_sq_rpe_trans": 5, "sum_sq_rpe_rot": 6, "frames": 7}


def _st():
    return torch.cuda.current_stream().cuda_stream


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- cameras
def _pack(We, Wg):
    """world_T_cam [T, 4, 4] of the estimate and of the gt -> (pose_est [16, T] f32, extr_gt [4, 4, T] f32)"""
    T = len(We)
    return We.transpose(1, 2, 0).reshape(16, T).astype(F), np.linalg.inv(Wg).transpose(1, 2, 0).astype(F)


def _line_centres(rng, T, direction):
    """T centres exactly on a line, exact in float32: integer steps of direction / 16 from a dyadic offset"""
    m = rng.permutation(np.arange(-2 * T, 2 * T))[:T].astype(np.float64)
    return m[:, None] * np.asarray(direction, np.float64) / 16.0 + np.array([0.25, -0.5, 1.5])


@functools.lru_cache(maxsize=None)
def camera_case(kind, T):
    """One clip and its restatement.  The estimate is a similarity of a 3-D path plus noise, with slightly turned cameras."""
    if kind in ("curved", "mirrored"):
        pose, extr = MR.make_camera_case(T, seed=11 + T % 7, reflect=kind == "mirrored")
        return pose, extr, MR.cameras(pose, extr)
    rng = np.random.default_rng(500 + T + sum(map(ord, kind)))
    path = MR.make_poses(T, seed=21)
    Wg, We = np.tile(np.eye(4), (T, 1, 1)), path.copy()
    for i in range(T):
        We[i, :3, :3] = path[i, :3, :3] @ MR.rot(rng.standard_normal(3), 0.02 * rng.standard_normal())
    if kind.startswith("gt_"):  # identity gt rotations: cam_T_world = [I | -c] is exact in float32
        direction = {"gt_x": [1, 0, 0], "gt_y": [0, 1, 0], "gt_z": [0, 0, 1], "gt_oblique": [1, 2, 3]}.get(kind)
        if direction is not None:
            Wg[:, :3, 3] = _line_centres(rng, T, direction)
        else:  # gt_planar: z = 1.5 exactly
            Wg[:, :3, 3] = np.round(path[:, :3, 3] * 64) / 64
            Wg[:, 2, 3] = 1.5
        extent = float(np.ptp(Wg[:, :3, 3], axis=0).max())
        noisy = Wg[:, :3, 3] + 0.05 * extent * rng.standard_normal((T, 3))
        We[:, :3, 3] = 1.7 * noisy @ MR.rot(SKEW, 0.9).T + np.array([0.5, -1.0, 2.0])
    elif kind == "est_collinear":
        Wg = path
        We[:, :3, 3] = _line_centres(rng, T, [1, 2, 3])
    elif kind == "static_gt":
        Wg[:, :3, 3] = np.array([1.5, -2.25, 0.75])
    elif kind == "static_est":
        Wg = path
        We[:, :3, 3] = np.array([1.5, -2.25, 0.75])
    else:
        raise ValueError(kind)
    pose, extr = _pack(We, Wg)
    return pose, extr, MR.cameras(pose, extr)


def run_cameras(clips, rows_before=1, rows_after=1):
    """l4p_metric_cameras on a list of (pose, extr) into the middle of a sentinel-filled buffer; returns the clips' rows"""
    B, T = len(clips), clips[0][0].shape[1]
    pose, extr = to_gpu(np.stack([c[0] for c in clips])), to_gpu(np.stack([c[1] for c in clips]))
    out = torch.full((rows_before + B + rows_after, 8), SENTINEL, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    _lib.check(lib.l4p_metric_cameras(_st(), pose.data_ptr(), extr.data_ptr(), B, T, out[rows_before:].data_ptr()), "l4p_metric_cameras")
    host = out.cpu().numpy()
    assert (host[:rows_before] == SENTINEL).all() and (host[rows_before + B:] == SENTINEL).all(), "a write outside the clips' rows"
    return host[rows_before:rows_before + B]


def check_camera_row(row, want, tag):
    assert np.isfinite(row).all(), (tag, row)
    for name, col in CAM_COLS.items():
        got, w = float(row[col]), float(want[name])
        print(f"{tag} {name}: kernel {got!r} restatement {w!r}")
        assert abs(got - w) <= 1e-9 * abs(w) + 1e-12, (tag, name, got, w)


DEGENERATE = ["gt_x", "gt_y", "gt_z", "gt_oblique", "est_collinear", "gt_planar", "static_gt", "static_est", "mirrored"]


@pytest.mark.parametrize("T", [3, 24])
@pytest.mark.parametrize("kind", DEGENERATE)
def test_cameras_on_degenerate_trajectories(dev, kind, T):
    pose, extr, want = camera_case(kind, T)
    row = run_cameras([(pose, extr)])[0]
    check_camera_row(row, want, f"{kind} T={T}")
    P = pose.astype(np.float64).reshape(4, 4, T).transpose(2, 0, 1)[:, :3, 3]
    G = np.linalg.inv(extr.astype(np.float64).transpose(2, 0, 1))[:, :3, 3]
    cov = MR.umeyama(P, G)[3]
    sv = np.linalg.svd(cov, compute_uv=False)
    if kind in ("gt_x", "gt_y", "gt_z"):  # the case is what it says: two rows of exact zeros, and a residual worth reporting
        assert not np.delete(cov, "xyz".index(kind[-1]), axis=0).any() and (want["ate"] > 0.1 or T == 3)
    if kind in ("gt_oblique", "est_collinear"):
        assert sv[1] <= 1e-14 * sv[0] and want["ate"] > 0.01
    if kind == "gt_planar":
        assert not cov[2].any() and sv[1] > 1e-3 * sv[0]
    if kind == "static_gt":
        assert not cov.any() and want["align_scale"] == 0.0 and row[3] == 0.0 and row[0] == 0.0
    if kind == "static_est":
        assert not cov.any() and want["align_scale"] == 1.0 and row[3] == 1.0 and want["ate"] > 0.1
    if kind == "mirrored" and T > 3:
        assert np.linalg.det(cov) < 0


@pytest.mark.parametrize("T", [255, 256, 257, 600])
def test_cameras_past_one_stride_of_frames(dev, T):
    pose, extr, want = camera_case("curved", T)
    check_camera_row(run_cameras([(pose, extr)])[0], want, f"curved T={T}")
    assert want["ate"] > 0 and want["rpe_rot"] > 0 and want["frames"] == T


def test_cameras_three_different_clips_in_one_call(dev):
    kinds = ["gt_x", "curved", "static_est"]
    rows = run_cameras([camera_case(k, 24)[:2] for k in kinds], rows_before=2, rows_after=2)
    for k, row in zip(kinds, rows):
        check_camera_row(row, camera_case(k, 24)[2], f"B=3 {k}")


# ------------------------------------------------------------------------------------------------- RANSAC
THR_REL, Q98 = 0.01, 1.0  # thr = 0.01: the cloud's extent is 2
T_PLANT = np.array([0.4, -1.1, 0.8])


@functools.lru_cache(maxsize=None)
def ransac_case(n, n_out, s, angle, seed, planar=False):
    """float32 src / dst with dst = s R src + t, inlier noise of norm <= thr / 10, and n_out planted outliers moved by 10 .. 100 thr"""
    rng = np.random.default_rng(seed)
    thr = THR_REL * Q98
    R = MR.rot(SKEW, angle)
    src = (rng.uniform(-1, 1, (n, 3)) + np.array([1.0, -0.5, 2.0])).astype(F)
    if planar:
        src[:, 2] = 2.0  # the camera looks at a wall
    noise = rng.standard_normal((n, 3))
    noise *= (0.09 * thr * rng.uniform(0, 1, (n, 1))) / np.linalg.norm(noise, axis=1, keepdims=True)
    dst = s * src.astype(np.float64) @ R.T + T_PLANT + noise
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:n_out]] = True
    push = rng.standard_normal((n, 3))
    push *= (thr * rng.uniform(10, 100, (n, 1))) / np.linalg.norm(push, axis=1, keepdims=True)
    dst = np.where(out[:, None], dst + push, dst).astype(F)
    return src, dst, ~out


def sample_indices(n, trial, min_samples, seed):
    j = np.arange(min_samples, dtype=np.uint64)
    return (jo.hash_u32((np.uint64(seed) + np.uint64(7919 * trial) + np.uint64(104729) * j) & np.uint64(0xFFFFFFFF)) % np.uint64(n)).astype(np.int64)


def closed_form(src, dst):
    """the float64 closed form as the 18 values of the entry: row-major [s R | t; 0 0 0 1], s, (count left out)"""
    s, R, t, _ = MR.umeyama(src.astype(np.float64), dst.astype(np.float64))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return np.concatenate([M.reshape(-1), [s]])


def run_ransac(src, dst, q98, trials, min_samples, seed, expect_rc=0):
    n = len(src)
    lib = _lib.load()
    ws = torch.zeros(15 * max(trials, 1), dtype=torch.float32, device="cuda")
    out = torch.full((18 + 14,), SENTINEL, dtype=torch.float32, device="cuda")
    q = torch.tensor([q98], dtype=torch.float32, device="cuda")
    s_, d_ = to_gpu(src), to_gpu(dst)
    rc = lib.l4p_similarity_ransac(_st(), s_.data_ptr(), d_.data_ptr(), n, q.data_ptr(), THR_REL, trials, min_samples, seed, ws.data_ptr(),
                                   out.data_ptr())
    assert rc == expect_rc, (rc, lib.l4p_last_error().decode())
    host = out.cpu().double().numpy()
    assert (host[18:] == SENTINEL).all(), "a write past out[17]"
    return host[:18]


def check_against_planted(n, n_out, s, angle, trials, min_samples, seed, planar=False):
    src, dst, inl = ransac_case(n, n_out, s, angle, 900 + n + trials, planar)
    thr = F(THR_REL) * F(Q98)
    # on the CPU: some trial draws three distinct inliers and nothing else, and the restated schedule (each trial's float64 closed form,
    # float residuals) separates the planted sets with room to spare in every trial that reaches the best count, so that rounding in
    # the kernel's residuals cannot move a point across the threshold
    samples = [sample_indices(n, t, min_samples, seed) for t in range(trials)]
    assert any(inl[idx].all() and len(set(idx)) >= 3 for idx in samples), "no trial draws three distinct inliers: choose another seed"
    res = [jo._residuals(closed_form(src[idx], dst[idx])[:16].reshape(4, 4), src, dst) for idx in samples]
    best = max(int((r < thr).sum()) for r in res)
    assert best == inl.sum(), "no trial of the restated schedule finds the planted inliers: choose another seed"
    for r in res:
        if int((r < thr).sum()) == best:
            assert np.array_equal(r < thr, inl) and r[inl].max() < 0.5 * thr and (inl.all() or r[~inl].min() > 2 * thr), "choose another seed"
    got = run_ransac(src, dst, Q98, trials, min_samples, seed)
    want = closed_form(src[inl], dst[inl])
    print(f"n={n} trials={trials} min_samples={min_samples}: count {got[17]} planted {inl.sum()} s {got[16]!r} closed form {want[16]!r} "
          f"max|dT| {np.abs(got[:16] - want[:16]).max():.3e}")
    assert got[17] == inl.sum()
    assert np.abs(got[:17] - want).max() <= 1e-5 * np.abs(want[:16]).max(), (got, want)
    assert abs(got[16] - s) <= 1e-2 * s  # and both recover the planted scale


# (n, planted outliers, s, angle, trials, min_samples, seed): the seeds were chosen on the CPU, by the two assertions above
PLANTED = [
    (3, 0, 0.5, 0.3, 100, 3, 1), (3, 0, 1.7, np.pi, 1, 3, 16), (4, 1, 1.7, 2.9, 100, 3, 1), (4, 1, 0.5, np.pi, 1, 3, 12),
    (255, 51, 0.5, np.pi, 100, 3, 1), (256, 51, 1.7, 0.3, 100, 3, 1), (257, 51, 0.5, 2.9, 100, 3, 5), (257, 51, 1.7, 0.3, 1, 3, 1),
    (1000, 200, 1.7, np.pi, 100, 3, 4), (1000, 200, 0.5, 2.9, 1, 3, 2), (257, 3, 1.7, 2.9, 100, 32, 1),
]


@pytest.mark.parametrize("n,n_out,s,angle,trials,min_samples,seed", PLANTED,
                         ids=[f"n{c[0]}_s{c[2]}_a{c[3]:.1f}_trials{c[4]}_min{c[5]}" for c in PLANTED])
def test_ransac_recovers_planted_similarity(dev, n, n_out, s, angle, trials, min_samples, seed):
    check_against_planted(n, n_out, s, angle, trials, min_samples, seed)


def test_ransac_planar_cloud(dev):
    check_against_planted(256, 51, 1.7, 0.3, 100, 3, 15, planar=True)


def test_ransac_mirrored_cloud_returns_a_proper_rotation(dev):
    """every point an inlier (a threshold of many extents), so the re-estimate runs the reflection branch on the whole cloud"""
    src, dst, _ = ransac_case(257, 0, 1.7, 2.9, 77)
    src = src * np.array([1.0, 1.0, -1.0], F)
    got = run_ransac(src, dst, 1e4, 100, 3, jo.ENGINE_SEED)
    want = closed_form(src, dst)
    assert np.linalg.det(MR.umeyama(src, dst)[3]) < 0 and got[17] == 257
    assert np.abs(got[:17] - want).max() <= 1e-5 * np.abs(want[:16]).max(), (got, want)
    R = got[:16].reshape(4, 4)[:3, :3] / got[16]
    assert abs(np.linalg.det(R) - 1.0) <= 1e-5 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-5


@pytest.mark.parametrize("min_samples,seed", [(3, 1), (10, 1)])
def test_ransac_without_inliers_keeps_the_first_trial_model(dev, min_samples, seed):
    """q98 = 0: no residual is below the threshold, every trial scores (0, 0), trial 0 wins and its model is returned as it is"""
    src, dst, _ = ransac_case(257, 51, 1.7, 0.3, 78)
    idx = sample_indices(257, 0, min_samples, seed)
    assert len(set(idx)) == min_samples, "trial 0 repeats a point: choose another seed"
    got = run_ransac(src, dst, 0.0, 100, min_samples, seed)
    want = closed_form(src[idx], dst[idx])
    assert got[17] == 0
    assert np.abs(got[:17] - want).max() <= 1e-5 * np.abs(want[:16]).max(), (got, want)
    assert list(got[12:16]) == [0.0, 0.0, 0.0, 1.0]


def test_ransac_repeated_sample_points_still_give_a_rotation(dev):
    """n = 3 draws with replacement: trial 0 repeats a point (a collinear sample, rank 1), nothing is an inlier at q98 = 0, and the
    model that is kept is a similarity with a proper rotation all the same"""
    src, dst, _ = ransac_case(3, 0, 1.7, 0.3, 79)
    seed = next(sd for sd in range(1, 100) if len(set(sample_indices(3, 0, 3, sd))) == 2)
    got = run_ransac(src, dst, 0.0, 1, 3, seed)
    assert np.isfinite(got).all() and got[17] == 0 and got[16] > 0
    R = got[:16].reshape(4, 4)[:3, :3] / got[16]
    assert abs(np.linalg.det(R) - 1.0) <= 1e-5 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-5
    idx = sample_indices(3, 0, 3, seed)
    want = closed_form(src[idx], dst[idx])
    assert abs(got[16] - want[16]) <= 1e-5 * want[16]
    fit = src[idx].astype(np.float64) @ got[:16].reshape(4, 4)[:3, :3].T + got[:16].reshape(4, 4)[:3, 3] - dst[idx]
    ref = src[idx].astype(np.float64) @ want[:16].reshape(4, 4)[:3, :3].T + want[:16].reshape(4, 4)[:3, 3] - dst[idx]
    assert np.abs(fit).max() <= np.abs(ref).max() + 1e-5 * np.abs(want[:16]).max()


def test_ransac_refusals_leave_out_untouched(dev):
    src, dst, _ = ransac_case(257, 51, 1.7, 0.3, 78)
    for n, trials, min_samples in [(2, 100, 3), (9, 100, 10), (257, 100, 2), (257, 100, 33), (257, 0, 3), (257, -1, 3)]:
        got = run_ransac(src[:n], dst[:n], Q98, trials, min_samples, 1, expect_rc=_lib.L4P_E_INVALID)
        assert (got == SENTINEL).all(), (n, trials, min_samples, got)
        assert "similarity_ransac" in _lib.load().l4p_last_error().decode()


# ------------------------------------------------------------------------------------------------- apply
def _sim_record(s=1.7, angle=2.9):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * MR.rot(SKEW, angle), T_PLANT
    return np.concatenate([M.reshape(-1), [s, 123.0]]).astype(F)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_apply_against_the_oracle(dev, T):
    rng = np.random.default_rng(40 + T)
    sim = _sim_record()
    pose = rng.standard_normal((16, T)).astype(F)
    depth = (rng.uniform(0.5, 1.5, 3 * T + 5)).astype(F)
    pad = 70
    pbuf = torch.full((16 * T + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    pbuf[:16 * T] = torch.from_numpy(pose.reshape(-1)).cuda()
    dbuf = torch.full((depth.size + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    dbuf[:depth.size] = torch.from_numpy(depth).cuda()
    sd = torch.from_numpy(sim).cuda()
    lib = _lib.load()
    _lib.check(lib.l4p_similarity_apply(_st(), sd.data_ptr(), pbuf.data_ptr(), T, dbuf.data_ptr(), depth.size), "l4p_similarity_apply")
    rel = {"T": torch.from_numpy(sim[:16].astype(np.float64)).view(1, 4, 4), "s": torch.from_numpy(sim[16:17].astype(np.float64))}
    want = jo.similarity_apply(rel, {"camray": torch.from_numpy(pose.astype(np.float64))[None], "depth": torch.from_numpy(depth.astype(np.float64))})
    got_p, got_d = pbuf.cpu().double(), dbuf.cpu().double()
    assert (got_p[16 * T:] == SENTINEL).all() and (got_d[depth.size:] == SENTINEL).all(), "a write past the T frames / n depths"
    wp, wd = want["camray"][0].reshape(-1), want["depth"]
    assert (got_p[:16 * T] - wp).abs().max() <= 1e-6 * wp.abs().max(), float((got_p[:16 * T] - wp).abs().max() / wp.abs().max())
    assert (got_d[:depth.size] - wd).abs().max() <= 1e-6 * wd.abs().max()
    assert torch.equal(sd.cpu(), torch.from_numpy(sim))
    # depth = NULL or n = 0: the poses again, the depth left alone
    before = dbuf.clone()
    p2 = pbuf.clone()
    p2[:16 * T] = torch.from_numpy(pose.reshape(-1)).cuda()
    _lib.check(lib.l4p_similarity_apply(_st(), sd.data_ptr(), p2.data_ptr(), T, dbuf.data_ptr(), 0), "l4p_similarity_apply")
    assert torch.equal(dbuf, before) and torch.equal(p2, pbuf)
    p2[:16 * T] = torch.from_numpy(pose.reshape(-1)).cuda()
    _lib.check(lib.l4p_similarity_apply(_st(), sd.data_ptr(), p2.data_ptr(), T, None, depth.size), "l4p_similarity_apply")
    assert torch.equal(dbuf, before) and torch.equal(p2, pbuf)
