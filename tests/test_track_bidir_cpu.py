"""CPU: the definition of tracking in both time directions (tests/track_bidir_restate.py) - against the reference-pinned fixture
tests/golden/mini_T32_bidir.npz (tools/gen_golden_bidir.py) when driven by the oracle, and at the edges of its ownership rule."""
import os

import numpy as np
import pytest
import torch

from l4p_amd.weights import ModelCfg, seeded_state_dict
from tests import track_bidir_restate as rs
from tests.golden_utils import make_batch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ORACLE = {}


def oracle_composition():
    """-> (batch, merged outputs, the reversed pass's trace, the fixture): the restatement driven by oracle.l4p_oracle.OracleModel on
    the fixture's inputs.  Computed once per process (the GPU tests compare against the same run)."""
    if not _ORACLE:
        from oracle.l4p_oracle import OracleModel

        cfg = ModelCfg.mini()
        sd = seeded_state_dict(cfg)
        gold = np.load(os.path.join(GOLD, "mini_T32_bidir.npz"))
        batch = make_batch(32, 12, int(gold["seed"]))
        traces = {}

        def run(b):
            tr = []
            out = OracleModel(sd, cfg).forward(b, ["track_2d"], trace=tr)
            traces["fwd" if b is batch else "rev"] = tr
            return out

        with torch.no_grad():
            merged = rs.compose(run, batch)
        _ORACLE.update(batch=batch, merged=merged, rev_trace=traces["rev"], gold=gold)
    return _ORACLE["batch"], _ORACLE["merged"], _ORACLE["rev_trace"], _ORACLE["gold"]


def test_restatement_on_the_oracle_reproduces_the_reference_fixture():
    batch, merged, rev_trace, gold = oracle_composition()
    assert float(gold["min_margin"]) >= 1e-3 and float(gold["oracle_rel_err"]) <= 1e-4
    for key in rs.KEYS:
        ref = torch.from_numpy(gold[key])
        assert merged[key].shape == ref.shape == (1, 12, 2 if "traj" in key else 1, 32)
        err = float((merged[key] - ref).abs().max() / ref.abs().max())
        print(f"{key}: max |oracle composition - reference composition| / max |reference| = {err:.2e}")
        assert err <= 1e-4, (key, err)
    # the reversed pass's integer state, window by window
    assert len(rev_trace) == 3
    for w, tr in enumerate(rev_trace):
        assert np.array_equal(tr["labels"].numpy(), gold[f"rev_trace{w}_labels"]), w
        assert np.array_equal(tr["prompt_labels"].numpy(), gold[f"rev_trace{w}_prompt_labels"]), w
        assert np.array_equal(tr["queries"][:, 0].numpy(), gold[f"rev_trace{w}_queries"][:, 0]), w
        assert np.array_equal(tr["valid_t"].numpy(), gold[f"rev_trace{w}_valid_t"]), w
        if w < 2:
            assert np.array_equal(tr["best_vis_id"].numpy(), gold[f"rev_trace{w}_best_vis_id"]), w
    # the fixture is not the forward pass in disguise: frames before a query hold estimates, not the fill values
    q = batch["track_2d_pointquerries_bn3"][0, :, 0].numpy()
    own = rs.forward_owned(q, 32)
    assert (~own).any() and (gold["track_2d_vis_est_bn1t"][0, :, 0][~own] != -10.0).all()


@pytest.mark.parametrize("T", [1, 2, 16])
def test_ownership_rule_at_its_edges(T):
    tq = np.array(rs.edge_times(T), dtype=np.float32)
    own = rs.forward_owned(tq, T)
    assert own.shape == (len(tq), T) and own.dtype == np.bool_
    # the sign of a correctly rounded f32 difference is the sign of the exact one: the rule is "frame centre >= query time", exactly
    centre = np.arange(T, dtype=np.float64) + 0.5
    with np.errstate(invalid="ignore"):
        want = centre[None, :] >= tq.astype(np.float64)[:, None]
    assert np.array_equal(own, want)
    # ... spelled out where it matters: a query on frame 0 (or one f32 step before its centre) leaves nothing to the reversed pass,
    # one step after it hands frame 0 over; a query past the end and a NaN hand over every frame
    assert own[0].all() and own[1].all()
    assert not own[2, 0] and own[2, 1:].all()
    assert not own[3, 0] and own[3, 1:].all()
    assert not own[4, :T - 1].any() and own[4, T - 1]
    assert not own[5].any() and not own[6].any()
    assert rs.need_count(tq) == int((~own[:, 0]).sum()) - 1  # (every query that does not own frame 0, but the NaN)
    assert [rs.need_count(tq[i:i + 1]) for i in range(7)] == [0, 0, 1, 1, 1 if T > 1 else 0, 1, 0]
    # every frame has exactly one owner, and that owner's pass estimates it: the forward pass by the same expression, the reversed
    # pass by its own causal rule on the flipped query time (at the query frame both do, and the forward value wins)
    rev_valid = rs.reversed_pass_valid(tq, T)
    finite = ~np.isnan(tq)
    assert (rev_valid | own)[finite].all() and not rev_valid[~finite].any()
    assert (rev_valid[finite] >= ~own[finite]).all()
    on_centre = (centre[None, :] == tq.astype(np.float64)[:, None])
    assert (own & rev_valid)[on_centre].all()
    # merge(): the forward value where owned, the reversed pass's frame T-1-g elsewhere; mode 1 fills the forward-owned frames
    n = len(tq)
    q = np.zeros((1, n, 3), dtype=np.float32)
    q[0, :, 0] = tq
    g = np.arange(T, dtype=np.float32)

    def passes(base):  # traj [1, n, 2, T], vis, depth [1, n, 1, T]: base + 100 * channel + frame (of the pass's own clip)
        return [np.stack([base + g, base + 100 + g])[None, None].repeat(n, 1), np.broadcast_to(base + 200 + g, (1, n, 1, T)).copy(),
                np.broadcast_to(base + 300 + g, (1, n, 1, T)).copy()]

    fwd, rev = passes(1000), passes(2000)
    for mode in (0, 1):
        traj, vis, dep = rs.merge(q, fwd if mode == 0 else None, rev, mode)
        for i in range(n):
            for f in range(T):
                if own[i, f]:
                    exp = (1000 + f, 1100 + f, 1200 + f, 1300 + f) if mode == 0 else (0.0, 0.0, -10.0, 0.0)
                else:
                    r = T - 1 - f
                    exp = (2000 + r, 2100 + r, 2200 + r, 2300 + r)
                assert (traj[0, i, 0, f], traj[0, i, 1, f], vis[0, i, 0, f], dep[0, i, 0, f]) == exp, (mode, i, f)


def test_query_map_is_one_f32_subtraction():
    q = np.array([[0.5, 3.0, 4.0], [0.50000006, 1.0, 2.0], [12.5, 7.0, 9.0], [np.nan, 5.0, 6.0]], dtype=np.float32)
    for T in (1, 16, 32):
        r = rs.flip_queries(q, T)
        assert r.dtype == np.float32 and np.array_equal(r[:, 1:], q[:, 1:])
        assert np.array_equal(r[:3, 0], (np.float32(T) - q[:3, 0]).astype(np.float32)) and np.isnan(r[3, 0])
        rt = rs.flip_queries(torch.from_numpy(q), T)
        assert np.array_equal(rt.numpy(), r, equal_nan=True)
    assert rs.flip_queries(q, 16)[1, 0] == np.float32(15.5)  # 16 - 0.50000006 rounds to the centre of frame 15
    x = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
    assert np.array_equal(rs.time_reverse(x)[:, 0], x[:, 2]) and np.array_equal(rs.time_reverse(rs.time_reverse(x)), x)


def _load(path, name):
    import importlib.util

    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(GOLD), "..", path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_and_evaluate_arguments():
    demo = _load("demo/demo.py", "demo_bidir_args")
    a = demo.parse_args(["--synthetic", "--frames", "32", "--bidirectional", "--query-frame", "12", "--vis", "out"])
    assert a.bidirectional and a.query_frame == 12
    assert demo.plan(a)[1]["estimation_directions"] == [1, -1]
    a = demo.parse_args(["--synthetic"])
    assert not a.bidirectional and a.query_frame is None and demo.plan(a)[1]["estimation_directions"] == [1]
    with pytest.raises(SystemExit):
        demo.parse_args(["--synthetic", "--query-frame", "-1"])
    ev = _load("tools/evaluate.py", "evaluate_bidir_args")
    assert ev.parse_args(["DIR", "--synthetic", "--bidirectional"])[1].bidirectional
    assert not ev.parse_args(["DIR", "--synthetic"])[1].bidirectional


def test_head_accepts_the_directions_and_refuses_a_call_of_its_own():
    """Host logic only (no GPU): which estimation_directions the head takes, and that one causal pass is never silently returned where
    -1 is configured and L4P_VideoMAE.forward has not selected the pass."""
    from l4p_amd.models.task_heads.sparse_heads import VideoMAETrack2DSamHead

    kw = dict(estimate_vis=True, estimate_depth=True, prompt_using_features=True, attend_to_past=True,
              modify_pointlabels_for_windowing=True, depth_fn="exp", vis_fn="linear")
    head = VideoMAETrack2DSamHead(estimation_directions=[1], **kw)
    assert head.pass_direction() is None
    for dirs in ([1, -1], [-1, 1], [-1]):
        head = VideoMAETrack2DSamHead(estimation_directions=dirs, **kw)
        with pytest.raises(RuntimeError, match=r"L4P_VideoMAE\.forward"):
            head.pass_direction()
        for d in (1, -1):
            with head.select_direction(d):
                assert head.pass_direction() == d
        assert head._direction is None
    for dirs in ([], [1, 1], [2], [1, -1, 1]):
        with pytest.raises(ValueError, match="estimation_directions"):
            VideoMAETrack2DSamHead(estimation_directions=dirs, **kw).pass_direction()
