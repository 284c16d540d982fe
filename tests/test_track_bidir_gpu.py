"""GPU: tracking in both time directions through L4P_VideoMAE.forward (estimation_directions [1, -1] / [-1]) on the MINI geometry.

The f32 engine is held to the live oracle composition and to the reference-pinned fixture (tests/golden/mini_T32_bidir.npz) at the
bar of tests/test_track_gpu.py: 1e-3 relative-to-max on the outputs, the reversed pass's integer state bit for bit (the fixture's
re-seed margin is >= 1e-3, tools/gen_golden_bidir.py).  Every precision is held to EXACT identities instead of a drift record of
its own: what the model returns for [1, -1] is, frame by frame, what the same model returns for [1] on the clip and on the
time-flipped clip - so whatever holds for the 16-bit engines' causal pass (tests/test_track_gpu.py) holds for both directions."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd.weights import ModelCfg, seeded_state_dict
from tests import track_bidir_restate as rs
from tests.golden_utils import make_batch
from tests.test_encoder_dpt_gpu import build

KEYS = list(rs.KEYS)
_MODELS = {}


def model_of(precision):
    """One model per precision for the whole module (the tests set what they change on it and put it back)."""
    if precision not in _MODELS:
        cfg = ModelCfg.mini()
        _MODELS[precision] = build(cfg, seeded_state_dict(cfg), precision)
    return _MODELS[precision]


def run(model, dirs, batch, tasks=("track_2d",), trace=False, **net_attrs):
    """model.forward with the tracker's estimation_directions = dirs -> (outputs, trace or None).  Everything set is put back."""
    net = model.l4p_model
    head = net.task_heads["track_2d"]
    saved = {k: getattr(net, k) for k in net_attrs}
    saved_dirs, saved_trace = head.estimation_directions, head.trace
    try:
        for k, v in net_attrs.items():
            setattr(net, k, v)
        head.estimation_directions = list(dirs)
        head.trace = [] if trace else None
        with torch.no_grad():
            out = model.forward({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, list(tasks))
        torch.cuda.synchronize()
        return out, head.trace
    finally:
        head.estimation_directions, head.trace = saved_dirs, saved_trace
        for k, v in saved.items():
            setattr(net, k, v)


def golden_batch():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini_T32_bidir.npz"))
    return make_batch(32, 12, int(gold["seed"])), gold


def owned(batch):
    """bool [B, N, 1, T] on the CPU: the frames the forward pass owns."""
    q = batch["track_2d_pointquerries_bn3"].float().numpy()
    return torch.from_numpy(rs.forward_owned(q[..., 0], batch["rgb_b3thw"].shape[2]))[:, :, None, :]


def assert_identities(out, fwd, rev, batch, what=""):
    """Forward-owned frames: the [1] run's; reversed-owned frames: the [1] run's on the flipped batch, mirrored.  fwd None: the fill
    values ([-1] alone)."""
    own = owned(batch)
    assert own.any() and (~own).any()
    for k in KEYS:
        y, r = out[k].cpu(), rev[k].cpu().flip(-1)
        f = fwd[k].cpu() if fwd is not None else torch.full_like(y, rs.FILL[k])
        m = own.expand_as(y)
        assert torch.equal(y[m], f[m]), (what, k, "forward-owned frames")
        assert torch.equal(y[~m], r[~m]), (what, k, "reversed-owned frames")


def test_f32_engine_vs_oracle_composition_and_reference_fixture(dev):
    from tests.test_track_bidir_cpu import oracle_composition

    batch, omerged, otrace, gold = oracle_composition()
    out, trace = run(model_of("32-true"), [1, -1], batch, trace=True)
    for k in KEYS:
        y = out[k].float().cpu()
        for name, ref in (("oracle", omerged[k]), ("fixture", torch.from_numpy(gold[k]))):
            assert y.shape == ref.shape
            err = float((y - ref).abs().max() / ref.abs().max())
            print(f"{k} vs {name}: {err:.2e}")
            assert err <= 1e-3, (k, name, err)
    assert [t["direction"] for t in trace] == [1, 1, 1, -1, -1, -1] and [t["window"] for t in trace] == [0, 1, 2, 0, 1, 2]
    for w, tr in enumerate(trace[3:]):
        assert torch.equal(tr["labels"].cpu(), otrace[w]["labels"]), w
        assert torch.equal(tr["prompt_labels"].cpu(), otrace[w]["prompt_labels"]), w
        assert torch.equal(tr["valid_t"].cpu().bool(), otrace[w]["valid_t"]), w
        assert torch.equal(tr["queries"][:, 0].cpu(), otrace[w]["queries"][:, 0]), w
        assert np.array_equal(tr["labels"].cpu().numpy(), gold[f"rev_trace{w}_labels"]), w
        assert np.array_equal(tr["prompt_labels"].cpu().numpy(), gold[f"rev_trace{w}_prompt_labels"]), w
        assert np.array_equal(tr["queries"][:, 0].cpu().numpy(), gold[f"rev_trace{w}_queries"][:, 0]), w
        assert np.array_equal(tr["valid_t"].cpu().numpy().astype(bool), gold[f"rev_trace{w}_valid_t"]), w
        if w < 2:
            assert torch.equal(tr["best_vis_id"].cpu().long(), otrace[w]["best_vis_id"]), w
            assert np.array_equal(tr["best_vis_id"].cpu().numpy().astype(np.int64), gold[f"rev_trace{w}_best_vis_id"]), w


@pytest.mark.parametrize("precision", ["32-true", "bf16", "16-mixed"])
def test_both_directions_are_the_two_causal_runs_frame_by_frame(dev, precision):
    model = model_of(precision)
    batch, _ = golden_batch()
    fwd, _ = run(model, [1], batch)
    rev, _ = run(model, [1], rs.flip_batch(batch))
    for dirs in ([1, -1], [-1, 1]):
        out, _ = run(model, dirs, batch)
        assert_identities(out, fwd, rev, batch, str(dirs))
        # the returned encoder features are the forward pass's
        assert len(out["enc_features_bpc_2dlist"]) == len(fwd["enc_features_bpc_2dlist"]) == 3
        for a, b in zip(out["enc_features_bpc_2dlist"], fwd["enc_features_bpc_2dlist"]):
            assert torch.equal(a.f32(-1), b.f32(-1))
    # [-1] alone: no forward tracker, the recursion's fill values on the frames it would own
    out, trace = run(model, [-1], batch, trace=True)
    assert_identities(out, None, rev, batch, "[-1]")
    assert [t["direction"] for t in trace] == [-1, -1, -1]


def test_queries_on_frame_0_skip_the_reversed_pass(dev):
    model = model_of("bf16")
    batch, _ = golden_batch()
    batch["track_2d_pointquerries_bn3"][..., 0] = 0.5
    fwd, t1 = run(model, [1], batch, trace=True)
    out, t2 = run(model, [1, -1], batch, trace=True)
    for k in KEYS:
        assert torch.equal(out[k], fwd[k]), k
    assert len(t1) == len(t2) == 3 and all(t["direction"] == 1 for t in t2) and all("direction" not in t for t in t1)
    # [-1] with nothing before any query: the fill values, no pass at all
    out, t3 = run(model, [-1], batch, trace=True)
    assert t3 == []
    for k in KEYS:
        assert out[k].shape == fwd[k].shape and bool((out[k] == rs.FILL[k]).all()), k


def test_two_clips_with_their_own_queries(dev):
    """B = 2, different clips and queries, the second clip with every query on frame 0 (no reversed frame of its own)."""
    model = model_of("32-true")
    b0, _ = golden_batch()
    b1 = make_batch(32, 12, 77)
    b1["track_2d_pointquerries_bn3"][..., 0] = 0.5
    both = {k: torch.cat([b0[k], b1[k]], dim=0) for k in b0}
    out, _ = run(model, [1, -1], both)
    fwd, _ = run(model, [1], both)
    rev, _ = run(model, [1], rs.flip_batch(both))
    own = owned(both)
    assert own[1].all() and not own[0].all()
    for k in KEYS:  # exactly the two causal runs of the same batch; the second clip is its forward result
        y, m = out[k].cpu(), own.expand_as(out[k])
        assert torch.equal(y[m], fwd[k].cpu()[m]) and torch.equal(y[~m], rev[k].cpu().flip(-1)[~m]), k
        assert torch.equal(y[1], fwd[k].cpu()[1]), k
    for i, b in enumerate((b0, b1)):  # each clip as its B = 1 result (the encoder's row count differs: equal to f32 rounding)
        one, _ = run(model, [1, -1], b)
        for k in KEYS:
            a, r = out[k][i].cpu(), one[k][0].cpu()
            assert (a - r).abs().max() <= 1e-4 * r.abs().max(), (i, k, float((a - r).abs().max()))


def test_window_batch_2_equals_window_batch_1(dev):
    """Through forward_windows_sharded: the same two-pass structure exactly, the values of the window-by-window loop to f32 rounding
    (tests/test_sharded_windows_gpu.py: batched windows change GEMM row counts)."""
    model = model_of("32-true")
    batch, _ = golden_batch()
    one, _ = run(model, [1, -1], batch)
    out, trace = run(model, [1, -1], batch, trace=True, window_batch=2)
    fwd, _ = run(model, [1], batch, window_batch=2)
    rev, _ = run(model, [1], rs.flip_batch(batch), window_batch=2)
    assert_identities(out, fwd, rev, batch, "window_batch 2")
    assert [t["direction"] for t in trace] == [1, 1, 1, -1, -1, -1]
    for k in KEYS:
        a, r = out[k].cpu(), one[k].cpu()
        assert (a - r).abs().max() <= 1e-4 * r.abs().max(), (k, float((a - r).abs().max()))


def test_one_window_clip(dev):
    """T = 16 on the windowed path (always_use_windowed_version=True): one window per pass."""
    model = model_of("16-mixed")
    assert model.l4p_model.always_use_windowed_version
    batch = make_batch(16, 12)
    fwd, _ = run(model, [1], batch)
    rev, _ = run(model, [1], rs.flip_batch(batch))
    out, trace = run(model, [1, -1], batch, trace=True)
    assert_identities(out, fwd, rev, batch, "T 16")
    assert [(t["direction"], t["window"]) for t in trace] == [(1, 0), (-1, 0)]


def test_more_queries_than_max_queries(dev):
    """The chunked path of forward_windowed (12 queries in chunks of 5, 5, 2), both passes."""
    model = model_of("bf16")
    head = model.l4p_model.task_heads["track_2d"]
    batch, _ = golden_batch()
    saved = head.max_queries
    try:
        head.max_queries = 5
        fwd, _ = run(model, [1], batch)
        rev, _ = run(model, [1], rs.flip_batch(batch))
        out, trace = run(model, [1, -1], batch, trace=True)
    finally:
        head.max_queries = saved
    assert_identities(out, fwd, rev, batch, "chunks")
    assert [t["direction"] for t in trace] == [1] * 9 + [-1] * 9


def test_head_on_its_own_refuses_and_names_the_model_entry(dev):
    model = model_of("bf16")
    head = model.l4p_model.task_heads["track_2d"]
    batch, _ = golden_batch()
    q, lab = batch["track_2d_pointquerries_bn3"].to(dev), batch["track_2d_pointlabels_bn"].to(dev)
    saved = head.estimation_directions
    try:
        for dirs in ([1, -1], [-1]):
            head.estimation_directions = dirs
            for entry in (head.forward_windowed, head.forward_windowed_core):
                with pytest.raises(RuntimeError, match=r"L4P_VideoMAE\.forward"):
                    entry([None, None, None], q, lab, time_strides=torch.tensor([0, 8, 16]))
        head.estimation_directions = [1, 2]
        with pytest.raises(ValueError, match="estimation_directions"):
            model.forward(batch, ["track_2d"])
    finally:
        head.estimation_directions = saved


def test_causal_model_is_unchanged_by_a_two_direction_run(dev):
    """[1] before and after a [1, -1] run on the same model object: same trace length, same outputs - no state leaks between modes."""
    model = model_of("bf16")
    head = model.l4p_model.task_heads["track_2d"]
    batch, _ = golden_batch()
    before, t_before = run(model, [1], batch, trace=True)
    run(model, [1, -1], batch, trace=True)
    assert head._direction is None
    after, t_after = run(model, [1], batch, trace=True)
    assert len(t_before) == len(t_after) == 3 and all(set(a) == set(b) and "direction" not in a for a, b in zip(t_before, t_after))
    for k in KEYS:
        assert torch.equal(before[k], after[k]), k
