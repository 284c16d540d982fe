"""Tracking in both time directions pinned to the REAL reference (runs only where /root/reference exists, on the CPU):

tests/golden/mini_T32_bidir.npz - mini geometry, make_batch(32, 12, seed): the imported reference (estimation_directions=[1], the
only direction it implements) on the clip and on its time-flip with the mapped queries, merged by the rule of
tests/track_bidir_restate.py - the recipe of the reference's own assert (sparse_heads.py:242-245).

  * the three merged tracker outputs in full (12 tracks x 32 frames);
  * the reversed pass's integer state per window (rev_trace{w}_*: labels, prompt labels, re-seeded query times from the reference;
    validity masks and the re-seed argmax index from the oracle on the reference's features, asserted equal where both exist);
  * min_margin: the smallest gap between the best and the second-best visibility over every re-seed argmax of BOTH passes, relative
    to the largest |visibility| either pass estimated.  (Rows of tracks that are not alive yet hold the fill value -10 in every
    overlap frame: an exact tie that every implementation resolves to index 0, not a near-tie; they are left out.)  Asserted
    >= 1e-3, over seeds 1234, 1235, ... until one holds, so that the bit-exact integer checks of the tests cannot rest on a near-tie;
  * oracle_rel_err: max |oracle - reference| over the merged outputs relative to the largest |reference|, asserted <= 1e-4 (the bar
    of tools/gen_golden.py), the oracle (oracle/l4p_oracle.py) composed by the same restatement.

  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bidir.py
Only arrays and numbers are written."""
from __future__ import annotations

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from l4p_amd.weights import ModelCfg, seeded_state_dict
from tests import track_bidir_restate as rs
from tests.golden_utils import make_batch
from tools.gen_golden import build_reference, install_stubs
from tools.gen_golden_full_autocast import oracle_trace, run_ref, trace_arrays

GOLD = os.path.join(ROOT, "tests", "golden")
T, NQ, FIRST_SEED, MARGIN = 32, 12, 1234, 1e-3


class ArgmaxRows:
    """Records the rows every re-seed argmax of oracle.l4p_oracle.track_windowed chooses from (its only torch.argmax)."""

    def __init__(self):
        self.rows, self._orig = [], torch.argmax

    def __enter__(self):
        def spy(x, *a, **kw):
            self.rows.append(x.detach().clone())
            return self._orig(x, *a, **kw)

        torch.argmax = spy
        return self

    def __exit__(self, *exc):
        torch.argmax = self._orig


def margin_of(rows) -> tuple:
    """-> (smallest best - second-best gap, largest |estimated visibility|) over [N, overlap] rows; all-fill rows left out."""
    gap, top = float("inf"), 0.0
    for x in rows:
        est = x != rs.FILL["track_2d_vis_est_bn1t"]
        if est.any():
            top = max(top, float(x[est].abs().max()))
        alive = est.any(dim=-1)
        if alive.any():
            s = torch.sort(x[alive], dim=-1, descending=True).values
            gap = min(gap, float((s[:, 0] - s[:, 1]).min()))
    return gap, top


def one_seed(model, sd, cfg, seed: int):
    from oracle.l4p_oracle import OracleModel

    batch = make_batch(T, NQ, seed)
    strides = list(range(0, T - cfg.frames + 1, 8))
    passes, rows = {}, []

    def run_reference(b):
        out, trace, feats = run_ref(model, b, ["track_2d"], False)
        with ArgmaxRows() as spy:
            _, otr = oracle_trace(sd, cfg, feats, b, strides, trace)  # (asserts the oracle's integer state equal to the reference's)
        assert len(spy.rows) == len(strides) - 1, len(spy.rows)
        rows.extend(spy.rows)
        passes["fwd" if b is batch else "rev"] = (trace, otr)
        return out

    merged = rs.compose(run_reference, batch)
    gap, top = margin_of(rows)
    min_margin = gap / top
    print(f"seed {seed}: smallest re-seed gap {gap:.4g}, largest |vis| {top:.4g} -> min_margin {min_margin:.3g}", flush=True)
    if min_margin < MARGIN:
        return None
    with torch.no_grad():
        omerged = rs.compose(lambda b: OracleModel(sd, cfg).forward(b, ["track_2d"]), batch)
    err = max(float((omerged[k] - merged[k]).abs().max() / merged[k].abs().max()) for k in rs.KEYS)
    print(f"seed {seed}: max |oracle - reference| over the merged outputs, relative: {err:.2e}", flush=True)
    assert err <= 1e-4, err
    npz = {k: merged[k].numpy() for k in rs.KEYS}
    npz.update({"rev_" + k: v for k, v in trace_arrays(*passes["rev"]).items()})
    npz.update(seed=np.int64(seed), min_margin=np.float64(min_margin), oracle_rel_err=np.float64(err))
    return npz


def main():
    install_stubs()
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count() or 8)
    cfg = ModelCfg.mini()
    model = build_reference(cfg)
    sd = seeded_state_dict(cfg)
    model.load_state_dict(sd, strict=True)
    for seed in range(FIRST_SEED, FIRST_SEED + 16):
        npz = one_seed(model, sd, cfg, seed)
        if npz is not None:
            np.savez_compressed(os.path.join(GOLD, "mini_T32_bidir.npz"), **npz)
            print(f"wrote mini_T32_bidir.npz (seed {seed})")
            return
    raise SystemExit("no seed with a re-seed margin of 1e-3")


if __name__ == "__main__":
    main()
