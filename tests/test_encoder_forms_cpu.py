"""The fixtures of tests/test_encoder_forms_gpu.py (tools/gen_golden_encoder_forms.py wrote them from the real reference at the
full model's width and depth 3): the oracle reproduces the recorded fp32 reference features at this geometry, and the drift
table the GPU bars are taken from is complete."""
import json
import math
import os

import numpy as np
import torch

from l4p_amd.weights import ModelCfg, seeded_state_dict
from tests.golden_utils import make_batch, sample_indices

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEEDS = (1234, 4321)


def forms_cfg() -> ModelCfg:
    """Full width, three blocks: every kernel shape is one the full model runs (only the encoder is used)."""
    return ModelCfg(dim=1408, depth=3, heads=16, mlp_hidden=6144, hooks=(1, 2, 3, 3))


def forms_drift() -> dict:
    with open(os.path.join(GOLD, "encoder_forms_drift.json")) as f:
        return json.load(f)


def test_oracle_reproduces_reference_features_at_depth3():
    """max |oracle - reference| <= 1e-3 max |reference| (the project's f32 bar) on the sampled values of every layer, both clips."""
    from oracle.l4p_oracle import encoder_forward

    cfg = forms_cfg()
    sd = seeded_state_dict(cfg, tasks=[])
    g = np.load(os.path.join(GOLD, "encoder_forms_T16.npz"))
    assert sorted(g.files) == sorted(f"clip{s}_feat{li}" for s in SEEDS for li in range(cfg.depth + 1))
    for seed in SEEDS:
        with torch.no_grad():
            feats = encoder_forward(sd, make_batch(16, 0, seed=seed)["rgb_b3thw"], cfg)
        assert len(feats) == cfg.depth + 1
        for li, f in enumerate(feats):
            assert tuple(f.shape) == (1, cfg.tokens, cfg.dim)
            v = f.reshape(-1)
            want = torch.from_numpy(g[f"clip{seed}_feat{li}"])
            assert want.numel() == 4096
            err = float((v[sample_indices(v.numel())] - want).abs().max() / want.abs().max())
            print(f"clip {seed} layer {li}: oracle vs recorded reference {err:.2e}")
            assert err <= 1e-3, (seed, li, err)


def test_drift_table_is_complete():
    rep = forms_drift()
    for dt in ("bf16", "f16"):
        for seed in SEEDS:
            for li in range(4):
                e = rep[dt][f"clip{seed}"][f"feat{li}"]
                for k in ("rel_l2", "row_max"):
                    assert math.isfinite(e[k]) and e[k] >= 0.0, (dt, seed, li, k, e)
                    if li >= 1:
                        assert e[k] > 0.0, (dt, seed, li, k, e)
                assert e["row_max"] >= e["rel_l2"] * 0.999  # (a maximum over rows is no smaller than the pooled figure)
