"""Reference figures for the encoder's residual hand-over forms (tests/test_encoder_forms_{cpu,gpu}.py), from the REAL reference
(runs only where /root/reference exists).

Geometry: the full model's width at depth 3 - ModelCfg(dim=1408, depth=3, heads=16, mlp_hidden=6144) on the default 16 x 224 x 224
clip (2048 tokens) - so that every GEMM / attention / LayerNorm shape is one the full model runs, while a forward is three blocks.
The reference's VideoMAEEncoder is built at this geometry with the name-seeded weights and run on CPU three ways (fp32, autocast
bfloat16, autocast float16) on two clips (make_batch(16, 0, seed=1234 / 4321)).

A. tests/golden/encoder_forms_drift.json - per autocast dtype, per clip, per layer 0..3 (layer 3 = norm(x), features_list[-1]):
   ``rel_l2`` over the whole tensor and ``row_max``, the largest per-token-row relative L2 error over the 2048 rows, of the
   autocast run against the fp32 run.  The GPU tests' bars are these figures times the standing margins of tests/golden_utils.py.
B. tests/golden/encoder_forms_T16.npz - the fp32 reference features of both clips at sample_indices(numel), 4096 values per layer:
   pins oracle.l4p_oracle.encoder_forward at this geometry where the reference is absent (tests/test_encoder_forms_cpu.py).

Asserted on the spot: the oracle in fp32 equals the reference's fp32 run within the f32 bar (max |diff| <= 1e-3 max |ref|).

  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_encoder_forms.py        (~1 minute)
Only data is written."""
from __future__ import annotations

import json
import os
import sys
import time

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from l4p_amd.weights import ModelCfg, encoder_schema, seeded_state_dict
from tests.golden_utils import make_batch, sample_indices
from tools.gen_golden import install_stubs

GOLD = os.path.join(ROOT, "tests", "golden")
SEEDS = (1234, 4321)
AC = {"bf16": torch.bfloat16, "f16": torch.float16}


def forms_cfg() -> ModelCfg:
    return ModelCfg(dim=1408, depth=3, heads=16, mlp_hidden=6144, hooks=(1, 2, 3, 3))


def build_encoder(cfg: ModelCfg):
    """The reference's VideoMAEEncoder as L4P_VideoMAE.__init__ builds it, at ``cfg``'s depth."""
    from functools import partial

    from l4p.models.l4p_videomae import VideoMAEEncoder

    enc = VideoMAEEncoder(
        img_size=cfg.img, patch_size=cfg.patch[1], in_chans=3, num_classes=0, embed_dim=cfg.dim, depth=cfg.depth,
        num_heads=cfg.heads, mlp_ratio=48 / 11, qkv_bias=True, qk_scale=None, drop_rate=0, attn_drop_rate=0,
        drop_path_rate=0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.0, tubelet_size=2,
        use_learnable_pos_emb=False, with_cp=False, all_frames=16, cos_attn=False)
    return enc.eval()


def drift(a: torch.Tensor, b: torch.Tensor) -> dict:
    """a: autocast run, b: fp32 run, [1, P, C] -> whole-tensor rel-L2 and the largest per-row rel-L2."""
    a, b = a.detach().double()[0], b.detach().double()[0]
    rows = (a - b).norm(dim=-1) / b.norm(dim=-1)
    return {"rel_l2": float((a - b).norm() / b.norm()), "row_max": float(rows.max())}


def main():
    from oracle.l4p_oracle import encoder_forward

    install_stubs()
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count() or 8)
    cfg = forms_cfg()
    enc = build_encoder(cfg)
    sd = seeded_state_dict(cfg, tasks=[])
    assert set(sd) == set(encoder_schema(cfg))
    enc.load_state_dict({k[len("video_encoder."):]: v for k, v in sd.items()}, strict=True)
    report = {"what": "reference VideoMAEEncoder (dim 1408, depth 3) under torch.autocast('cpu', dtype) vs its own fp32 run: "
                      "rel_l2 over the whole tensor, row_max = largest per-token-row rel-L2",
              "torch": torch.__version__, "bf16": {}, "f16": {}}
    npz = {}
    for seed in SEEDS:
        rgb = make_batch(16, 0, seed=seed)["rgb_b3thw"]
        t0 = time.time()
        with torch.no_grad():
            f32 = [f.float() for f in enc(rgb.clone())]
            of = encoder_forward(sd, rgb, cfg)
        assert len(f32) == cfg.depth + 1 == len(of)
        for li in range(cfg.depth + 1):
            e = float((of[li] - f32[li]).abs().max() / f32[li].abs().max())
            print(f"clip {seed} layer {li}: oracle vs reference fp32, max |diff| / max |ref| = {e:.2e}", flush=True)
            assert e <= 1e-3, (seed, li, e)
            v = f32[li].reshape(-1)
            npz[f"clip{seed}_feat{li}"] = v[sample_indices(v.numel())].numpy().astype(np.float32)
        for name, dt in AC.items():
            with torch.no_grad(), torch.autocast("cpu", dtype=dt):
                f16 = enc(rgb.clone())
            report[name][f"clip{seed}"] = {f"feat{li}": drift(f16[li].float(), f32[li]) for li in range(cfg.depth + 1)}
            print(name, f"clip{seed}", json.dumps(report[name][f"clip{seed}"]), flush=True)
        print(f"clip {seed}: {time.time() - t0:.1f}s", flush=True)
    with open(os.path.join(GOLD, "encoder_forms_drift.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(GOLD, "encoder_forms_T16.npz"), **npz)


if __name__ == "__main__":
    main()
