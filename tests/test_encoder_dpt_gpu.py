"""End-to-end parity on the GPU: encoder + dense DPT heads of the MINI geometry (704-wide, 4 blocks)
against (a) the oracle run live on the host CPU and (b) the golden vectors produced by the real
reference (tests/golden/mini_T16_all.npz).

Tolerances: L4P_F32 engine — 1e-3 * max|ref| (north_star; measured ~1e-5).  L4P_BF16 engine — the
bf16 storage/MFMA drift of a 4-block encoder + 20-conv decoder: rel-L2 <= 3e-2 (reported, not the
1e-3 gate; see DESIGN.md "precision modes").
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd._lib import L4P_BF16, L4P_F32
from l4p_amd.models.utils import build_model
from l4p_amd.weights import ModelCfg, seeded_state_dict
from tests.golden_utils import make_batch, sample_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mini():
    cfg = ModelCfg.mini()
    sd = seeded_state_dict(cfg)
    return cfg, sd


def build(cfg, sd, precision):
    m = build_model(os.path.join(ROOT, "configs", "model.yaml"), precision=precision, model_cfg=cfg)
    # hooks of the mini geometry
    for k, h in m.l4p_model.task_heads.items():
        if hasattr(h, "hooks_idx"):
            h.hooks_idx = list(cfg.hooks)
    m.l4p_model.task_heads["camray"].use_intrinsics = True  # as demo.py:215 (cv2-free path)
    m.load_state_dict({"l4p_model." + k: v for k, v in sd.items()})
    return m


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


_ORACLE_T16 = {}


@pytest.mark.parametrize("precision,tol_max,tol_l2", [("32-true", 1e-3, 1e-3), ("bf16", None, 3e-2), ("16-mixed", None, 4e-3)])
def test_mini_encoder_and_dense_heads_vs_oracle_and_golden(dev, mini, precision, tol_max, tol_l2):
    from oracle.l4p_oracle import OracleModel, encoder_forward

    cfg, sd = mini
    model = build(cfg, sd, precision)
    batch = make_batch(16, 8)
    gold = np.load(os.path.join(GOLD, "mini_T16_all.npz"))
    tasks = ["depth", "flow_2d_backward", "dyn_mask", "camray"]
    with torch.no_grad():
        out = model.forward({k: v.clone() for k, v in batch.items()}, tasks)
        feats = out["enc_features_bpc_2dlist"][0]
        if "oout" not in _ORACLE_T16:  # (the CPU oracle's forward is the same for every engine precision: once)
            _ORACLE_T16["ofeats"] = encoder_forward(sd, batch["rgb_b3thw"], cfg)
            _ORACLE_T16["oout"] = OracleModel(sd, cfg, use_intrinsics=True).forward(batch, tasks)
        ofeats, oout = _ORACLE_T16["ofeats"], _ORACLE_T16["oout"]
    torch.cuda.synchronize()
    # encoder hooks vs oracle (full tensors) and vs the reference's golden samples
    drift = {}
    for li in cfg.hooks:
        f = feats.f32(li).cpu()
        drift[f"feat{li}"] = rel_l2(f, ofeats[li])
        assert rel_l2(f, ofeats[li]) <= tol_l2, (li, rel_l2(f, ofeats[li]))
        if tol_max is not None:
            assert (f - ofeats[li]).abs().max() <= tol_max * ofeats[li].abs().max()
            g = torch.from_numpy(gold[f"feat{li}"])
            s = f.reshape(-1)[sample_indices(f.numel())]
            assert (s - g).abs().max() <= tol_max * g.abs().max(), li
    for key in ["depth_est_b1thw", "flow_2d_backward_est_b2thw", "dyn_mask_est_b1thw", "traj3d_est_b16t",
                "traj3d_intrinsics_est_b16t"]:
        y, ref = out[key].float().cpu(), oout[key]
        assert y.shape == ref.shape, key
        e = rel_l2(y, ref)
        drift[key] = e
        assert e <= tol_l2, (key, e)
        if tol_max is not None:
            assert (y - ref).abs().max() <= tol_max * ref.abs().max(), key
            g = torch.from_numpy(gold[key]).reshape(-1)
            s = y.reshape(-1)[sample_indices(y.numel())] if y.numel() > 4096 else y.reshape(-1)
            assert (s - g).abs().max() <= tol_max * g.abs().max(), key
    if tol_max is None:
        # the bf16 engine against the reference's OWN autocast drift on these inputs (tools/gen_golden_full_autocast.py)
        from tests.golden_utils import assert_bf16_within_reference_drift

        assert_bf16_within_reference_drift(drift, "mini_T16_all", precision=precision)


def test_dpt_workspace_too_small_is_refused_and_its_size_ignores_the_fold_knob(dev, mini, knob, monkeypatch):
    """l4p_dpt_forward on a workspace declared half as large as l4p_dpt_workspace_bytes asks: L4P_E_INVALID, "workspace too small"
    (the pointer is the full buffer: nothing can be overrun whatever the code does); the full-size call on the same buffer then
    equals the model's own forward bit for bit.  And the size is that of the unfolded form whatever dpt_fold_rn says (the knob may
    change between sizing and a forward): a full-resolution head and camray."""
    import ctypes as C

    from l4p_amd import _lib
    from l4p_amd.weights import actpost_of, fusion_of

    cfg, sd = mini
    model = build(cfg, sd, "bf16")
    heads = model.l4p_model.task_heads
    eng = heads["depth"]._rt.engine
    calls = {}
    real = eng.dpt_forward

    def spy(task, hooks, *args):
        calls[task] = (hooks, args, real(task, hooks, *args))
        return calls[task][2]

    monkeypatch.setattr(eng, "dpt_forward", spy)
    batch = make_batch(16, 2)
    with torch.no_grad():
        fresh = model.forward({k: v.clone() for k, v in batch.items()}, ["depth", "camray"])
    torch.cuda.synchronize()
    lib = _lib.load()
    for task in ("depth", "camray"):
        hooks, (out_ch, actpost, fusion, osz, post_exp), want = calls[task]
        assert actpost == actpost_of(task) and fusion == fusion_of(task)
        B = hooks[0].shape[0]
        dc = eng.dpt_cfg(out_ch, actpost, fusion, osz, post_exp)
        sizes, default = {}, int(lib.l4p_get_knob(b"dpt_fold_rn"))
        for v in (0, 1, 2):
            knob("dpt_fold_rn", v)
            sizes[v] = int(lib.l4p_dpt_workspace_bytes(eng.handle, C.byref(dc), B))
        knob("dpt_fold_rn", default)  # (what the model's forward above ran with)
        need = sizes[default]
        assert need > 0 and sizes[0] == need and sizes[2] == need, sizes
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        hs = [h.contiguous() for h in hooks]
        hp = (C.c_void_p * 4)(*[h.data_ptr() for h in hs])
        out = torch.zeros((B, out_ch) + tuple(osz), dtype=torch.float32, device="cuda")
        args = (eng.handle, torch.cuda.current_stream().cuda_stream, task.encode(), C.byref(dc), hp, B, ws.data_ptr())
        rc = lib.l4p_dpt_forward(*args, need // 2, out.data_ptr())
        assert rc == _lib.L4P_E_INVALID and "workspace too small" in lib.l4p_last_error().decode(), (rc, lib.l4p_last_error())
        _lib.check(lib.l4p_dpt_forward(*args, need, out.data_ptr()), "l4p_dpt_forward")
        torch.cuda.synchronize()
        assert torch.equal(out, want), task
        if task == "depth":
            assert torch.equal(out[:, :1], fresh["depth_est_b1thw"])


@pytest.mark.parametrize("precision", ["bf16", "16-mixed"])
def test_dpt_head_with_the_upsampling_fused_into_the_head_conv(dev, probe_kernels, mini, precision, knob):
    """l4p_dpt_forward: interpolate -> head conv (dpt_head.py:79-84) with the up-sampling formed in the conv's loader (knob conv_ups,
    default) against up-sample-then-convolve: every dense output bit for bit, and the fused form is the one that ran."""
    import ctypes as C

    from l4p_amd import _lib

    cfg, sd = mini
    model = build(cfg, sd, precision)
    batch = make_batch(16, 2)
    tasks = ["depth", "flow_2d_backward", "dyn_mask"]
    lib = _lib.load()
    outs = {}
    for v in (1, 0):
        knob("conv_ups", v)
        torch.cuda.synchronize()
        lib.l4p_prof_reset()
        lib.l4p_prof_enable(1)
        with torch.no_grad():
            o = model.forward({k: t.clone() for k, t in batch.items()}, tasks)
        torch.cuda.synchronize()
        lib.l4p_prof_enable(0)
        n = lib.l4p_prof_detail(None, 0)
        buf = C.create_string_buffer(int(n) + 16)
        lib.l4p_prof_detail(buf, len(buf))
        tags = buf.value.decode()
        lib.l4p_prof_reset()
        assert (" halo ups " in tags) == bool(v), tags[:2000]
        outs[v] = {k: t.clone() for k, t in o.items() if torch.is_tensor(t)}
    for k in outs[1]:
        assert torch.equal(outs[1][k], outs[0][k]), k
