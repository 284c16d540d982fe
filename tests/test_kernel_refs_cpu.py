"""The float64 references of tests/kernel_refs.py against independent statements, on the CPU (no gpu marker).

tests/test_small_kernels_gpu.py compares the HIP kernels with these references; this file is what makes that comparison
trustworthy: torch's own ops in float64 (F.interpolate, F.conv3d, F.scaled_dot_product_attention, F.layer_norm + F.gelu) on the
shape list the GPU file uses, and the tracker code of oracle/l4p_oracle.py (_pe_encoding, the prompt-token code of
track_single_window, the window state of track_windowed).  Gate for floats: max |a - b| <= 1e-12 max|b| (float64 round-off);
integer / boolean state and byte-level results are equal.
"""
import math
from types import SimpleNamespace
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import l4p_oracle as orc
from tests import kernel_refs as R


def rnd(shape, seed, scale=1.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def close(a, b, rel=1e-12):
    scale = b.abs().max().item() + 1e-300
    err = (a.double() - b.double()).abs().max().item()
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------
# torch's ops in float64
# ------------------------------------------------------------------------------------------------
def _interp(x_cl, size, align):
    return F.interpolate(x_cl.permute(0, 4, 1, 2, 3), size=size, mode="trilinear", align_corners=align).permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("name,B,isz,osz,C,align", R.UPSAMPLE_CASES, ids=[c[0] for c in R.UPSAMPLE_CASES])
def test_trilinear_ref_vs_interpolate_f64(name, B, isz, osz, C, align):
    """ATen indexes double data in double: index_dtype = float64."""
    x = rnd((B, *isz, C), 11)
    close(R.trilinear_ref(x, osz, align, np.float64), _interp(x, osz, align))


@pytest.mark.parametrize("name,B,isz,osz,C,align", R.UPSAMPLE_CASES, ids=[c[0] for c in R.UPSAMPLE_CASES])
def test_trilinear_ref_f32_index_vs_interpolate_f32(name, B, isz, osz, C, align):
    """The float32 index (what ATen and the kernel form for float data) against F.interpolate on float32 data; torch then blends in
    float: 2e-6 of the maximum."""
    x = rnd((B, *isz, C), 12, dtype=torch.float32)
    close(R.trilinear_ref(x, osz, align, np.float32), _interp(x, osz, align), rel=2e-6)


def test_trilinear_ref_identity_is_exact():
    x = rnd((2, 3, 5, 7, 16), 13)
    for align in (True, False):
        assert torch.equal(R.trilinear_ref(x, (3, 5, 7), align, np.float32), x)


@pytest.mark.parametrize("post_exp", [0, 1])
@pytest.mark.parametrize("cout", R.HEAD_OUT_COUT)
@pytest.mark.parametrize("vox", R.HEAD_OUT_VOX)
def test_head_out_ref_vs_conv3d(vox, cout, post_exp):
    for B in R.HEAD_OUT_B:
        x, w, b = rnd((B, vox, 128), 20), rnd((cout, 128), 21, 128 ** -0.5), rnd((cout,), 22)
        y = F.conv3d(x.permute(0, 2, 1).reshape(B, 128, 1, 1, vox), w.reshape(cout, 128, 1, 1, 1), b).reshape(B, cout, vox)
        close(R.head_out_ref(x, w, b, post_exp), torch.exp(y) if post_exp else y)


def _sdpa(q, k, v, heads):
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)
    return F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(q.shape)


@pytest.mark.parametrize("N,P,D,heads", R.ATTN_SHAPES)
def test_attention_refs_vs_sdpa(N, P, D, heads):
    q6, kimg, vimg = rnd((N, 6, D), 30), rnd((N, P, D), 31), rnd((N, P, D), 32)
    qimg, k6, v6 = rnd((N, P, D), 33), rnd((N, 6, D), 34), rnd((N, 6, D), 35)
    ref1 = _sdpa(q6, kimg, vimg, heads)
    close(R.small_attn_ref(1, q6, kimg, vimg, heads), ref1)
    close(R.small_attn_ref(2, qimg, k6, v6, heads), _sdpa(qimg, k6, v6, heads))
    rep = lambda t: t[0:1].expand(N, -1, -1)
    close(R.small_attn_ref(3, q6, kimg[0], vimg[0], heads), _sdpa(q6, rep(kimg), rep(vimg), heads))
    close(R.small_attn_ref(4, qimg[0], k6, v6, heads), _sdpa(rep(qimg), k6, v6, heads))
    # scores passed in: the layout of l4p_t2i_attn_scores (column t * heads + h), padded rows
    hd = D // heads
    s = R.t2i_scores_ref(q6, kimg, heads)
    for t in (0, 5):
        for h in (0, heads - 1):
            direct = (kimg[:, :, h * hd:(h + 1) * hd] * q6[:, t:t + 1, h * hd:(h + 1) * hd]).sum(-1) / math.sqrt(hd)
            close(s[:, :, t * heads + h], direct)
    s_pad = torch.cat([s, torch.full((N, P, 4), 1e30, dtype=torch.float64)], dim=-1)
    close(R.t2i_from_scores_ref(s_pad, vimg, heads), ref1)


@pytest.mark.parametrize("C", R.MASK_PRODUCT_C)
def test_mask_product_ref_vs_bmm(C):
    for vox in R.MASK_PRODUCT_VOX:
        for N in R.MASK_PRODUCT_N:
            up, hyper = rnd((N, vox, C), 40), rnd((N, 3, C), 41)
            close(R.mask_product_ref(up, hyper), torch.bmm(hyper, up.transpose(1, 2)))


@pytest.mark.parametrize("name,NT,lo,hi,wide", R.READOUT_CASES, ids=[c[0] for c in R.READOUT_CASES])
def test_track_readout_ref_vs_interpolate_softmax_f64(name, NT, lo, hi, wide):
    """sparse_heads.py:572-589,645-647 in torch's own float64 ops (ATen indexes double data in double: index_dtype = float64), on random
    logits and on a peaked channel 0 (one source pixel 600 above the rest), where the softmax is near one-hot.  The float32 index the
    kernel tests use comes from the same axis_taps, checked against float32 F.interpolate above."""
    (N, T), (h, w), (H, W) = NT, lo, hi
    N = min(N, 3)  # (many_groups: its geometry, not its 528 groups)
    masks = torch.stack([rnd((N, T, h, w), 60 + c, 3.0) for c in range(3)], dim=1)
    peaked = masks.clone()
    peaked[:, 0] -= 300.0
    peaked[:, 0, :, h // 2, w // 3] = 300.0
    xs, ys = torch.arange(W, dtype=torch.float64) + 0.5, torch.arange(H, dtype=torch.float64) + 0.5
    for m in (masks, peaked):
        up = F.interpolate(m, size=(T, H, W), mode="trilinear", align_corners=False)
        p = torch.softmax(up[:, 0].reshape(N, T, H * W), dim=-1).reshape(N, T, H, W)
        want = torch.stack([(p.sum(2) * xs).sum(-1), (p.sum(3) * ys).sum(-1)], dim=1)
        traj, vis, depth = (torch.from_numpy(a) for a in R.track_readout_ref(m.numpy(), H, W, np.float64))
        assert traj.shape == (N, 2, T) and vis.shape == (N, T) and depth.shape == (N, T)
        close(traj, want)
        close(vis, up[:, 1].mean((-1, -2)))
        close(depth, up[:, 2].mean((-1, -2)).exp())
        # the float32 index moves a weight by a few 1e-8: the estimates move with it, far below the kernel tests' gates
        t32 = torch.from_numpy(R.track_readout_ref(m.numpy(), H, W)[0])
        assert (t32 - want).abs().max().item() <= 1e-4


def test_track_readout_ref_one_hot_identity_is_the_pixel_centre():
    m = np.full((1, 3, 1, 7, 5), -1e3)
    m[0, 0, 0, 4, 1] = 1e3
    traj, vis, depth = R.track_readout_ref(m, 7, 5)
    assert traj[0, 0, 0] == 1.5 and traj[0, 1, 0] == 4.5 and vis[0, 0] == -1e3 and depth[0, 0] == 0.0


@pytest.mark.parametrize("N,T,h,w,cpt", R.MASK_GATHER_CASES[:2] + [(2, 3, 4, 6, 3)])
def test_mask_gather_ref_vs_einsum(N, T, h, w, cpt):
    """The statement of include/l4p_hip.h (row m = ((n T + t) h + y / 2) w + x / 2, tap = (y % 2) * 2 + x % 2) by reshape + einsum.  Integer-valued
    floats: every sum is exact, so the fixed-order float32 sum and the einsum must agree to the bit."""
    g = torch.Generator().manual_seed(70)
    partial = torch.randint(-1000, 1000, (4 * cpt, 3, N * T * h * w), generator=g).float()
    want = torch.einsum("abcintyx->nityaxb", partial.reshape(2, 2, cpt, 3, N, T, h, w)).reshape(N, 3, T, 2 * h, 2 * w)
    got = R.mask_gather_ref(partial.numpy(), N, T, h, w, cpt)
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    # and element by element from the header's index formula
    M = N * T * h * w
    for (n, i, t, y, x) in [(0, 0, 0, 0, 0), (N - 1, 2, T - 1, 2 * h - 1, 2 * w - 1), (N - 1, 1, 0, 1, 2 * w - 2), (0, 2, T - 1, 2 * h - 2, 3)]:
        m_ = ((n * T + t) * h + y // 2) * w + x // 2
        tap = (y % 2) * 2 + x % 2
        s = np.float32(0)
        for c in range(cpt):
            s = s + partial.numpy().reshape(-1)[((tap * cpt + c) * 3 + i) * M + m_]
        assert got[n, i, t, y, x] == s


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,C", R.LN_SHAPES)
def test_layernorm_ex_ref_vs_layer_norm(M, C, act):
    x, g, b = rnd((M, C), 50, 3.0) + 0.5, rnd((C,), 51, 0.2) + 1.0, rnd((C,), 52, 0.1)
    ref = F.layer_norm(x, (C,), g, b, 1e-5)
    if act:
        ref = F.gelu(ref)
    for am in R.LN_ADD_MODS:
        am = M if am == "M" else am
        add = rnd((am, C), 53)
        y, y2 = R.layernorm_ex_ref(x, g, b, 1e-5, add, am, act)
        close(y, ref)
        close(y2, ref + add.repeat((M + am - 1) // am, 1)[:M])
    y, y2 = R.layernorm_ex_ref(x, g, b, 1e-5, None, 0, act)
    close(y, ref)
    assert y2 is None


# ------------------------------------------------------------------------------------------------
# the tracker's prompt tokens against the oracle
# ------------------------------------------------------------------------------------------------
def test_gauss_pe_ref_vs_oracle_pe_encoding():
    G = rnd((3, 176), 60)
    c01 = torch.rand((7, 2, 3), generator=torch.Generator().manual_seed(61), dtype=torch.float64)
    close(R.gauss_pe_ref(G, c01), orc._pe_encoding(G, c01))


class _Captured(Exception):
    pass


def _oracle_tokens(sd, cfg, queries, labels, pfeat, plabel):
    """The [N][6][C] prompt tokens track_single_window hands to its transformer, with every input in float64: the function is run
    up to that call (the transformer is replaced by a capture) with its float32 casts lifted to float64."""
    got = {}

    def capture(sd_, p_, src, pos, tokens, depth, heads):
        got["tokens"] = tokens.clone()
        raise _Captured

    P = cfg.tokens
    with mock.patch.object(orc, "two_way_transformer", capture), \
            mock.patch.object(orc, "dense_pe", lambda G, size: torch.zeros(P, cfg.dim, dtype=torch.float64)), \
            mock.patch.object(torch.Tensor, "float", lambda self: self.double()):
        with pytest.raises(_Captured):
            orc.track_single_window(sd, cfg, torch.zeros(1, P, cfg.dim, dtype=torch.float64), queries, labels, pfeat, plabel)
    assert got["tokens"].dtype == torch.float64
    return got["tokens"]


@pytest.mark.parametrize("N,C", R.TOKENS_CASES)
def test_track_tokens_ref_vs_oracle_prompt_tokens(N, C):
    T, H = 16, 224
    p = "task_heads.track_2d."
    sd = {
        p + "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix": rnd((3, C // 2), 70),
        p + "prompt_encoder.not_a_point_embed.weight": rnd((1, C), 71),
        p + "prompt_encoder.point_embeddings.0.weight": rnd((1, C), 72),
        p + "prompt_encoder.point_embeddings.1.weight": rnd((1, C), 73),
        p + "prompt_encoder.prompt_feature_embeddings.0.weight": rnd((1, C), 74),
        p + "prompt_encoder.prompt_feature_embeddings.1.weight": rnd((1, C), 75),
        p + "mask_decoder.mask_tokens.weight": rnd((3, C), 76),
    }
    cfg = SimpleNamespace(dim=C, frames=T, img=None, grid=(2, 2, 2), tokens=8, sam_depth=2, sam_heads=8)
    # (the oracle takes one image size for H and W; give it H and W separately)
    cfg.img = H
    g = torch.Generator().manual_seed(77)
    queries = torch.rand((N, 3), generator=g, dtype=torch.float64) * torch.tensor([T, H, H], dtype=torch.float64)
    queries[0] = torch.tensor([0.5, H - 0.5, 0.5], dtype=torch.float64)  # borders
    # point labels are what l4p_track_prepare produces: {0, 1, 2}.  (-1 is the label of the PADDED point - token 4, not-a-point - in the
    # oracle; on a real point the oracle would replace the PE by that embedding, the kernel's contract (include/l4p_hip.h: labels
    # {0, 1, 2}) leaves the PE alone for anything but 0 / 1.)  The feature label takes any value: only 0 / 1 select an embedding.
    label_sets = [([2.0], [2.0]), ([0.0], [1.0]), ([1.0], [0.0]), ([2.0], [-1.0])] if N == 1 else \
        [([0.0, 1.0, 2.0, 2.0, 0.0, 1.0, 2.0], [1.0, 0.0, -1.0, 2.0, 0.0, 1.0, -1.0])]
    for labels, plabel in label_sets:
        labels, plabel = torch.tensor(labels, dtype=torch.float64), torch.tensor(plabel, dtype=torch.float64)
        pfeat = rnd((N, C), 78)
        want = _oracle_tokens(sd, cfg, queries, labels, pfeat, plabel)
        k = lambda s: sd[p + s]
        got = R.track_tokens_ref(queries, labels, pfeat, plabel, k("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"),
                                 k("mask_decoder.mask_tokens.weight"), k("prompt_encoder.point_embeddings.0.weight")[0],
                                 k("prompt_encoder.point_embeddings.1.weight")[0], k("prompt_encoder.not_a_point_embed.weight")[0],
                                 k("prompt_encoder.prompt_feature_embeddings.0.weight")[0],
                                 k("prompt_encoder.prompt_feature_embeddings.1.weight")[0], T, H, H)
        close(got, want)
        neither = (plabel != 0) & (plabel != 1)
        assert bool((got[neither][:, 5] == 0).all())  # "neither": the feature row stays zero


# ------------------------------------------------------------------------------------------------
# the window state, keys and history rows against the oracle's recursion
# ------------------------------------------------------------------------------------------------
def _recursion_case(N=70, ws=16, C=16, grid=(4, 2, 2), strides=(0, 8, 16, 24)):
    """Fixed window outputs for a recursion of track_windowed: visibilities on a coarse grid (ties inside the overlap), some tracks'
    x estimate equal to their original query's x (one coordinate equal, the others changed), crafted query times."""
    g = torch.Generator().manual_seed(90)
    P = grid[0] * grid[1] * grid[2]
    T = strides[-1] + ws
    q = torch.rand((N, 3), generator=g) * torch.tensor([float(T - 8), 224.0, 224.0])
    q[0, 0] = 3.5     # exactly on a frame centre: valid_t switches at t + 0.5 == q_t
    q[1, 0] = 100.0   # after every window: never a valid frame, pfeat / plabel must stay
    q[2, 0] = 12.5
    q[3, 0] = 30.5    # the first windows' re-seed would move its time backwards
    q[4, 0] = 0.0
    q[5, 0] = 15.5    # the last frame of window 0
    q[6, 0] = 16.0    # just past it
    outs = []
    for wi in range(len(strides)):
        vis = torch.round(torch.randn((N, 1, ws), generator=g) * 2.0) / 2.0
        vis[7] = 1.0  # all equal: the first frame of the overlap wins
        traj = torch.rand((N, 2, ws), generator=g) * 224.0
        traj[8:20, 0, :] = q[8:20, 1:2]  # x estimate == the original x: after a re-seed one coordinate is equal again
        outs.append({"vis": vis, "traj": traj, "depth": torch.rand((N, 1, ws), generator=g) + 0.5,
                     "prompt_features": torch.randn((N, C), generator=g), "history": torch.randn((N, P, C), generator=g)})
    feats = [torch.randn((1, P, C), generator=g) for _ in strides]
    mask_tok = torch.randn((1, C), generator=g)
    return SimpleNamespace(N=N, ws=ws, C=C, grid=grid, P=P, T=T, strides=list(strides), q=q, outs=outs, feats=feats, mask_tok=mask_tok)


def _run_oracle_recursion(case):
    calls, trace = [], []

    def window(sd, cfg, enc_feat, queries_n3, labels_n, pfeat, plab, task="track_2d"):
        calls.append({"keys_in": enc_feat.clone(), "q_off": queries_n3.clone(), "labels": labels_n.clone(), "pfeat": pfeat.clone(),
                      "plabel": plab.clone()})
        return case.outs[len(calls) - 1]

    cfg = SimpleNamespace(dim=case.C, frames=case.ws, grid=case.grid, tokens=case.P)
    sd = {"task_heads.track_2d.processed_video_mask_token.weight": case.mask_tok}
    with mock.patch.object(orc, "track_single_window", window):
        out = orc.track_windowed(sd, cfg, case.feats, case.q[None].clone(), torch.zeros(1, case.N), case.strides, trace=trace)
    return out, calls, trace


def test_track_prepare_and_commit_refs_vs_oracle_recursion():
    """track_prepare_ref / track_commit_ref drive the same recursion as the oracle's track_windowed (its window network replaced by
    fixed outputs): every traced integer / boolean state, the carried prompt state and the stitched buffers are EQUAL."""
    case = _recursion_case()
    out, calls, trace = _run_oracle_recursion(case)
    N, ws, T = case.N, case.ws, case.T
    traj, vis, dep = np.zeros((N, 2, T), np.float32), np.full((N, T), -10.0, np.float32), np.zeros((N, T), np.float32)
    cur_q, orig_q = case.q.numpy().copy(), case.q.numpy().copy()
    plabel, pfeat = np.zeros(N, np.float32), np.zeros((N, case.C), np.float32)
    seen = {"l1": 0, "l2": 0, "tie": 0, "back": 0, "stay": 0}
    for wi, start in enumerate(case.strides):
        last = wi == len(case.strides) - 1
        nxt = 0 if last else case.strides[wi + 1]
        q_off, labels, valid_t, valid_n = R.track_prepare_ref(cur_q, orig_q, start, ws)
        assert np.array_equal(labels, trace[wi]["labels"].numpy())
        assert np.array_equal(valid_t.astype(bool), trace[wi]["valid_t"].numpy())
        assert np.array_equal(q_off, trace[wi]["queries"].numpy())
        assert np.array_equal(plabel, trace[wi]["prompt_labels"].numpy())
        assert np.array_equal(pfeat, calls[wi]["pfeat"].numpy())
        for v in (1, 2):  # (0 - never valid, no coordinate equal - cannot arise inside a recursion: test_track_prepare_ref_edges)
            seen[f"l{v}"] += int((labels == v).sum())
        o = case.outs[wi]
        r = R.track_commit_ref(o["traj"].numpy(), o["vis"][:, 0].numpy(), o["depth"][:, 0].numpy(), valid_t, valid_n, traj, vis, dep,
                               start, ws, nxt, int(last), cur_q, plabel, o["prompt_features"].numpy(), pfeat)
        if not last:
            assert np.array_equal(r["best"], trace[wi]["best_vis_id"].numpy())
            reseeded = (r["cur_q"] != cur_q).any(axis=1)
            assert np.array_equal(reseeded, trace[wi]["reseeded"].numpy() & reseeded)  # (a re-seed onto equal values is no change)
            ov = r["vis"][:, nxt:start + ws]
            seen["tie"] += int(((ov == ov.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            seen["back"] += int((~trace[wi]["reseeded"].numpy()).sum())
            seen["stay"] += int((valid_n == 0).sum())
        traj, vis, dep, cur_q, plabel, pfeat = r["traj"], r["vis"], r["depth"], r["cur_q"], r["plabel"], r["pfeat"]
    assert np.array_equal(traj, out["track_2d_traj_est_bn2t"][0].numpy())
    assert np.array_equal(vis, out["track_2d_vis_est_bn1t"][0, :, 0].numpy())
    assert np.array_equal(dep, out["track_2d_depth_est_bn1t"][0, :, 0].numpy())
    assert all(v > 0 for v in seen.values()), seen  # every crafted situation occurred


def test_track_prepare_ref_edges():
    cur = np.array([[3.5, 1, 2], [3.5000002, 1, 2], [40.0, 5, 6], [2.0, 7, 8], [2.0, 9, 9], [40.0, 1, 1]], np.float32)
    orig = np.array([[3.5, 0, 0], [0.0, 0, 0], [40.0, 5, 6], [1.0, 0, 8], [1.0, 0, 0], [41.0, 2, 2]], np.float32)
    q_off, labels, valid_t, valid_n = R.track_prepare_ref(cur, orig, 0, 8)
    assert valid_t[0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1]  # 3 + 0.5 - 3.5 == 0 is valid
    assert valid_t[1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]  # one float32 step later it is not
    assert valid_n.tolist() == [1, 1, 0, 1, 1, 0]
    assert labels.tolist() == [1.0, 2.0, 1.0, 1.0, 2.0, 0.0]  # equal time; none equal; invalid but equal -> 1; y equal only; none; invalid, none
    q_off2, _, _, _ = R.track_prepare_ref(cur, orig, 8, 8)
    assert q_off2[:, 0].tolist() == [-4.5, np.float32(3.5000002) - np.float32(8), 32.0, -6.0, -6.0, 32.0] and np.array_equal(q_off2[:, 1:], cur[:, 1:])


def test_keys_init_and_fill_rows_refs_vs_oracle_recursion():
    """The keys the oracle's recursion hands to its window network (encoder feature + history, in float64) against keys_init_ref
    on a history built with fill_rows_ref's row map (second half of every track = the mask token); with shared_from = P / 2 the rows
    keys_init_ref leaves unwritten are the ones that equal track 0's in the oracle, and the shared set holds them."""
    case = _recursion_case(N=24)
    for d in case.outs:
        d["history"] = d["history"].double()
    case.feats = [f.double() for f in case.feats]
    case.mask_tok = case.mask_tok.double()
    _, calls, _ = _run_oracle_recursion(case)
    N, P, C, half = case.N, case.P, case.C, case.P // 2
    G = rnd((3, C // 2), 95)
    pos = orc.dense_pe(G.float(), case.grid).double()
    tok_u8 = case.mask_tok[0].numpy().view(np.uint8)
    for wi in range(len(case.strides)):
        hist = np.zeros((N, P, C), np.float64)
        if wi == 0:
            hist_u8 = R.fill_rows_ref(hist.reshape(-1).view(np.uint8), tok_u8, N * P, C * 8, P, P, 0)
        else:
            hist[:, :half] = case.outs[wi - 1]["history"][:, half:].numpy()
            hist_u8 = R.fill_rows_ref(hist.reshape(-1).view(np.uint8), tok_u8, N * half, C * 8, half, P, half)
        hist = torch.from_numpy(hist_u8.view(np.float64).reshape(N, P, C).copy())
        want = calls[wi]["keys_in"]
        k, kp, written, shared = R.keys_init_ref(case.feats[wi][0], hist, pos, 0, round_f32=False)
        assert bool(written.all()) and shared is None
        close(k, want)
        close(kp, want + pos[None])
        k2, kp2, written2, shared2 = R.keys_init_ref(case.feats[wi][0], hist, pos, half, round_f32=False)
        assert written2.sum().item() == N * half + half and bool(written2[0].all()) and not bool(written2[1:, half:].any())
        close(k2[written2], want[written2])
        close(kp2[written2], (want + pos[None])[written2])
        close(shared2, want[0, half:])
        assert torch.equal(want[:, half:], want[0:1, half:].expand(N, -1, -1))  # what makes the sharing valid


def test_keys_init_ref_float_storage():
    enc, hist, pos = rnd((8, 16), 96, dtype=torch.float32), rnd((3, 8, 16), 97, dtype=torch.float32), rnd((8, 16), 98, dtype=torch.float32)
    k, kp, _, _ = R.keys_init_ref(enc, hist, pos, 0)
    assert torch.equal(k.float(), enc[None] + hist) and torch.equal(k.float().double(), k)
    assert torch.equal(kp.float(), (enc[None] + hist) + pos[None])


# ------------------------------------------------------------------------------------------------
# byte-level fills, casts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("nbytes", [16, 16 * 1000])
def test_fill_rows_and_broadcast_block_refs_vs_slicing(n, nbytes):
    rs = np.random.RandomState(3)
    gr, gs, go = 3, 7, 2
    buf = rs.randint(0, 256, size=(n * gs + 1) * nbytes).astype(np.uint8)
    v = rs.randint(0, 256, size=nbytes).astype(np.uint8)
    want = buf.copy().reshape(n * gs + 1, nbytes)
    for g in range(n):
        want[g * gs + go:g * gs + go + gr] = v
    assert np.array_equal(R.fill_rows_ref(buf, v, n * gr, nbytes, gr, gs, go), want.reshape(-1))
    off, stride = 48, nbytes + 96
    buf = rs.randint(0, 256, size=n * stride + 32).astype(np.uint8)
    want = buf.copy()
    groups = want[:n * stride].reshape(n, stride)
    groups[1:, off:off + nbytes] = groups[0, off:off + nbytes]
    assert np.array_equal(R.broadcast_block_ref(buf, off, nbytes, stride, n), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_cast_ref_vs_torch_conversion(dtype):
    x = torch.cat([R.cast_specials(), rnd((4000,), 99, 30.0, torch.float32), rnd((4000,), 100, 1e-6, torch.float32)])
    got, want = R.cast_ref(x, dtype), x.to(dtype)
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(bits(got), bits(want))


def test_ulp_of():
    r = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, 3e-6, -100.0], dtype=torch.float64)
    assert R.ulp_of(r, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -26, 2.0 ** -1]
    assert R.ulp_of(r, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -4]
