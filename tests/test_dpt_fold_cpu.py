"""CPU: the pack-time fold of the DPT up-scaling ConvTranspose3d into the 3x3x3 conv behind it (packing.fold_convT_rn) against
F.conv3d(F.conv_transpose3d(x, W_ct, b_ct, stride=k), W_rn, padding=1) in float64 - the sub-pixel conv that
l4p_conv3d_subpixel computes, stated with torch ops: per sub-position only the ACTIVE cells, in the packed row order, plus the
border-class bias row."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from l4p_amd import packing

L, FOUT = 8, 6
CASES = [  # k, grid, B, active (sub-position, cell) blocks, distinct bias classes
    ((2, 4, 4), (2, 3, 5), 2, 144, 27),
    ((2, 2, 2), (1, 3, 2), 2, 64, 18),
    ((2, 1, 1), (2, 3, 3), 1, 36, 27),
    ((2, 4, 4), (1, 1, 1), 1, 144, 18),
]


def subpixel_reference(x, w, bias, k, fout):
    """What the kernel computes from the packed operands: x [B, L, t, h, w] float64 -> [B, fout, t*kt, h*kh, w*kw]; every
    (sub-position, active cell) block once, cells ascending, out-of-grid cells zero, bias row by border class."""
    B, l, gt, gh, gw = x.shape
    T, H, W = gt * k[0], gh * k[1], gw * k[2]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    out = torch.zeros(B, fout, T, H, W, dtype=x.dtype)
    classes = set()
    for st, sh, sw in itertools.product(range(k[0]), range(k[1]), range(k[2])):
        s = (st * k[1] + sh) * k[2] + sw
        acc = torch.zeros(B, fout, gt, gh, gw, dtype=x.dtype)
        j = 0
        for ct in packing.fold_axis_cells(k[0], st):
            for ch in packing.fold_axis_cells(k[1], sh):
                for cw in packing.fold_axis_cells(k[2], sw):
                    blk = w[s * fout:(s + 1) * fout, j * l:(j + 1) * l]
                    acc += torch.einsum("fl,blthw->bfthw", blk, xp[:, :, 1 + ct:1 + ct + gt, 1 + ch:1 + ch + gh, 1 + cw:1 + cw + gw])
                    j += 1
        assert float(w[s * fout:(s + 1) * fout, j * l:].abs().max() if j * l < w.shape[1] else 0.0) == 0.0  # zero behind the cells
        for it, ih, iw in itertools.product(range(gt), range(gh), range(gw)):
            p = (it * k[0] + st, ih * k[1] + sh, iw * k[2] + sw)
            c = tuple(packing.fold_bias_class(p[a], (T, H, W)[a]) for a in range(3))
            classes.add(c)
            out[:, :, p[0], p[1], p[2]] = acc[:, :, it, ih, iw] + bias[(c[0] * 3 + c[1]) * 3 + c[2]]
    return out, len(classes)


@pytest.mark.parametrize("k,grid,B,blocks,nclasses", CASES)
def test_fold_equals_conv_of_conv_transpose(k, grid, B, blocks, nclasses):
    g = torch.Generator().manual_seed(7)
    w_ct = torch.randn(L, L, *k, generator=g, dtype=torch.float64)
    b_ct = torch.randn(L, generator=g, dtype=torch.float64)
    w_rn = torch.randn(FOUT, L, 3, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(B, L, *grid, generator=g, dtype=torch.float64)
    ref = F.conv3d(F.conv_transpose3d(x, w_ct, b_ct, stride=k), w_rn, padding=1)
    w, bias, nblk = packing.fold_convT_rn(w_ct, b_ct, w_rn)
    assert nblk == blocks
    assert w.dtype == torch.float64 and tuple(w.shape) == (k[0] * k[1] * k[2] * FOUT, packing.fold_max_cells(k) * L)
    assert tuple(bias.shape) == (27, FOUT)
    got, ncls = subpixel_reference(x, w, bias, k, FOUT)
    assert ncls == nclasses
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"k={k} grid={grid}: relative max error {err:.3g}, {nblk} blocks, {ncls} bias classes")
    assert err <= 1e-12


def test_axis_cells_and_bias_classes():
    assert packing.fold_axis_cells(1, 0) == [-1, 0, 1]
    assert packing.fold_axis_cells(2, 0) == [-1, 0] and packing.fold_axis_cells(2, 1) == [0, 1]
    assert [packing.fold_axis_cells(4, s) for s in range(4)] == [[-1, 0], [0], [0], [0, 1]]
    assert [packing.fold_bias_class(p, 4) for p in range(4)] == [0, 1, 1, 2]
    assert [packing.fold_bias_class(p, 2) for p in range(2)] == [0, 2]
    with pytest.raises(ValueError):
        packing.fold_bias_class(0, 1)


def test_pack_dpt_adds_fold_entries_next_to_the_unfolded_ones():
    from l4p_amd.weights import ModelCfg, actpost_of, seeded_state_dict

    cfg = ModelCfg.mini()
    sd = seeded_state_dict(cfg, tasks=["depth", "camray"])
    pw = packing.pack_state_dict(sd, cfg, torch.float32, torch.device("cpu"), tasks=["depth", "camray"])
    for task in ("depth", "camray"):
        for i, sf in enumerate(actpost_of(task)):
            up = any(s > 0 for s in sf)
            assert (f"dpt.{task}.fold{i}.w" in pw) == up and (f"dpt.{task}.fold{i}.b" in pw) == up
            assert f"dpt.{task}.rn{i}.w" in pw
            if up:
                k = tuple(2 ** s for s in sf)
                Li = cfg.layer_dims[i]
                assert f"dpt.{task}.act{i}.1.w" in pw
                assert tuple(pw[f"dpt.{task}.fold{i}.w"].shape) == (k[0] * k[1] * k[2] * cfg.feature_dim, packing.fold_max_cells(k) * Li)
                assert tuple(pw[f"dpt.{task}.fold{i}.b"].shape) == (27, cfg.feature_dim)
