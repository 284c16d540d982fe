"""Plain float64 restatements of the small tracker / DPT kernels of the C ABI (include/l4p_hip.h), and the shape lists their tests share.

Every function is written from the operation's definition (the index formulas of the header comments) with torch / numpy on the
CPU in float64.  None of them calls the torch op it is later compared with: tests/test_kernel_refs_cpu.py checks each one against
an independent statement (F.interpolate, F.conv3d, F.scaled_dot_product_attention, F.layer_norm, the functions of
oracle/l4p_oracle.py) on a machine without a GPU, tests/test_small_kernels_gpu.py then checks the HIP kernels against them.
A reference that were wrong the same way as a kernel fails the first file.
"""
import math

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------
# shape lists (one place: the CPU checks of the references and the GPU checks of the kernels walk the same cases)
# ------------------------------------------------------------------------------------------------
# name, B, (Ti, Hi, Wi), (To, Ho, Wo), C, align_corners - each reaches one branch of launch_upsample / upsample_kernel
UPSAMPLE_CASES = [
    ("a_dpt_head_x2", 1, (4, 28, 28), (4, 56, 56), 128, True),       # T kept: lt == 0 on every line (NT = 1), the DPT head form
    ("b_fractional", 1, (4, 60, 72), (4, 112, 128), 128, True),      # fractional non-square factors (the scale divided once on the host,
                                                                     # multiplied per thread in float), cv_shift path (C / 8 = 16)
    ("c_odd_div", 2, (3, 5, 7), (5, 9, 16), 24, False),              # C / 8 = 3: the division path (cv_shift = -1); odd sizes; border
                                                                     # clamp (negative source coordinate); all four NT / NH forms
    ("d_down", 1, (8, 16, 16), (4, 8, 8), 8, False),                 # down-sampling by an integer factor
    ("e_readout", 1, (2, 56, 56), (2, 224, 224), 8, False),          # the tracker read-out's form, align_corners = False
    ("f_lines_z1", 2, (80, 112, 1), (160, 224, 2), 8, False),        # 71 680 lines > 65 535: blockIdx.z = 1 lines
    ("g_long_line", 1, (1, 1, 15000), (1, 2, 40000), 8, False),      # Wo * C / 8 = 40 000 > 64 * 512: gx capped, threads stride
    ("c352_div", 1, (2, 6, 5), (3, 12, 11), 352, True),              # C / 8 = 44: the division path at the DPT fusion width
]

# (N, P, D, heads) of l4p_small_attn kinds 1 - 4 and l4p_t2i_attn_scores (hd = D / heads <= 96).  The comments say what each shape is
# for; that it reaches the kernel form named (i2t LDS / direct), with which grid and LDS size, is asserted by tests/test_track_select_cpu.py
ATTN_SHAPES = [
    (3, 2048, 704, 8),   # the full model's shape: hd 88, whole-row score form (16-bit), i2t LDS kernel with 32 rows
    (2, 96, 352, 4),     # P < 256 (tid < P on the first row load); P < 1024: grown LDS of the P.V reduction; i2t rows = 64, ragged
    (5, 1000, 256, 8),   # hd 32, P below 1024 and P % 256 != 0; i2t: (P + 31) / 32 leaves a ragged last workgroup
    (2, 36, 288, 3),     # hd 96; heads do not divide 256: the direct i2t kernel
    (1, 1028, 96, 6),    # hd 16, just past 1024 (no LDS growth); direct i2t kernel (256 % 6 != 0)
    (2, 512, 352, 8),    # hd 44, hd % 8 != 0: 16-bit engines take the generic score loop: two 16-groups + three tails of four
    (2, 260, 96, 8),     # hd 12: tail only
]

# (C = 1540 is the first width that takes the row kernel's seventh float4 slot per lane, 2048 its limit: the 8-slot instantiations)
LN_SHAPES = [(37, 352), (2048, 1408), (6, 176), (5, 1540), (6, 2048)]
LN_ADD_MODS = ["M", 6, 5]  # "M": one addend row per row; 5 does not divide 37 or 2048

HEAD_OUT_VOX = [256 * 3, 1000, 255, 1]
HEAD_OUT_B = [1, 3]
HEAD_OUT_COUT = [1, 3, 6, 8]

MASK_PRODUCT_C = [176, 40, 352]
MASK_PRODUCT_VOX = [128 * 5, 1000, 7]
MASK_PRODUCT_N = [1, 3]

TOKENS_CASES = [(1, 352), (7, 352), (1, 1408), (7, 1408)]  # (N, C)

CAST_SIZES = [4, 8, 4 * 1000, 4 * (2048 * 256 + 3)]


def _f64(x):
    return x.detach().cpu().to(torch.float64)


# ------------------------------------------------------------------------------------------------
# trilinear resize, channels-last
# ------------------------------------------------------------------------------------------------
def axis_taps(in_size, out_size, align_corners, index_dtype=np.float32):
    """Source indices i0, i1 and the weight of i1 for one axis: the half-pixel formula with the clamp (align_corners False) or the
    corner-aligned one, formed in ``index_dtype`` without fused operations; the weight is returned as float64."""
    f = np.dtype(index_dtype).type
    dst = np.arange(out_size).astype(index_dtype)
    if align_corners:
        scale = f(in_size - 1) / f(out_size - 1) if out_size > 1 else f(0)
        src = scale * dst
    else:
        scale = f(in_size) / f(out_size)
        src = scale * (dst + f(0.5)) - f(0.5)
        src = np.where(src < 0, f(0), src)
    assert src.dtype == np.dtype(index_dtype)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    lam = np.clip(src - i0.astype(index_dtype), f(0), f(1))
    i1 = i0 + (i0 < in_size - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam.astype(np.float64))


def trilinear_ref(x_cl, size, align_corners, index_dtype=np.float32):
    """x_cl [B][Ti][Hi][Wi][C] -> float64 [B][To][Ho][Wo][C]; separable: the blend of the eight taps in float64."""
    y = _f64(x_cl)
    for axis, out_size in zip((1, 2, 3), size):
        i0, i1, lam = axis_taps(y.shape[axis], out_size, align_corners, index_dtype)
        shape = [1] * 5
        shape[axis] = out_size
        lam = lam.reshape(shape)
        y = y.index_select(axis, i0) * (1.0 - lam) + y.index_select(axis, i1) * lam
    return y


# ------------------------------------------------------------------------------------------------
# DPT head output projection
# ------------------------------------------------------------------------------------------------
def head_out_ref(x_cl, w, b, post_exp):
    """x_cl [B][vox][C] (any leading voxel dims flattened by the caller), w [Cout][C], b [Cout] -> float64 [B][Cout][vox]."""
    x, w, b = _f64(x_cl), _f64(w), _f64(b)
    B, C = x.shape[0], x.shape[-1]
    x = x.reshape(B, -1, C)
    y = torch.stack([(x * w[o]).sum(-1) + b[o] for o in range(w.shape[0])], dim=1)
    return torch.exp(y) if post_exp else y


# ------------------------------------------------------------------------------------------------
# tracker attention: 6 prompt tokens <-> P image tokens
# ------------------------------------------------------------------------------------------------
def _softmax_last(s):
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def small_attn_ref(kind, q, k, v, heads):
    """kind 1: q [N][6][D], k, v [N][P][D] -> [N][6][D]; kind 2: q [N][P][D], k, v [N][6][D] -> [N][P][D];
    kind 3 / 4: the image-side operand (k, v resp. q) is one [P][D] set shared by every track."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    if kind == 3:
        k, v = k.unsqueeze(0).expand(q.shape[0], -1, -1), v.unsqueeze(0).expand(q.shape[0], -1, -1)
    if kind == 4:
        q = q.unsqueeze(0).expand(k.shape[0], -1, -1)
    N, Lq, D = q.shape
    hd = D // heads
    qh, kh, vh = (t.reshape(N, t.shape[1], heads, hd) for t in (q, k, v))
    s = torch.einsum("nihd,njhd->nhij", qh, kh) / math.sqrt(hd)
    return torch.einsum("nhij,njhd->nihd", _softmax_last(s), vh).reshape(N, Lq, D)


def t2i_scores_ref(q, k, heads):
    """The scaled scores of kind 1 in l4p_t2i_attn_scores' layout: float64 [N][P][6 * heads], column t * heads + h."""
    q, k = _f64(q), _f64(k)
    N, _, D = q.shape
    hd = D // heads
    s = torch.einsum("nihd,njhd->njih", q.reshape(N, 6, heads, hd), k.reshape(N, -1, heads, hd)) / math.sqrt(hd)
    return s.reshape(N, k.shape[1], 6 * heads)


def t2i_from_scores_ref(scores, v, heads):
    """scores [N][P][ld] (column t * heads + h, ld >= 6 * heads), v [N][P][D] -> softmax over p, then P.V: float64 [N][6][D]."""
    s, v = _f64(scores), _f64(v)
    N, P, D = v.shape
    hd = D // heads
    s = s[:, :, :6 * heads].reshape(N, P, 6, heads).permute(0, 3, 2, 1)  # n h t p
    out = torch.einsum("nhtp,nphd->nthd", _softmax_last(s), v.reshape(N, P, heads, hd))
    return out.reshape(N, 6, D)


def mask_product_ref(up, hyper):
    """up [N][vox][C], hyper [N][3][C] -> float64 [N][3][vox]."""
    up, hyper = _f64(up), _f64(hyper)
    return torch.stack([(up * hyper[:, m:m + 1, :]).sum(-1) for m in range(3)], dim=1)


# ------------------------------------------------------------------------------------------------
# tracker output tail: gather of the mask up-scaling's partial sums, read-out of the mask logits
# ------------------------------------------------------------------------------------------------
# id, (N, T), (h, w), (H, W), wide: whether launch_track_readout takes the 1024-thread form with the knob readout_wide on
# (W <= 256, N T <= 512 and its LDS request (3 h w + w + h + 2 (W + H) + 32 W) * 4 <= 160 KiB).  The flag restates the rule by hand:
# tests/test_track_select_cpu.py holds it to the selection itself (csrc/track_select.hpp track_readout_select), with both LDS sizes
READOUT_CASES = [
    ("int4_nonsquare", (3, 2), (8, 12), (32, 48), True),     # integer scale, h != w, W < 64: lanes tid >= W inside the one summed wave
    ("frac_small", (2, 3), (6, 10), (20, 36), True),         # non-integer scales, H < 32: one partial row block
    ("row_tail", (2, 1), (10, 6), (72, 40), True),           # row blocks 32 + 32 + 8, T = 1
    ("identity", (1, 2), (7, 5), (7, 5), True),              # lam == 0 everywhere
    ("wide_W", (1, 2), (8, 72), (16, 288), False),           # W > 256: column form, a second x stride
    ("many_groups", (33, 16), (6, 10), (20, 36), False),     # N T = 528 > 512
    ("lds_over", (1, 2), (112, 112), (16, 128), False),      # wide LDS 168 960 B > 160 KiB (column form: 151 424 B); down-sampling in y
    ("model", (2, 2), (56, 56), (224, 224), True),           # the workload's geometry
]

# (N, T, h, w, chunks per tap); N T 4 h w voxels per channel: 360, 120, 368 640 (1440 blocks of 256) and 4 262 400 - past the
# 16 384 * 256 = 4 194 304 the capped grid covers in one trip of its grid-stride loop
MASK_GATHER_CASES = [(3, 2, 3, 5, 2), (2, 1, 5, 3, 1), (5, 4, 64, 72, 1), (4, 3, 296, 300, 1)]


def mask_gather_ref(partial, N, T, h, w, cpt):
    """partial [4 * cpt][3][M] with M = N T h w (chunk c of tap (dy, dx) is slice (dy * 2 + dx) * cpt + c; row m = ((n T + t) h + y) w + x)
    -> float32 numpy [N][3][T][2 h][2 w]: out[n][i][t][2 y + dy][2 x + dx] = the float32 sum over the tap's chunks in index order."""
    p = np.asarray(partial, dtype=np.float32).reshape(2, 2, cpt, 3, N, T, h, w)
    out = np.zeros((N, 3, T, 2 * h, 2 * w), dtype=np.float32)
    for dy in range(2):
        for dx in range(2):
            acc = np.zeros((3, N, T, h, w), dtype=np.float32)
            for c in range(cpt):
                acc = acc + p[dy, dx, c]  # float32 + float32, one rounding per chunk, as the kernel's a += pp[..]
            out[:, :, :, dy::2, dx::2] = acc.transpose(1, 0, 2, 3, 4)
    return out


def track_readout_ref(masks, H, W, index_dtype=np.float32):
    """masks [N][3][T][h][w] -> float64 numpy (traj [N][2][T] = (x, y), vis [N][T], depth [N][T]): bilinear resize (align_corners False;
    the source index formed in ``index_dtype`` by axis_taps: float32 is what ATen and the kernel form for float data, float64 what ATen
    forms for double data) to H x W; channel 0: softmax over the H W samples with their TRUE maximum as the shift, expectation of the
    pixel centres (+0.5); channel 1: spatial mean; channel 2: exp(spatial mean)."""
    m = np.asarray(masks, dtype=np.float64)
    h, w = m.shape[-2:]
    y0, y1, ly = (a.numpy() for a in axis_taps(h, H, False, index_dtype))
    x0, x1, lx = (a.numpy() for a in axis_taps(w, W, False, index_dtype))
    rows = m[..., y0, :] * (1.0 - ly)[:, None] + m[..., y1, :] * ly[:, None]
    up = rows[..., x0] * (1.0 - lx) + rows[..., x1] * lx  # [N][3][T][H][W]
    z = up[:, 0]
    e = np.exp(z - z.max(axis=(-1, -2), keepdims=True))
    p = e / e.sum(axis=(-1, -2), keepdims=True)
    tx = (p.sum(axis=-2) * (np.arange(W) + 0.5)).sum(-1)
    ty = (p.sum(axis=-1) * (np.arange(H) + 0.5)).sum(-1)
    return np.stack([tx, ty], axis=1), up[:, 1].mean(axis=(-1, -2)), np.exp(up[:, 2].mean(axis=(-1, -2)))


# ------------------------------------------------------------------------------------------------
# LayerNorm with the tracker's extras
# ------------------------------------------------------------------------------------------------
def layernorm_ex_ref(x, g, b, eps, add=None, add_mod=0, act=0):
    """y = LN(x) (biased variance), then erf-GELU when act == 1 (L4P_ACT_GELU); returns (y, y + add[row % add_mod]) in float64."""
    x, g, b = _f64(x), _f64(g), _f64(b)
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / x.shape[-1]
    y = d / torch.sqrt(var + eps) * g + b
    if act == 1:
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    y2 = None
    if add is not None:
        rows = torch.arange(x.shape[0]) % add_mod
        y2 = y + _f64(add)[rows]
    return y, y2


# ------------------------------------------------------------------------------------------------
# prompt tokens, key initialisation
# ------------------------------------------------------------------------------------------------
def gauss_pe_ref(gauss, coords01):
    """Gaussian positional formula: coords01 [..., 3] in [0, 1] -> [sin(2 pi c G) | cos(2 pi c G)], G [3][C / 2], c = 2 coords - 1."""
    G, c = _f64(gauss), 2.0 * _f64(coords01) - 1.0
    a = c[..., 0:1] * G[0] + c[..., 1:2] * G[1] + c[..., 2:3] * G[2]
    a = 2.0 * math.pi * a
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


def track_tokens_ref(queries, labels, pfeat, plabel, gauss, mask_tokens, point_emb0, point_emb1, not_a_point, feat_emb0, feat_emb1,
                     T, H, W):
    """tokens float64 [N][6][C] = 3 mask tokens | point PE + label embedding | not-a-point | feature prompt.
    queries [N][3] = (t, x, y) normalised by (T, W, H); the label embedding is added for label 0 / 1 only; the feature row is
    pfeat + feature embedding for plabel 0 / 1 and zero otherwise."""
    q, lab, pl = _f64(queries), _f64(labels), _f64(plabel)
    N, C = q.shape[0], mask_tokens.shape[-1]
    tok = torch.zeros(N, 6, C, dtype=torch.float64)
    tok[:, 0:3] = _f64(mask_tokens)
    c01 = torch.stack([q[:, 0] / T, q[:, 1] / W, q[:, 2] / H], dim=-1)
    pe = gauss_pe_ref(gauss, c01)
    pe = pe + (lab == 0)[:, None] * _f64(point_emb0) + (lab == 1)[:, None] * _f64(point_emb1)
    tok[:, 3] = pe
    tok[:, 4] = _f64(not_a_point)
    pf = _f64(pfeat)
    tok[:, 5] = (pl == 0)[:, None] * (pf + _f64(feat_emb0)) + (pl == 1)[:, None] * (pf + _f64(feat_emb1))
    return tok


def keys_init_ref(enc, hist, pos, shared_from, round_f32=True):
    """keys = enc [P][C] (broadcast over tracks) + hist [N][P][C]; kp = keys + pos [P][C].  round_f32: the keys are STORED as float
    (k32) and kp is formed from the stored value, as the kernel does; False: no intermediate rounding.
    Returns (k, kp, written [N][P] bool, shared [P - shared_from][C] or None): with shared_from > 0 rows >= shared_from are written for
    track 0 only, whose float rows are also the shared set."""
    k = _f64(enc)[None] + _f64(hist)
    if round_f32:
        k = k.float().double()
    kp = k + _f64(pos)[None]
    N, P = k.shape[0], k.shape[1]
    written = torch.ones(N, P, dtype=torch.bool)
    shared = None
    if shared_from > 0:
        written[1:, shared_from:] = False
        shared = k[0, shared_from:].clone()
    return k, kp, written, shared


# ------------------------------------------------------------------------------------------------
# byte-level fills
# ------------------------------------------------------------------------------------------------
def fill_rows_ref(out_u8, v_u8, rows, row_bytes, group_rows, group_stride, group_off):
    """Logical row r of the fill lives at physical row (r / group_rows) * group_stride + group_off + r % group_rows (numpy uint8)."""
    out = out_u8.copy()
    for r in range(rows):
        row = (r // group_rows) * group_stride + group_off + (r % group_rows)
        out[row * row_bytes:(row + 1) * row_bytes] = v_u8[:row_bytes]
    return out


def broadcast_block_ref(buf_u8, off, nbytes, stride, n):
    """The nbytes bytes at off are copied to the same offset of the following n - 1 groups (group g starts at g * stride)."""
    out = buf_u8.copy()
    for g in range(1, n):
        out[g * stride + off:g * stride + off + nbytes] = buf_u8[off:off + nbytes]
    return out


# ------------------------------------------------------------------------------------------------
# sliding-window state (float comparisons in float32: equality and >= edges match bit for bit)
# ------------------------------------------------------------------------------------------------
def track_prepare_ref(cur_q, orig_q, start, ws):
    """cur_q, orig_q float32 [N][3] (t, x, y) -> q_off float32 [N][3], labels float32 [N], valid_t uint8 [N][ws], valid_n uint8 [N]."""
    cur, orig = np.asarray(cur_q, dtype=np.float32), np.asarray(orig_q, dtype=np.float32)
    tj = (np.arange(ws) + start).astype(np.float32) + np.float32(0.5)
    valid_t = (tj[None, :] - cur[:, 0:1]) >= np.float32(0)
    valid_n = valid_t.any(axis=1)
    q_off = cur.copy()
    q_off[:, 0] = cur[:, 0] - np.float32(start)
    same = (cur == orig).any(axis=1)  # ANY coordinate equal to the original query's
    labels = np.where(valid_n, np.float32(1), np.float32(0))
    labels = np.where(same, np.float32(1), labels)
    labels = np.where(valid_n & ~same, np.float32(2), labels).astype(np.float32)
    return q_off, labels, valid_t.astype(np.uint8), valid_n.astype(np.uint8)


def track_commit_ref(w_traj, w_vis, w_depth, valid_t, valid_n, traj, vis, depth, start, ws, next_start, last_window, cur_q, plabel,
                     new_pfeat, pfeat):
    """Masked scatter of a window's estimates [N][2][ws] / [N][ws] into the clip buffers [N][2][T] / [N][T]; unless last_window:
    plabel = 1 and pfeat = new_pfeat on valid tracks, best = FIRST maximum of the stitched visibility over [next_start, start + ws),
    and the query is re-seeded at that frame only when that moves its time forward.  Returns new copies (float32 numpy) + best."""
    traj, vis, depth = (np.array(a, dtype=np.float32, copy=True) for a in (traj, vis, depth))
    cur_q, plabel, pfeat = (np.array(a, dtype=np.float32, copy=True) for a in (cur_q, plabel, pfeat))
    vt, vn = np.asarray(valid_t).astype(bool), np.asarray(valid_n).astype(bool)
    sl = slice(start, start + ws)
    vis[:, sl] = np.where(vt, w_vis, vis[:, sl])
    depth[:, sl] = np.where(vt, w_depth, depth[:, sl])
    traj[:, :, sl] = np.where(vt[:, None, :], w_traj, traj[:, :, sl])
    best = None
    if not last_window:
        plabel[vn] = np.float32(1)
        pfeat[vn] = np.asarray(new_pfeat, dtype=np.float32)[vn]
        ov = vis[:, next_start:start + ws]
        N = ov.shape[0]
        best = np.zeros(N, dtype=np.int32)
        bv = ov[:, 0].copy()
        for j in range(1, ov.shape[1]):  # strictly greater: ties keep the first maximum
            up = ov[:, j] > bv
            best[up] = j
            bv[up] = ov[up, j]
        nt = best.astype(np.float32) + np.float32(next_start) + np.float32(0.5)
        use = nt > cur_q[:, 0]
        rows = np.arange(N)
        cur_q[use, 0] = nt[use]
        cur_q[use, 1] = traj[rows, 0, next_start + best][use]
        cur_q[use, 2] = traj[rows, 1, next_start + best][use]
    return {"traj": traj, "vis": vis, "depth": depth, "cur_q": cur_q, "plabel": plabel, "pfeat": pfeat, "best": best}


# ------------------------------------------------------------------------------------------------
# float -> engine type
# ------------------------------------------------------------------------------------------------
def cast_specials():
    """±inf, ±0, rounding ties of both 16-bit types (to even: down at 1 + 2^-8 / 1 + 2^-11, up at 1 + 3 2^-8 / 1 + 3 2^-11), values
    just beside the ties, the largest finite half and the first value that rounds to its infinity."""
    return torch.tensor([float("inf"), float("-inf"), 0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
                         -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -22, 65504.0, 65520.0, 65519.0, 1e-8, -3e38],
                        dtype=torch.float32)


def cast_ref(x, torch_dtype):
    """Round-to-nearest-even conversion of float32 data, stated on the bit patterns (bf16) / by numpy (half); float32 is a copy."""
    a = np.ascontiguousarray(x.detach().cpu().numpy().astype(np.float32))
    if torch_dtype == torch.float32:
        return torch.from_numpy(a.copy())
    if torch_dtype == torch.float16:
        with np.errstate(over="ignore"):
            return torch.from_numpy(a.astype(np.float16))
    assert torch_dtype == torch.bfloat16
    bits = a.view(np.uint32).astype(np.uint64)
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    nan = np.isnan(a)
    rounded = np.where(nan, (bits >> 16) | 0x40, rounded).astype(np.uint16)
    return torch.from_numpy(rounded.view(np.int16).copy()).view(torch.bfloat16)


def ulp_of(r, torch_dtype):
    """Spacing of ``torch_dtype`` (bfloat16 / float16) at the values r (float64 tensor)."""
    mant, emin = (7, -126) if torch_dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(r.abs().double())  # |r| = m 2^e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, emin + 1), e)
    return torch.pow(2.0, (torch.clamp(e - 1, min=emin) - mant).double())
