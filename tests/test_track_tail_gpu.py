"""The tracker's output tail - l4p_mask_gather and both forms of l4p_track_readout (csrc/track_readout.hip) - against the float64
references of tests/kernel_refs.py (checked on the CPU by tests/test_kernel_refs_cpu.py), at the smallest shapes that reach each path of
launch_track_readout and of the two kernels: R.READOUT_CASES says which case reaches what (held to the selection itself, with grid and
LDS sizes, by tests/test_track_select_cpu.py).

Every read-out case runs with the knob readout_wide on and off and asserts that the two runs agree bit for bit, that the launch carried
the tag the case expects (l4p_prof_detail), that the sentinel-filled outputs are fully overwritten with nothing written around them, and
parity with track_readout_ref.  Gates (the project's own, tests/test_kernels_gpu.py): traj <= 1e-3 px absolute, vis <= 1e-5 max(1, max|ref|),
depth <= 1e-5 relative.  The kernel's float arithmetic emulated on the CPU stays at <= 3.1e-5 px, 6e-8 and 8e-8 on these shapes.
MEASURED on MI355X (largest over all cases of this file): see TRAJ_SEEN, VIS_SEEN, DEPTH_SEEN below.

Peaked logits (one source pixel `span` above the rest): the kernels shift the exponent by the maximum of the low-resolution SOURCE, which
bounds the up-sampled maximum from above but is not attained when the peak lies between output samples (the best sample of an interior
peak at 4x carries weight 0.875^2: its exponent is -0.234 span) or is skipped by a down-sampling grid; with span >= 600 every sample's
exponential then underflows, z = 0 and traj = 0 / 0.  The kernels therefore repeat the soft-argmax with the exact up-sampled maximum
when z comes out below 2^-64 (track_readout.hip, READOUT_Z_MIN); the cases here hold both forms to the float64 value on that path as well.
Before that change the seven interior cases with span 600 / 2000 (int4_nonsquare, wide_W, model, lds_over) returned traj = NaN from both
forms on MI355X and every other case of this file passed.
No case is skipped: a launch that launch_track_readout refuses is asserted to return L4P_E_INVALID before any launch.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib
from tests import kernel_refs as R
from tests.test_kernels_gpu import rnd

E_INVALID = _lib.L4P_E_INVALID
SENT = 0xA5          # sentinel byte of pre-filled buffers
SENT32 = -1515870811  # 0xA5A5A5A5 as int32
GUARD = 64           # sentinel floats around and between the outputs

TRAJ_GATE, VIS_GATE, DEPTH_GATE = 1e-3, 1e-5, 1e-5
# largest [measured] values of this file on MI355X (traj: model, peak at the last pixel, span 100; vis / depth: many_groups); the peaked
# cases on the exact-maximum path stay at <= 2.3e-5 px.  Records, not gates.
TRAJ_SEEN, VIS_SEEN, DEPTH_SEEN = 4.4e-5, 1.2e-7, 1.5e-7

CASES = {c[0]: c for c in R.READOUT_CASES}
TAG_WIDE, TAG_COLUMN = "track_readout wide", "track_readout"


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def report(what, value):
    print(f"[measured] {what}: {value:.3e}")


class prof_tags:
    """The (class, tag, count) of every launch inside the block (l4p_prof_detail: class, tag, count, ms)."""

    def __enter__(self):
        torch.cuda.synchronize()
        lib().l4p_prof_reset()
        lib().l4p_prof_enable(1)
        self.launches = []
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib().l4p_prof_enable(0)
        n = lib().l4p_prof_detail(None, 0)
        buf = C.create_string_buffer(int(n) + 16)
        lib().l4p_prof_detail(buf, len(buf))
        lines = [ln.split("\t") for ln in buf.value.decode().splitlines() if ln]
        self.launches = [(ln[0], ln[1], int(float(ln[2]))) for ln in lines]
        lib().l4p_prof_reset()
        return False


class Arena:
    """Float outputs carved out of one sentinel-filled buffer with GUARD sentinel floats before, between and after them."""

    def __init__(self, *shapes):
        sizes = [int(np.prod(s)) for s in shapes]
        self.buf = torch.full((4 * (GUARD + sum(n + GUARD for n in sizes)),), SENT, dtype=torch.uint8, device="cuda").view(torch.float32)
        self.views, self.spans, off = [], [], GUARD
        for s, n in zip(shapes, sizes):
            self.views.append(self.buf[off:off + n].view(s))
            self.spans.append((off, off + n))
            off += n + GUARD

    def untouched_outside(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for a, b in self.spans:
            keep[a:b] = False
        return bool((self.buf.view(torch.int32)[keep] == SENT32).all())

    def fully_written(self):
        return all(bool((v.contiguous().view(torch.int32) != SENT32).all()) for v in self.views)

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENT32).all())


def readout_call(masks, N, T, h, w, H, W, arena):
    traj, vis, dep = arena.views
    return lib().l4p_track_readout(st(), None if masks is None else masks.data_ptr(), traj.data_ptr(), vis.data_ptr(), dep.data_ptr(),
                                   N, T, h, w, H, W)


def run_both_forms(knob, masks, H, W, tag_on):
    """masks: float32 CPU [N][3][T][h][w].  Runs the read-out with readout_wide = 1 and 0; asserts the tag of each launch, the sentinel
    rules and the bitwise equality of the two runs; returns the outputs (float32 CPU tensors traj, vis, depth)."""
    N, _, T, h, w = masks.shape
    md = masks.cuda().contiguous()
    outs = {}
    for wide in (1, 0):
        knob("readout_wide", wide)
        arena = Arena((N, 2, T), (N, T), (N, T))
        with prof_tags() as p:
            _lib.check(readout_call(md, N, T, h, w, H, W, arena), "l4p_track_readout")
        want = tag_on if wide else TAG_COLUMN
        assert p.launches == [("track", want, 1)], f"readout_wide={wide}: expected one launch tagged {want!r}, saw {p.launches}"
        assert arena.untouched_outside(), f"readout_wide={wide}: wrote outside traj / vis / depth"
        assert arena.fully_written(), f"readout_wide={wide}: an output element was left unwritten"
        outs[wide] = [v.cpu().clone() for v in arena.views]
    assert torch.equal(md.cpu(), masks), "the read-out changed its input"
    for name, a, b in zip(("traj", "vis", "depth"), outs[1], outs[0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: the two forms differ (knob on vs off)"
    return outs[1]


def check_parity(what, out, ref, gate_vis_depth=True):
    traj, vis, dep = (t.double().numpy() for t in out)
    rt, rv, rd = ref
    assert np.isfinite(traj).all() and np.isfinite(vis).all() and np.isfinite(dep).all(), f"{what}: non-finite output (traj {traj.ravel()[:4]})"
    et = np.abs(traj - rt).max()
    ev = np.abs(vis - rv).max() / max(1.0, np.abs(rv).max())
    ed = (np.abs(dep - rd) / np.abs(rd)).max()
    report(f"{what} traj px", et)
    report(f"{what} vis", ev)
    report(f"{what} depth rel", ed)
    assert et <= TRAJ_GATE, f"{what}: traj off by {et:.3e} px"
    if gate_vis_depth:
        assert ev <= VIS_GATE, f"{what}: vis off by {ev:.3e}"
        assert ed <= DEPTH_GATE, f"{what}: depth off by {ed:.3e} (relative)"


def base_masks(name):
    """randn * 3 with one seed per channel: the three channels cannot be confused."""
    _, (N, T), (h, w), _, _ = CASES[name]
    return torch.stack([rnd((N, T, h, w), 1400 + 10 * list(CASES).index(name) + c, 3.0) for c in range(3)], dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def base_ref(name):
    _, _, _, (H, W), _ = CASES[name]
    return R.track_readout_ref(base_masks(name).numpy(), H, W)


def tag_of(name):
    return TAG_WIDE if CASES[name][4] else TAG_COLUMN


# ------------------------------------------------------------------------------------------------
# l4p_track_readout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_readout_vs_float64(dev, knob, name):
    _, _, _, (H, W), _ = CASES[name]
    out = run_both_forms(knob, base_masks(name), H, W, tag_of(name))
    check_parity(name, out, base_ref(name))


def test_readout_identity_one_hot_is_the_pixel_centre(dev, knob):
    """h == H, w == W: lam == 0 everywhere, the samples are the source values; a one-hot logit map gives its pixel centre exactly."""
    _, (N, T), (h, w), (H, W), _ = CASES["identity"]
    masks = base_masks("identity")
    masks[:, 0] = -1000.0
    masks[0, 0, 0, 4, 1] = 1000.0
    masks[0, 0, 1, 6, 4] = 1000.0
    traj, vis, dep = run_both_forms(knob, masks, H, W, TAG_WIDE)
    assert traj[0, :, 0].tolist() == [1.5, 4.5] and traj[0, :, 1].tolist() == [4.5, 6.5]
    check_parity("identity one-hot", (traj, vis, dep), R.track_readout_ref(masks.numpy(), H, W))


PEAK_SHAPES = ["int4_nonsquare", "wide_W", "model"]
PEAK_CASES = [(n, pos, span) for n in PEAK_SHAPES for pos in ("first", "last", "interior") for span in (100, 600, 2000)]
PEAK_CASES.append(("lds_over", "interior", 600))  # down-sampling: the grid skips the source maximum


def peaked_masks(name, pos, span):
    _, (N, T), (h, w), _, _ = CASES[name]
    masks = base_masks(name)
    masks[:, 0] = rnd((N, T, h, w), 1390) - span / 2
    y, x = {"first": (0, 0), "last": (h - 1, w - 1), "interior": (h // 2, w // 3)}[pos]
    masks[:, 0, :, y, x] = span / 2
    return masks


@pytest.mark.parametrize("name,pos,span", PEAK_CASES, ids=[f"{n}-{p}-{s}" for n, p, s in PEAK_CASES])
def test_readout_peaked_logits_stay_finite_and_exact(dev, knob, name, pos, span):
    """Channel 0 = randn - span / 2 with one source pixel at + span / 2 (see the file's docstring).  All outputs finite, traj within 1e-3 px
    of float64, both forms bitwise equal, vis / depth the very bits of the run on the unpeaked map (they do not depend on channel 0)."""
    _, _, _, (H, W), _ = CASES[name]
    masks = peaked_masks(name, pos, span)
    out = run_both_forms(knob, masks, H, W, tag_of(name))
    rt, _, _ = R.track_readout_ref(masks.numpy(), H, W)
    _, rv, rd = base_ref(name)
    check_parity(f"{name} peak {pos} span {span}", out, (rt, rv, rd))
    base = run_both_forms(knob, base_masks(name), H, W, tag_of(name))
    assert torch.equal(out[1].view(torch.int32), base[1].view(torch.int32)), "vis depends on channel 0"
    assert torch.equal(out[2].view(torch.int32), base[2].view(torch.int32)), "depth depends on channel 0"


@pytest.mark.parametrize("value", [0.0, -1e4])
@pytest.mark.parametrize("name", [n for n in CASES if n != "many_groups"])
def test_readout_flat_map_gives_the_image_centre(dev, knob, name, value):
    """A constant channel 0: every sample weighs the same and the soft-argmax is the image centre (W / 2, H / 2).  At -1e4 too: the shift
    by the maximum makes the estimate independent of the level."""
    _, _, _, (H, W), _ = CASES[name]
    masks = base_masks(name)
    masks[:, 0] = value
    traj, vis, dep = run_both_forms(knob, masks, H, W, tag_of(name))
    ex, ey = (traj[:, 0] - W / 2).abs().max().item(), (traj[:, 1] - H / 2).abs().max().item()
    report(f"{name} flat {value:g} centre px", max(ex, ey))
    assert bool(torch.isfinite(traj).all()) and max(ex, ey) <= TRAJ_GATE
    check_parity(f"{name} flat {value:g}", (traj, vis, dep), R.track_readout_ref(masks.numpy(), H, W))


REFUSALS = [("null masks", {"masks": None}), ("null traj", {"null": 0}), ("null vis", {"null": 1}), ("null depth", {"null": 2}),
            ("N = 0", {"N": 0}), ("T = 0", {"T": 0}), ("h = 0", {"h": 0}), ("w = -1", {"w": -1}), ("H = 0", {"H": 0}), ("W = 0", {"W": 0}),
            # the column form's request (3 h w + w + h) * 4 = 173 760 B > 160 KiB, the wide form's is larger still
            ("LDS over the limit", {"h": 120, "w": 120, "H": 16, "W": 16})]


@pytest.mark.parametrize("what,change", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("wide", [1, 0])
def test_readout_refusals_launch_nothing(dev, knob, wide, what, change):
    knob("readout_wide", wide)
    a = dict(N=2, T=2, h=6, w=10, H=20, W=36)
    a.update({k: v for k, v in change.items() if k in a})
    masks = torch.zeros(2, 3, 2, max(a["h"], 1), max(a["w"], 1), device="cuda")
    arena = Arena((2, 2, 2), (2, 2), (2, 2))
    ptrs = [v.data_ptr() for v in arena.views]
    if "null" in change:
        ptrs[change["null"]] = None
    with prof_tags() as p:
        rc = lib().l4p_track_readout(st(), None if "masks" in change else masks.data_ptr(), *ptrs, a["N"], a["T"], a["h"], a["w"], a["H"], a["W"])
    assert rc == E_INVALID, f"{what}: rc = {rc}"
    assert "track_readout" in lib().l4p_last_error().decode()
    assert p.launches == [] and arena.untouched()


# ------------------------------------------------------------------------------------------------
# l4p_mask_gather
# ------------------------------------------------------------------------------------------------
def gather(partial, N, T, h, w, cpt):
    arena = Arena((N, 3, T, 2 * h, 2 * w))
    pd = partial.cuda().contiguous()
    _lib.check(lib().l4p_mask_gather(st(), pd.data_ptr(), arena.views[0].data_ptr(), N, T, h, w, cpt), "l4p_mask_gather")
    torch.cuda.synchronize()
    assert arena.untouched_outside() and arena.fully_written()
    assert torch.equal(pd.cpu(), partial)
    return arena.views[0]


@pytest.mark.parametrize("N,T,h,w,cpt", R.MASK_GATHER_CASES)
def test_mask_gather_nonsquare_is_exact(dev, N, T, h, w, cpt):
    """A random partial driven straight into l4p_mask_gather at h != w (a swap of the two in the row or tap index moves every voxel), at a
    size of many blocks (368 640 outputs per channel: 1440 blocks) and at one past the grid cap (GRID1D(total, 16384): 16 384 blocks of
    256 threads cover 4 194 304 voxels; 4 262 400 send the grid-stride loop on a second trip).  A fixed-order float sum of cpt terms:
    exact."""
    partial = rnd((4 * cpt, 3, N * T * h * w), 1500)
    got = gather(partial, N, T, h, w, cpt).cpu().numpy()
    assert np.array_equal(got, R.mask_gather_ref(partial.numpy(), N, T, h, w, cpt))


def test_mask_gather_then_readout_chained(dev, knob):
    """l4p_mask_gather at h, w = 3, 5 -> masks 6 x 10 -> read-out at 20 x 36, against the two references chained."""
    N, T, h, w, cpt, H, W = 2, 3, 3, 5, 2, 20, 36
    partial = rnd((4 * cpt, 3, N * T * h * w), 1501, 1.5)
    masks = gather(partial, N, T, h, w, cpt).cpu().clone()
    ref_masks = R.mask_gather_ref(partial.numpy(), N, T, h, w, cpt)
    assert np.array_equal(masks.numpy(), ref_masks)
    out = run_both_forms(knob, masks, H, W, TAG_WIDE)
    check_parity("chained", out, R.track_readout_ref(ref_masks, H, W))
