"""The four forms in which l4p_encoder_forward (csrc/api.hip) runs a block's two residual sums, each driven on purpose:

  1. fused GEMM epilogue (knob enc_defer_res = 0; always for the MLP sum of a block that is tapped next or is the last one),
  2. deferred through ``delta`` - the projection leaves bias + product in the engine dtype in the dead q / k slot and the next
     LayerNorm forms x + delta and writes the sum back over x (layernorm_kernel<RES>, csrc/elementwise.hip),
  3. split-K partials summed in the next block's norm1, four slices per round trip (layernorm_kernel<RES, PART>),
  4. split-K with the finish pass (splitk_finish_kernel; knob enc_sk_in_ln = 0, or a tapped / last block).

Geometry: the full model's width at depth 3 (tests/test_encoder_forms_cpu.py: forms_cfg), so no kernel sees a new shape; only the
encoder is packed and bound and Engine.encoder_forward is driven directly.  At batch 1 (M = 2048) enc_fc2_splitk gives 4 slices
of 8-phase 256x192 tiles, knob fc2_splitk8 = 0 / 5 / 8 gives 2 / 5 / 8 slices (less than one round of the four-at-a-time loop,
4 + 1 with three clamped duplicates, two full rounds); at batch 2 (M = 4096: 704 tiles >= 512) fc2 is not split and the MLP sum
takes the ``delta`` hand-over.  Every case asserts through the event profiler's tags that it launched the form it claims to test.

A. accuracy: per case and tapped layer >= 1, the whole-tensor rel-L2 and the largest per-token-row rel-L2 of the engine's float
   tap against the fp32 oracle on the same clip, held to the REFERENCE's own autocast drift for that dtype, clip and layer
   (tests/golden/encoder_forms_drift.json, tools/gen_golden_encoder_forms.py): rel_l2 <= BF16_MARGIN x, row_max <=
   BF16_MARGIN_SMALL x (a maximum over 2048 rows is an extreme-value statistic of one run on each side).  A row that misses a
   slice, the bias or its residual is off by the size of the signal - two orders of magnitude above either bar.
B. identities, bit for bit: layer 0 is the same in every case; batch rows are independent; re-runs repeat; a workspace filled
   with 0xFF bytes (NaN in f32 / bf16 / f16) or holding stale slices of a run with more slices changes nothing; a T tap is the
   float tap converted; the f32 engine ignores the three knobs.
C. the knobs are back at their shipped values afterwards."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib
from l4p_amd._lib import L4P_BF16, L4P_F16, L4P_F32
from tests.golden_utils import BF16_MARGIN, BF16_MARGIN_SMALL, make_batch
from tests.test_encoder_forms_cpu import SEEDS, forms_cfg, forms_drift

A_SEED, B_SEED = SEEDS
KNOBS_SHIPPED = {"enc_defer_res": 1, "enc_sk_in_ln": 1, "fc2_splitk8": -1}

# case -> batch (clips), float taps, knobs, what must launch: fc2 launches (count, tag part, 8-phase kernel or not: None = the
# un-split form) and LayerNorm launches tagged "res".  Counts read from api.hip:
#   norm2 is a "res" launch in every block once the projection's sum is deferred (3 blocks, 2 in ``short``);
#   norm1 of block l + 1 is a "res" launch when block l's MLP sum was handed over (delta at batch 2, partials at batch 1), which
#   needs block l + 1 not tapped and block l not the last one run.
# fc2_splitk8 = 8: 48 tiles x 8 slices = 384 workgroups is more than the one round (<= 256) the 8-phase split-K form takes
# (gemm_select.hpp), so the 8 slices run on the LDS-staged kernel - tagged "sk8", not "8p sk8".
CASES = {
    "default":     dict(clips="a", taps=(0, 3), knobs={}, fc2=(3, " sk4 ", True), res=5),
    "finish":      dict(clips="a", taps=(0, 3), knobs={"enc_sk_in_ln": 0}, fc2=(3, " sk4 ", True), res=3),
    "fused":       dict(clips="a", taps=(0, 3), knobs={"enc_defer_res": 0}, fc2=(3, " sk4 ", True), res=0),
    "sk2":         dict(clips="a", taps=(0, 3), knobs={"fc2_splitk8": 0}, fc2=(3, " sk2 ", False), res=5),
    "sk5":         dict(clips="a", taps=(0, 3), knobs={"fc2_splitk8": 5}, fc2=(3, " sk5 ", True), res=5),
    "sk8":         dict(clips="a", taps=(0, 3), knobs={"fc2_splitk8": 8}, fc2=(3, " sk8 ", False), res=5),
    "delta":       dict(clips="ab", taps=(0, 3), knobs={}, fc2=(3, None, False), res=5),
    "delta-fused": dict(clips="ab", taps=(0, 3), knobs={"enc_defer_res": 0}, fc2=(3, None, False), res=0),
    "all-taps":    dict(clips="a", taps=(0, 1, 2, 3), knobs={}, fc2=(3, " sk4 ", True), res=3),
    "mid-tap":     dict(clips="a", taps=(0, 2, 3), knobs={}, fc2=(3, " sk4 ", True), res=4),
    "short":       dict(clips="a", taps=(0, 2), knobs={}, fc2=(2, " sk4 ", True), res=3),
}
POISON_CASES = ("default", "finish", "sk5", "delta", "mid-tap")


class prof_tags:
    """Collect the (class, tag, count) lines of every launch inside the block (l4p_prof_detail)."""

    def __enter__(self):
        self.lib = _lib.load()
        torch.cuda.synchronize()
        self.lib.l4p_prof_reset()
        self.lib.l4p_prof_enable(1)
        self.lines = []
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.l4p_prof_enable(0)
        n = self.lib.l4p_prof_detail(None, 0)
        buf = C.create_string_buffer(int(n) + 16)
        self.lib.l4p_prof_detail(buf, len(buf))
        self.lines = [ln.split("\t") for ln in buf.value.decode().splitlines() if ln]
        self.lib.l4p_prof_reset()
        return False

    def launches(self, cls, part):
        """[(tag, count)] of the launches of one class whose tag contains ``part``."""
        return [(ln[1], int(ln[2])) for ln in self.lines if ln[0] == cls and part in ln[1]]


# ---- shared, computed once per module ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup():
    """Geometry, name-seeded encoder weights, the two clips and their fp32 oracle features (CPU, once)."""
    from l4p_amd.weights import seeded_state_dict
    from oracle.l4p_oracle import encoder_forward

    cfg = forms_cfg()
    sd = seeded_state_dict(cfg, tasks=[])
    clips = {"a": make_batch(16, 0, seed=A_SEED)["rgb_b3thw"], "b": make_batch(16, 0, seed=B_SEED)["rgb_b3thw"]}
    with torch.no_grad():
        oracle = {k: [f[0] for f in encoder_forward(sd, v, cfg)] for k, v in clips.items()}
    return dict(cfg=cfg, sd=sd, clips=clips, oracle=oracle, drift=forms_drift())


def _engine(setup, dev, mode):
    from l4p_amd.engine import Engine
    from l4p_amd.ops import torch_dtype
    from l4p_amd.packing import pack_state_dict

    pw = pack_state_dict(setup["sd"], setup["cfg"], torch_dtype(mode), dev, tasks=[])
    return Engine(setup["cfg"], pw, mode, dev)


@pytest.fixture(scope="module", params=[L4P_BF16, L4P_F16], ids=["bf16", "f16"])
def eng(request, setup, dev):
    """One engine per 16-bit dtype, with the cache of the cases it has run: {case: (taps on the CPU, profiler lines)}."""
    e = _engine(setup, dev, request.param)
    e.forms_cache = {}
    e.forms_name = "bf16" if request.param == L4P_BF16 else "f16"
    yield e
    del e.forms_cache


@pytest.fixture(scope="module")
def eng_f32(setup, dev):
    return _engine(setup, dev, L4P_F32)


def _rgb(setup, clips: str, dev):
    return torch.cat([setup["clips"][c] for c in clips]).to(dev).contiguous()


def _forward(e, rgb, taps, taps_T=(), poison=False):
    """One encoder forward -> ({layer: float tap}, {layer: T tap}) on the CPU."""
    if poison:
        e._workspace(rgb.shape[0]).fill_(0xFF)
    f, t = e.encoder_forward(rgb, taps, taps_T)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in f.items()}, {k: v.cpu() for k, v in t.items()}


def _set(knob, knobs):
    for k, v in KNOBS_SHIPPED.items():  # (every knob is set: a case never inherits another's)
        knob(k, knobs.get(k, v))


def _case(e, setup, knob, name, dev):
    """The float taps of a case (run once per engine, under the profiler) and its launches."""
    if name not in e.forms_cache:
        c = CASES[name]
        _set(knob, c["knobs"])
        rgb = _rgb(setup, c["clips"], dev)
        with prof_tags() as p:
            f, _ = _forward(e, rgb, c["taps"])
        e.forms_cache[name] = (f, p)
    return e.forms_cache[name]


def _row_metrics(y: torch.Tensor, ref: torch.Tensor):
    """[P, C] engine tap against the oracle -> (whole-tensor rel-L2, largest per-row rel-L2), in float64."""
    y, ref = y.double(), ref.double()
    rows = (y - ref).norm(dim=-1) / ref.norm(dim=-1)
    return float((y - ref).norm() / ref.norm()), float(rows.max())


# ---- the case table: launches + A ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_form_within_reference_drift(eng, setup, knob, dev, name):
    c = CASES[name]
    f, p = _case(eng, setup, knob, name, dev)
    # -- the launches prove the case ran the form it claims to test
    n_fc2, part, is8p = c["fc2"]
    fc2 = p.launches("gemm", " K6144 ")
    assert sum(n for _, n in fc2) == n_fc2, p.lines
    for tag, _ in fc2:
        if part is None:
            assert " sk1 " in tag or " sk" not in tag, p.lines
        else:
            assert part in tag and (" 8p " in tag) == is8p, p.lines
    assert sum(n for _, n in p.launches("layernorm", " res ")) == c["res"], p.lines
    # -- A: float taps against the fp32 oracle, bar = the reference's own autocast drift
    ratios, bad = {}, {}
    for bi, clip in enumerate(c["clips"]):
        seed = A_SEED if clip == "a" else B_SEED
        for layer in c["taps"]:
            y = f[layer][bi]
            assert bool(torch.isfinite(y).all()), (name, clip, layer)
            if layer == 0:
                continue
            want = setup["drift"][eng.forms_name][f"clip{seed}"][f"feat{layer}"]
            rel, row = _row_metrics(y, setup["oracle"][clip][layer])
            r = (rel / want["rel_l2"], row / want["row_max"])
            ratios[f"{clip}{layer}"] = f"rel_l2 {r[0]:.2f} row_max {r[1]:.2f}"
            if r[0] > BF16_MARGIN or r[1] > BF16_MARGIN_SMALL:
                bad[f"{clip}{layer}"] = (rel, row, want)
    print(f"{eng.forms_name} engine drift / reference autocast drift [encoder forms, {name}]:", ratios)
    assert not bad, (name, bad)


# ---- B: identities ---------------------------------------------------------------------------------------------------------------------------
def test_layer0_is_the_same_in_every_case(eng, setup, knob, dev):
    """The patch embed + position table: knobs and taps must not reach it."""
    base = _case(eng, setup, knob, "default", dev)[0][0][0]
    for name, c in CASES.items():
        f, _ = _case(eng, setup, knob, name, dev)
        if c["clips"] == "a":
            assert torch.equal(f[0][0], base), name
    # (batch 2: the same rows, whichever position the clip has in the batch)
    d, df = _case(eng, setup, knob, "delta", dev)[0][0], _case(eng, setup, knob, "delta-fused", dev)[0][0]
    assert torch.equal(d, df)
    assert torch.equal(d[0], base), "clip a's embeddings differ between batch 1 and batch 2"


@pytest.mark.parametrize("name", ["delta", "delta-fused"])
def test_batch_rows_are_independent(eng, setup, knob, dev, name):
    """[a, b] and [b, a] give the same bits per clip, [a, a] two equal halves: every kernel on this path computes a row, or a
    (batch, head) tile, in an order that does not depend on its position."""
    c = CASES[name]
    ab, _ = _case(eng, setup, knob, name, dev)
    _set(knob, c["knobs"])
    ba, _ = _forward(eng, _rgb(setup, "ba", dev), c["taps"])
    aa, _ = _forward(eng, _rgb(setup, "aa", dev), c["taps"])
    for layer in c["taps"]:
        assert torch.equal(ab[layer][0], ba[layer][1]), (name, layer, "clip a")
        assert torch.equal(ab[layer][1], ba[layer][0]), (name, layer, "clip b")
        assert torch.equal(aa[layer][0], aa[layer][1]), (name, layer, "[a, a]")
        assert torch.equal(aa[layer][0], ab[layer][0]), (name, layer, "[a, a] vs [a, b]")


@pytest.mark.parametrize("name", list(CASES))
def test_rerun_gives_the_same_bits(eng, setup, knob, dev, name):
    """Fixed slice order, no atomics."""
    c = CASES[name]
    first, _ = _case(eng, setup, knob, name, dev)
    _set(knob, c["knobs"])
    again, _ = _forward(eng, _rgb(setup, c["clips"], dev), c["taps"])
    for layer in c["taps"]:
        assert torch.equal(first[layer], again[layer]), (name, layer)


@pytest.mark.parametrize("name", POISON_CASES)
def test_workspace_contents_do_not_matter(eng, setup, knob, dev, name):
    """The workspace holds activations only: filled with 0xFF bytes (NaN in every engine type) before the forward, the result
    is finite and the same bits - no form reads a slot that it, or the kernels before it, did not write."""
    c = CASES[name]
    clean, _ = _case(eng, setup, knob, name, dev)
    _set(knob, c["knobs"])
    got, _ = _forward(eng, _rgb(setup, c["clips"], dev), c["taps"], poison=True)
    for layer in c["taps"]:
        assert bool(torch.isfinite(got[layer]).all()), (name, layer)
        assert torch.equal(got[layer], clean[layer]), (name, layer)


def test_stale_slices_past_the_last_are_not_read(eng, setup, knob, dev):
    """8, then 5, then the default 4 slices on the same engine: the partials buffer holds the earlier run's slices past the last
    one in use (and the clamped duplicate lanes of the four-at-a-time loop point at live ones)."""
    rgb = _rgb(setup, "a", dev)
    want = {n: _case(eng, setup, knob, n, dev)[0] for n in ("sk8", "sk5", "default")}
    eng._workspace(1).fill_(0xFF)
    for n in ("sk8", "sk5", "default"):
        _set(knob, CASES[n]["knobs"])
        got, _ = _forward(eng, rgb, CASES[n]["taps"])
        for layer in CASES[n]["taps"]:
            assert torch.equal(got[layer], want[n][layer]), (n, layer)


@pytest.mark.parametrize("name,layer", [("all-taps", 2), ("default", 3)])
def test_T_tap_is_the_float_tap_converted(eng, setup, knob, dev, name, layer):
    """One call, the same layer as float and as T (layer 2: the cast of x; layer 3: the final norm's two outputs)."""
    c = CASES[name]
    _set(knob, c["knobs"])
    f, t = _forward(eng, _rgb(setup, c["clips"], dev), c["taps"], taps_T=(layer,))
    assert t[layer].dtype == eng.tdtype
    assert torch.equal(t[layer], f[layer].to(eng.tdtype))
    assert torch.equal(f[layer], _case(eng, setup, knob, name, dev)[0][layer])  # (asking for the T tap changes nothing else)


def test_f32_engine_ignores_the_knobs(eng_f32, setup, knob, dev):
    """The float engine keeps the fused form whatever the knobs say, and meets the f32 bar (1e-3 of max |ref|) at every layer."""
    rgb = _rgb(setup, "a", dev)
    taps = (0, 1, 2, 3)
    out = []
    for knobs in ({}, {"enc_defer_res": 0, "enc_sk_in_ln": 0, "fc2_splitk8": 5}):
        _set(knob, knobs)
        with prof_tags() as p:
            f, _ = _forward(eng_f32, rgb, taps)
        assert sum(n for _, n in p.launches("layernorm", " res ")) == 0, p.lines
        assert all(" sk1 " in tag or " sk" not in tag for tag, _ in p.launches("gemm", " K6144 ")), p.lines
        out.append(f)
    for layer in taps:
        assert torch.equal(out[0][layer], out[1][layer]), layer
        ref = setup["oracle"]["a"][layer]
        err = float((out[0][layer][0] - ref).abs().max() / ref.abs().max())
        print(f"f32 engine layer {layer}: max |diff| / max |ref| = {err:.2e}")
        assert err <= 1e-3, (layer, err)


# ---- C ----------------------------------------------------------------------------------------------------------------------------------------
def test_knobs_are_back_at_their_shipped_values(dev):
    lib = _lib.load()
    assert {k: int(lib.l4p_get_knob(k.encode())) for k in KNOBS_SHIPPED} == KNOBS_SHIPPED
