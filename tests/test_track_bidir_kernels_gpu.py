"""GPU: the three entry points of csrc/track_bidir.hip, each called through the C ABI on its own and held bit for bit to the
definition in tests/track_bidir_restate.py (pure data movement and f32 comparisons: nothing to round differently)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l4p_amd import _lib
from l4p_amd.ops import _p, _stream
from tests import track_bidir_restate as rs

INVALID = _lib.L4P_E_INVALID


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _times(n: int, T: int, seed: int) -> np.ndarray:
    """n query times: the edges of the rule first, then frame centres and times between frames all over (and past) the clip."""
    rng = np.random.default_rng(seed)
    edge = np.array(rs.edge_times(T), dtype=np.float32)
    rest = np.concatenate([rng.integers(0, T + 1, n).astype(np.float32) + 0.5, rng.uniform(-1.0, T + 1.0, n).astype(np.float32)])
    rng.shuffle(rest)
    return np.concatenate([edge, rest])[:n] if n >= len(edge) else rng.permutation(edge)[:n]


@pytest.mark.parametrize("inner", [1, 7, 64, 50176])
@pytest.mark.parametrize("T", [1, 2, 5, 16])
@pytest.mark.parametrize("outer", [1, 3])
def test_time_reverse(dev, outer, T, inner):
    lib = _lib.load()
    x = torch.randn(outer, T, inner, generator=torch.Generator().manual_seed(outer * 1000 + T * 10 + inner % 7)).to(dev)
    guard = 8
    buf = torch.full((outer * T * inner + 2 * guard,), 7.0, device=dev)
    dst = buf[guard:guard + x.numel()]  # (32 bytes in: as aligned as the allocation; the floats around it must stay as they are)
    _lib.check(lib.l4p_time_reverse(_stream(), _p(x), dst.data_ptr(), outer, T, inner), "l4p_time_reverse")
    torch.cuda.synchronize()
    assert torch.equal(dst.view(outer, T, inner), x.flip(1))
    assert np.array_equal(dst.view(outer, T, inner).cpu().numpy(), rs.time_reverse(x.cpu().numpy()))
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + x.numel():] == 7.0).all())


@pytest.mark.parametrize("which", ["dst", "src"])
def test_time_reverse_misaligned_pointer_takes_the_scalar_path(dev, which):
    """inner % 4 == 0 but one pointer sits one float off a 16-byte boundary: scalar accesses, still exact, nothing beside it written."""
    lib = _lib.load()
    outer, T, inner = 3, 5, 64
    n = outer * T * inner
    src_buf = torch.randn(n + 8, generator=torch.Generator().manual_seed(3)).to(dev)
    dst_buf = torch.full((n + 8,), 7.0, device=dev)
    so, do = (0, 1) if which == "dst" else (1, 0)
    src, dst = src_buf[so:so + n], dst_buf[do:do + n]
    assert (src.data_ptr() % 16 != 0) != (dst.data_ptr() % 16 != 0)
    _lib.check(lib.l4p_time_reverse(_stream(), src.data_ptr(), dst.data_ptr(), outer, T, inner), "l4p_time_reverse")
    torch.cuda.synchronize()
    assert torch.equal(dst.view(outer, T, inner), src.view(outer, T, inner).flip(1))
    assert bool((dst_buf[:do] == 7.0).all()) and bool((dst_buf[do + n:] == 7.0).all())


def test_time_reverse_invalid_arguments(dev):
    lib = _lib.load()
    x = torch.zeros(2, 4, 8, device=dev)
    y = torch.full_like(x, 7.0)
    for args in ((_p(x), _p(x), 2, 4, 8), (_p(x), _p(y), 2, 0, 8), (_p(x), _p(y), 0, 4, 8), (_p(x), _p(y), 2, 4, 0),
                 (None, _p(y), 2, 4, 8), (_p(x), None, 2, 4, 8)):
        assert lib.l4p_time_reverse(_stream(), *args) == INVALID, args
        assert b"l4p_time_reverse" in lib.l4p_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # nothing was launched


@pytest.mark.parametrize("BN", [1, 63, 65, 257])
def test_bidir_queries(dev, BN):
    lib = _lib.load()
    T = 16
    rng = np.random.default_rng(BN)
    q = rng.uniform(0.0, 224.0, (BN, 3)).astype(np.float32)
    q[:, 0] = _times(BN, T, BN)
    want = rs.need_count(q[:, 0])
    qd = torch.from_numpy(q).to(dev)
    out = torch.full((BN + 1, 3), 7.0, device=dev)
    count = torch.full((3,), 5, dtype=torch.int32, device=dev)  # (the entry ADDS to [1]; its neighbours stay)
    _lib.check(lib.l4p_track_bidir_queries(_stream(), _p(qd), T, _p(out), count[1:].data_ptr(), BN), "l4p_track_bidir_queries")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = rs.flip_queries(q, T)
    assert np.array_equal(np.isnan(got[:BN]), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(_bits(got[:BN])[ok], _bits(ref)[ok])
    assert (got[BN] == 7.0).all()
    assert count.cpu().tolist() == [5, 5 + want, 5]
    if BN >= 7:
        assert 0 < want < BN
    # every query on frame 0: nothing for the reversed pass
    q[:, 0] = 0.5
    count.zero_()
    _lib.check(lib.l4p_track_bidir_queries(_stream(), _p(torch.from_numpy(q).to(dev)), T, _p(out), count[1:].data_ptr(), BN),
               "l4p_track_bidir_queries")
    assert count.cpu().tolist() == [0, 0, 0]
    assert bool((out[:BN, 0] == T - 0.5).all())


def test_bidir_queries_invalid_arguments(dev):
    lib = _lib.load()
    q = torch.zeros(4, 3, device=dev)
    out = torch.full((4, 3), 7.0, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    for args in ((None, 16, _p(out), _p(count), 4), (_p(q), 16, None, _p(count), 4), (_p(q), 16, _p(out), None, 4),
                 (_p(q), 0, _p(out), _p(count), 4), (_p(q), 16, _p(out), _p(count), 0)):
        assert lib.l4p_track_bidir_queries(_stream(), *args) == INVALID, args
        assert b"l4p_track_bidir_queries" in lib.l4p_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(count.item()) == 0


def _merge_case(B, N, T, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 224.0, (B, N, 3)).astype(np.float32)
    q[..., 0] = _times(B * N, T, seed).reshape(B, N)
    arrays = lambda: [rng.standard_normal((B, N, c, T)).astype(np.float32) for c in (2, 1, 1)]  # noqa: E731
    return q, arrays(), arrays()


@pytest.mark.parametrize("T", [1, 16, 24])
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("B", [1, 2])
def test_bidir_merge(dev, B, N, T):
    lib = _lib.load()
    q, fwd, rev = _merge_case(B, N, T, B * 100 + N + T)
    qd = torch.from_numpy(q).to(dev)
    fd = [torch.from_numpy(a).to(dev) for a in fwd]
    rd = [torch.from_numpy(a).to(dev) for a in rev]

    def check(outs, want, what):
        torch.cuda.synchronize()
        for o, w, k in zip(outs, want, rs.KEYS):
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(w)), (what, k)

    # both passes, separate outputs
    outs = [torch.full_like(t, 7.0) for t in fd]
    _lib.check(lib.l4p_track_bidir_merge(_stream(), _p(qd), *map(_p, fd), *map(_p, rd), *map(_p, outs), B, N, T, 0), "merge 0")
    want0 = rs.merge(q, fwd, rev, 0)
    check(outs, want0, "mode 0")
    for t, a in zip(fd + rd, fwd + rev):  # the inputs are read only
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
    # no forward pass: fill values on the forward-owned frames, the forward pointers NULL
    outs = [torch.full_like(t, 7.0) for t in fd]
    _lib.check(lib.l4p_track_bidir_merge(_stream(), _p(qd), None, None, None, *map(_p, rd), *map(_p, outs), B, N, T, 1), "merge 1")
    check(outs, rs.merge(q, None, rev, 1), "mode 1")
    # both passes, written over the forward buffers
    _lib.check(lib.l4p_track_bidir_merge(_stream(), _p(qd), *map(_p, fd), *map(_p, rd), *map(_p, fd), B, N, T, 0), "merge alias")
    check(fd, want0, "mode 0, outputs on the forward buffers")


def test_bidir_merge_invalid_arguments(dev):
    lib = _lib.load()
    B, N, T = 1, 3, 4
    q, fwd, rev = _merge_case(B, N, T, 1)
    qd = _p(torch.from_numpy(q).to(dev))
    fd = [torch.from_numpy(a).to(dev) for a in fwd]
    rd = [torch.from_numpy(a).to(dev) for a in rev]
    outs = [torch.full_like(t, 7.0) for t in fd]
    f, r, o = list(map(_p, fd)), list(map(_p, rd)), list(map(_p, outs))
    bad = [(None, *f, *r, *o, B, N, T, 0), (qd, *f, *r, *o, 0, N, T, 0), (qd, *f, *r, *o, B, 0, T, 0), (qd, *f, *r, *o, B, N, 0, 0),
           (qd, *f, *r, *o, B, N, T, 2), (qd, *f, *r, *o, B, N, T, -1), (qd, None, None, None, *r, *o, B, N, T, 0)]
    for i in range(3):
        for grp, mode in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
            ptrs = [list(f), list(r), list(o)]
            ptrs[grp][i] = None
            bad.append((qd, *ptrs[0], *ptrs[1], *ptrs[2], B, N, T, mode))
    for args in bad:
        assert lib.l4p_track_bidir_merge(_stream(), *args) == INVALID, args
        assert b"l4p_track_bidir_merge" in lib.l4p_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)  # nothing was launched
