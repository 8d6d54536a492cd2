"""CPU tier: tests/guards.py would fail on a wrong kernel. Ordinary torch functions on CPU tensors stand in for kernels; each wrong
one is caught by the mechanism named for it (halo check, NaN fill, 3e38 fill, 0xA5 pattern, allocation count)."""
import types

import pytest
import torch

from tests import guards as G


def _fake_engine():
    """A module whose wrappers allocate through its own ``torch`` name, the way text2loc_amd.engine does."""
    m = types.ModuleType("fake_engine")
    m.torch = torch
    src = """
def row_sums(x, rows=None, write=None):
    n = int(x.shape[0])
    out = torch.empty((n,), dtype=torch.float32, device=x.device)
    flag = torch.zeros((1,), dtype=torch.int32)
    like = torch.empty_like(out)
    like.copy_(x.sum(dim=1))
    (write or (lambda o, v: o.copy_(v)))(out, x.sum(dim=1))
    return out, flag, like

def escaped(x):
    import torch as real
    out = real.empty((int(x.shape[0]),), dtype=real.float32)
    out.copy_(x.sum(dim=1))
    return out
"""
    exec(compile(src, "fake_engine", "exec"), m.__dict__)
    return m


def _past(v, extra):
    """``v`` with ``extra`` more leading rows read from whatever follows it in memory (what a missing clamp does)."""
    shape = (v.shape[0] + extra,) + tuple(v.shape[1:])
    return v.as_strided(shape, v.stride(), v.storage_offset())


X = torch.arange(12, dtype=torch.float32).reshape(4, 3) - 20.0  # (all negative: a zero or a pattern word would win a max)


def test_halo_geometry_and_fills():
    for fill in G.FLOAT_FILLS:
        v = G.guarded(X, fill)
        assert v.shape == X.shape and v.dtype == X.dtype and v.is_contiguous() and torch.equal(v, X)
        g = v._guard
        assert g.lo >= G.HALO_BYTES and g.buf.numel() - g.lo - g.nbytes >= G.HALO_BYTES
        assert g.lo % 256 == 0 and g.buf.numel() % 256 == 0 and G.HALO_BYTES >= max(1 << 20, 256 * 1024 * 4)
        halo = _past(v, 1)[-1]
        assert torch.isnan(halo).all() if fill != fill else (halo == fill).all()
        G.check_halos(v)
    i = G.guarded(torch.tensor([3, 4, 5], dtype=torch.int32), 2)
    assert int(_past(i, 1)[-1]) == 2 and i.tolist() == [3, 4, 5]
    s = G.guarded(X, G.NAN, skew_bytes=5 * 12)  # a row slice: the payload starts a whole number of rows into its buffer
    assert s._guard.lo % 256 == 60 and torch.equal(s, X) and s.data_ptr() % 16 == (s._guard.buf.data_ptr() + 60) % 16
    with pytest.raises(TypeError):
        G.guarded(X, 1)
    with pytest.raises(ValueError):
        G.guarded(X, G.NAN, skew_bytes=2)


@pytest.mark.parametrize("fill", G.FLOAT_FILLS, ids=G.fill_id)
def test_a_correct_op_passes(fill):
    m = _fake_engine()
    ref = m.row_sums(X)[0]
    x = G.guarded(X, fill)
    with G.guarded_outputs(m) as g:
        out, flag, like = m.row_sums(x)
        assert isinstance(out, torch.Tensor) and isinstance(out, m.torch.Tensor)
    assert m.torch is torch  # restored
    assert g.count == 3 and [q.kind for q in g.guards] == ["empty", "zeros", "empty"]
    G.check_halos(x)
    assert torch.equal(out, ref) and torch.equal(like, ref) and int(flag) == 0


def test_a_write_past_the_end_is_caught():
    m = _fake_engine()
    with pytest.raises(AssertionError, match="output 0 .*back halo changed 0 bytes"):
        with G.guarded_outputs(m):
            m.row_sums(X, write=lambda o, v: _past(o, 1).copy_(torch.cat([v, v[:1]])))
    x = G.guarded(X, G.NAN)
    _past(x, 1)[-1, 0] = 1.0  # a kernel that scribbles behind an input
    with pytest.raises(AssertionError, match="back halo"):
        G.check_halos(x)


def test_a_write_before_the_start_is_caught():
    m = _fake_engine()

    def write(o, v):
        o.copy_(v)
        o.as_strided((1,), (1,), o.storage_offset() - 1).fill_(7.0)

    with pytest.raises(AssertionError, match="output 0 .*front halo changed 0 bytes"):
        with G.guarded_outputs(m):
            m.row_sums(X, write=write)


def test_a_sum_over_one_row_too_many_is_caught_by_the_nan_fill():
    x = G.guarded(X, G.NAN)
    assert torch.equal(x.sum(dim=0), X.sum(dim=0))
    wrong = _past(x, 1).sum(dim=0)
    assert not torch.equal(wrong, X.sum(dim=0)) and torch.isnan(wrong).all()
    masked = (_past(x, 1) * torch.tensor([1.0, 1.0, 1.0, 1.0, 0.0])[:, None]).sum(dim=0)  # "masked" by a multiply with 0: still caught
    assert torch.isnan(masked).all()


def test_a_max_over_one_row_too_many_needs_the_big_fill():
    """The reason for two fills: a comparison drops a NaN (v_max_f32, fmaxf and ``x > best`` all do), so only 3e38 shows the over-read."""
    want = X.max(dim=0).values
    nan_run = torch.fmax(_past(G.guarded(X, G.NAN), 1)[:-1].max(dim=0).values, _past(G.guarded(X, G.NAN), 1)[-1])
    assert torch.equal(nan_run, want)  # missed
    big_run = torch.fmax(_past(G.guarded(X, G.BIG), 1)[:-1].max(dim=0).values, _past(G.guarded(X, G.BIG), 1)[-1])
    assert not torch.equal(big_run, want) and (big_run == G.BIG).all()  # caught


def test_an_output_left_half_unwritten_is_caught():
    m = _fake_engine()
    with pytest.raises(AssertionError, match="output 0 .*2 of 4 words were never written"):
        with G.guarded_outputs(m):
            m.row_sums(X, write=lambda o, v: o[:2].copy_(v[:2]))
    with G.guarded_outputs(m, partly_written=(0,)) as g:  # ... unless the case exempts it by position (and says why)
        m.row_sums(X, write=lambda o, v: o[:2].copy_(v[:2]))
    assert g.count == 3


def test_an_output_allocated_outside_the_proxy_trips_the_count():
    m = _fake_engine()
    with G.guarded_outputs(m) as g:
        out = m.escaped(X)
    assert torch.equal(out, X.sum(dim=1))
    assert g.count == 0  # a case that expects 1 fails here
    with pytest.raises(AssertionError):
        assert g.count == 1


def test_the_engine_module_allocates_only_through_the_three_names():
    """guarded_outputs intercepts ``empty``, ``empty_like`` and ``zeros``: engine.py must not allocate any other way."""
    import os.path as osp
    import re

    src = open(osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "text2loc_amd", "engine.py")).read()
    for name in ("ones", "full", "zeros_like", "ones_like", "full_like", "empty_strided", "tensor", "arange", "rand", "randn"):
        assert not re.search(r"\btorch\.%s\(" % name, src), name
    assert not re.search(r"\.new_(empty|zeros|ones|full|tensor)\(", src)
