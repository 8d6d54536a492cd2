"""GPU half of the phased-BatchNorm block tier: the fine step's cross-rank statistics kernels through the dev library's wrapper
(t2l_blk_ft_bn_sync_fwd / _bwd: the ranks emulated as parts of the rows, the slots — NaN before the statistics launch — added up on
the device in the callback's place), every element of every output against the float64 reference of the WHOLE row set
(tests/fine_sync_blocks.py). Operands sit between NaN halos; inputs are verified unwritten. Each case prints an `FTSYNC` line
(pytest -s); the MI355X figures are in profiles/fine_train_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import fine_sync_blocks as S
from tests import fine_train_blocks as B
from tests.test_gpu_fine_train_blocks import Mat, ok, settle

pytestmark = pytest.mark.gpu

CASES = [(M, rows) for M, splits in S.SPLITS.items() for rows in splits]


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return S.load_blocks()


@pytest.mark.parametrize("M,rows", CASES, ids=["+".join(map(str, r)) for _, r in CASES])
def test_phased_batchnorm_over_parts_is_the_whole_set_batchnorm(lib, M, rows):
    """forward out, x̂, rstd, running buffers; backward dy, dγ, dβ — plain columns, |mean| = 100 std, exactly constant columns; running
    buffers and dγ / dβ given and null"""
    parts = (ctypes.c_int32 * len(rows))(*rows)
    worst = {}
    for N in S.COLS:
        for kind in S.KINDS:
            for full in (True, False):
                if not full and kind != "plain":
                    continue
                Y0, g, b, rm, rv = B.bn_case(M, N, kind)
                Y, G, Bt = Mat(Y0), Mat(g), Mat(b)
                RM, RV = (Mat(rm), Mat(rv)) if full else (None, None)
                rstd, out = Mat(np.full(N, np.nan)), Mat(np.full((M, N), np.nan))
                ok(lib, lib.t2l_blk_ft_bn_sync_fwd(Y.ptr(), parts, len(rows), N, G.ptr(), Bt.ptr(), RM.ptr() if full else None,
                                                   RV.ptr() if full else None, rstd.ptr(), out.ptr()))
                settle([G, Bt], [Y, rstd, out] + ([RM, RV] if full else []))
                ref = S.sync_fwd_ref(Y0, g, b, rm if full else None, rv if full else None)
                got = {"xhat": Y.get(), "out": out.get(), "rstd": rstd.get()[0]}
                if full:
                    got.update(rm=RM.get()[0], rv=RV.get()[0])
                assert set(got) == set(ref)
                for k in ref:
                    worst[f"fwd {k} N={N} {kind} run={int(full)}"] = B.ratio(got[k], *ref[k])
                dout, o, xh, rs, g, dg0, db0 = B.bn_bwd_case(M, N, kind)
                ins = [Mat(a) for a in (dout, o, xh, rs, g)]
                DG, DB, dy = Mat(dg0), Mat(db0), Mat(np.full((M, N), np.nan))
                ok(lib, lib.t2l_blk_ft_bn_sync_bwd(*[m.ptr() for m in ins], parts, len(rows), N, DG.ptr() if full else None,
                                                   DB.ptr() if full else None, dy.ptr()))
                settle(ins, [DG, DB, dy])
                ref = S.sync_bwd_ref(dout, o, xh, rs, g, dg0 if full else None, db0 if full else None, rows)
                got = {"dy": dy.get(), "dg": DG.get()[0], "db": DB.get()[0]}
                if not full:
                    assert DG.unwritten() and DB.unwritten()
                for k in ref:
                    worst[f"bwd {k} N={N} {kind} grads={int(full)}"] = B.ratio(got[k], *ref[k])
    for d in ("fwd", "bwd"):
        k = max((k for k in worst if k.startswith(d + " ")), key=worst.get)
        print(f"FTSYNC bn_sync_{d} rows={'+'.join(map(str, rows))} {k[4:]} {worst[k]:.4g}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_the_wrapper_refuses_before_it_launches(lib):
    p = Mat(np.zeros((16, 128))).ptr()
    one = (ctypes.c_int32 * 1)(16)
    for fn, args, msg in [
        (lib.t2l_blk_ft_bn_sync_fwd, (p, one, 1, 128, p, None, None, None, p, p), b"null"),
        (lib.t2l_blk_ft_bn_sync_fwd, (p, one, 0, 128, p, p, None, None, p, p), b"1..16 parts"),
        (lib.t2l_blk_ft_bn_sync_fwd, (p, one, 17, 128, p, p, None, None, p, p), b"1..16 parts"),
        (lib.t2l_blk_ft_bn_sync_fwd, (p, one, 1, 1025, p, p, None, None, p, p), b"N <= 1024"),
        (lib.t2l_blk_ft_bn_sync_fwd, (p, (ctypes.c_int32 * 2)(16, 0), 2, 128, p, p, None, None, p, p), b"at least one row"),
        (lib.t2l_blk_ft_bn_sync_bwd, (p, p, p, p, p, one, 1, 128, None, None, None), b"null"),
        (lib.t2l_blk_ft_bn_sync_bwd, (p, p, p, p, p, None, 1, 128, None, None, p), b"1..16 parts"),
    ]:
        assert fn(*args) == -1 and msg in lib.t2l_blk_last_error(), (fn.__name__, lib.t2l_blk_last_error())
