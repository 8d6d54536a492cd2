"""CPU tier of the training-block tests: the bars of tests/train_blocks.py tell right from wrong before a GPU is
involved. For every product case of the GPU tier a float32 numpy.matmul of the modelled operands stays inside ``tol`` everywhere, and
every mutant of the reference — the ways a tile kernel goes subtly wrong — leaves ``tol`` on at least one element. The wrappers'
contract refusals need the dev library and no GPU."""
import ctypes

import numpy as np
import pytest

from oracle import arith
from tests import train_blocks as TB

KINDS = ("nt", "nn", "tn")


def _cases(kind, rows=TB.ROWS):
    """every product case of the GPU tier: the launchers' widths, and the multi-job kernels' own (each job is such a product)"""
    for M in rows:
        for N, Kp in TB.WIDTHS + TB.MULTI_WIDTHS[:1]:
            yield TB.product_case(kind, M, N, Kp)


def _extras(c):
    """(bias, C0) as the launcher of this kind adds them."""
    return (c.b if c.kind == "nt" else None), (None if c.kind == "nt" else c.C0)


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("kind", KINDS)
def test_float32_restatement_is_accepted(kind, ar):
    worst = 0.0
    for c in _cases(kind):
        bias, C0 = _extras(c)
        ref, tol = TB.linear(c.A, c.B, ar, bias=bias, C0=C0, base=c.base(ar))
        got = TB.f32_matmul(c.A, c.B, ar).astype(np.float32)
        if bias is not None:
            got = got + bias.astype(np.float32)
        if C0 is not None:
            got = got + C0.astype(np.float32)
        ratio = float((np.abs(got.astype(np.float64) - ref) / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{kind} M={c.M} N={c.N} Kp={c.Kp} arith {ar}: float32 matmul at {ratio:.3f} of tol"
    print(f"{kind} arith {ar}: float32 restatement worst err / tol {worst:.4f}")


def test_float32_colsum_is_accepted():
    for c in _cases("tn"):
        ref, tol = TB.colsum(c.dY, c.db0)
        got = c.db0.astype(np.float32) + c.dY.astype(np.float32).sum(axis=0, dtype=np.float32)
        assert (np.abs(got.astype(np.float64) - ref) <= tol).all()


def _rejected(c, ar, mutant, ref, tol, what):
    assert mutant.shape == ref.shape
    assert (np.abs(mutant - ref) > tol).any(), f"{what}: {c.kind} M={c.M} N={c.N} Kp={c.Kp} arith {ar} passes the bar"


@pytest.mark.parametrize("kind", KINDS)
def test_mutant_bf16_by_truncation(kind):
    for c in _cases(kind):
        ref, tol = TB.linear(c.A, c.B, arith.BF16, base=c.base(arith.BF16))
        _rejected(c, arith.BF16, arith.product(c.A, c.B, arith.BF16_TRUNC), ref, tol, "bf16 by truncation")


@pytest.mark.parametrize("kind", KINDS)
def test_mutant_split_without_lo_hi(kind):
    for c in _cases(kind):
        ref, tol = TB.linear(c.A, c.B, arith.SPLIT, base=c.base(arith.SPLIT))
        _rejected(c, arith.SPLIT, arith.product(c.A, c.B, arith.SPLIT_NO_LOHI), ref, tol, "split-bf16 without lo * hi")


def _chunk_starts(c):
    """first reduction index of the last z-chunk, for each blocking the launcher may choose (one chunk: index 0)"""
    if c.kind != "tn":
        return {0}
    blks = [32] + ([64] if c.N % 64 == 0 and c.Kp % 64 == 0 else [])
    out = set()
    for blk in blks:
        ksplit, kchunk = TB.tn_split(c.M, c.N, c.Kp, blk)
        out.add((ksplit - 1) * kchunk)
    return out


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("kind", KINDS)
def test_mutant_one_reduction_index_dropped(kind, ar):
    for c in _cases(kind):
        bias, C0 = _extras(c)
        ref, tol = TB.linear(c.A, c.B, ar, bias=bias, C0=C0, base=c.base(ar))
        for k in sorted({c.K - 1} | _chunk_starts(c)):
            assert 0 <= k < c.K
            _rejected(c, ar, ref - arith.product(c.A[:, k:k + 1], c.B[k:k + 1, :], ar), ref, tol, f"reduction index {k} dropped")


def test_tn_split_matches_the_issue_shapes():
    assert TB.tn_split(257, 32, 96, 32) == (2, 192)  # second chunk: 65 rows — three waves busy, one idle
    assert TB.tn_split(600, 256, 256, 32)[0] == 3 and TB.tn_split(600, 768, 256, 64)[0] == 3
    assert TB.tn_split(140, 256, 256, 32)[0] == 1


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("kind", KINDS)
def test_mutant_last_32_columns_from_half_the_rows(kind, ar):
    for c in _cases(kind):
        ref, tol = TB.linear(c.A, c.B, ar, base=c.base(ar))
        h = c.K // 2
        mutant = ref.copy()
        mutant[:, -32:] = arith.product(c.A[:, :h], c.B[:h, -32:], ar)
        _rejected(c, ar, mutant, ref, tol, "last 32 columns from half the reduction")


@pytest.mark.parametrize("ar", TB.ARITHS)
def test_mutant_dropout_index_transposed(ar):
    for c in _cases("nt"):  # epi == 1: C2 = dropout(C)
        ref, tol = TB.linear(c.A, c.B, ar, bias=c.b, relu=True, base=c.base(ar))
        good = TB.masked_dropped(ref, tol, TB.drop_factor(TB.SEED, 2, TB.P_DROP, ref.shape))
        bad = TB.masked_dropped(ref, tol, TB.drop_factor(TB.SEED, 2, TB.P_DROP, ref.shape, transposed=True))
        _rejected(c, ar, bad[0], good[0], good[1], "dropout bit at col * ldc + row (epi 1)")
    for c in _cases("nn"):  # epi == 2: mask, then dropout
        ref, tol = TB.linear(c.A, c.B, ar, base=c.base(ar))
        good = TB.masked_dropped(ref, tol, TB.drop_factor(TB.SEED, 2, TB.P_DROP, ref.shape), c.mask_src)
        bad = TB.masked_dropped(ref, tol, TB.drop_factor(TB.SEED, 2, TB.P_DROP, ref.shape, transposed=True), c.mask_src)
        _rejected(c, ar, bad[0], good[0], good[1], "dropout bit at col * ldc + row (epi 2)")


@pytest.mark.parametrize("ar", TB.ARITHS)
def test_mutant_bias_added_in_every_z_chunk(ar):
    """No launcher of the step gives a split product a bias, so the kernel's `bz == 0` is only visible to a reference that does: the
    split shapes of gemm_tn with a per-column bias."""
    for c in _cases("tn", rows=(257, 600)):
        bias = TB.gauss((TB.SEED, 9, c.M, c.N, c.Kp), c.Kp)
        ref, tol = TB.linear(c.A, c.B, ar, bias=bias, C0=c.C0, base=c.base(ar))
        ksplit, _ = TB.tn_split(c.M, c.N, c.Kp, 32)
        assert ksplit > 1
        _rejected(c, ar, ref + (ksplit - 1) * bias, ref, tol, "bias added in every z-chunk")


def test_layer_references_agree_with_their_float32_runs():
    """the layer tier's bound is built on e32: it must be small (the float32 restatement IS the same function) and never zero-width"""
    B, S, HD = 3, 17, 64
    qkv = TB.gauss((TB.SEED, 20), B * S, 12 * HD)
    fac = TB.drop_factor(TB.SEED, 0, TB.P_DROP, (B, 4, S, S))
    for ref, tol in TB.layer_tol(TB.attn_fwd, qkv, B, S, HD, fac):
        assert 0 < tol < 1e-4 * max(1.0, float(np.abs(ref).max()))
    x, y, g, b = (TB.gauss((TB.SEED, 21, k), *s) for k, s in enumerate(((5, 256), (5, 256), (256,), (256,))))
    for ref, tol in TB.layer_tol(TB.ln_fwd, x, y, g, b, TB.drop_factor(TB.SEED, 1, TB.P_DROP, (5, 256))):
        assert 0 < tol < 1e-4 * max(1.0, float(np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------------------------------------
# contract refusals of the dev library: shapes outside a kernel's documented contract are refused BEFORE any launch (null
# pointers throughout: a wrapper that got as far as a launch would not return -1)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks():
    return TB.load_blocks()


def test_wrappers_refuse_shapes_outside_the_contract(blocks):
    L = blocks
    n = None
    refused = [
        # N not a multiple of 32
        (L.t2l_blk_gemm_nt(n, n, n, n, n, 64, 48, 64, 0, 0, 0, 0, 1, 0, 0.0), "multiple of 32"),
        (L.t2l_blk_gemm_nn(n, n, n, 64, 64, 40, 0, 0, 0), "multiple of 32"),
        (L.t2l_blk_gemm_tn(n, n, n, n, 64, 64, 72, 0, 0), "multiple of 32"),
        (L.t2l_blk_gemm_nt_multi(2, n, n, n, n, 64, 100, 64, 0), "multiple of 32"),
        # M not a multiple of 32 when !A_KC (the dW product's output rows are the N of dY)
        (L.t2l_blk_gemm_tn(n, n, n, n, 64, 48, 64, 0, 0), "multiple of 32"),
        (L.t2l_blk_gemm_tn_nn(n, n, n, n, n, n, 64, 16, 64, 0, n, 0, 0, 1, 0, 0.0), "multiple of 32"),
        (L.t2l_blk_gemm_tn_nn_multi(3, n, n, n, n, n, n, 64, 250, 64, 0), "multiple of 32"),
        # a k-contiguous operand with K not a multiple of 16
        (L.t2l_blk_gemm_nt(n, n, n, n, n, 64, 64, 72, 0, 0, 0, 0, 1, 0, 0.0), "multiple of 16"),
        (L.t2l_blk_gemm_nt(n, n, n, n, n, 64, 64, 3, 0, 0, 1, 1, 1, 0, 0.0), "multiple of 16"),
        (L.t2l_blk_gemm_nn(n, n, n, 64, 24, 64, 0, 2, 0), "multiple of 16"),
        (L.t2l_blk_gemm_nt_multi(1, n, n, n, n, 64, 256, 60, 0), "multiple of 16"),
        # S > 32
        (L.t2l_blk_attn_fwd(n, n, n, 1, 33, 64, 1, 0, 0.0), "S > 32"),
        (L.t2l_blk_attn_bwd(n, n, n, n, 1, 40, 256, 1, 0, 0.0), "S > 32"),
        (L.t2l_blk_seq_max_fwd(n, n, 2, 33, 256, n, n), "S > 32"),
        (L.t2l_blk_seq_max_bwd(n, n, 2, 64, 1024, n), "S > 32"),
        # instances the step does not build, empty problems, options out of range
        (L.t2l_blk_attn_fwd(n, n, n, 1, 8, 128, 1, 0, 0.0), "head dim"),
        (L.t2l_blk_ln_fwd(n, n, 4, 512, n, n, n, n, n, 1, 0, 0.0), "D 128, 256 or 1024"),
        (L.t2l_blk_ln_bwd(n, n, n, 4, 1024, 16, n, n, n, n, n, 1, 0, 0.0), "(D, waves)"),
        (L.t2l_blk_ln_bwd(n, n, n, 0, 256, 16, n, n, n, n, n, 1, 0, 0.0), "T >= 1"),
        (L.t2l_blk_pool_norm_fwd(n, n, n, n, n, 0), "at least one cell"),
        (L.t2l_blk_gemm_nt(n, n, n, n, n, 64, 64, 64, 0, 0, 3, 0, 1, 0, 0.0), "arith"),
        (L.t2l_blk_gemm_nt(n, n, n, n, n, 64, 64, 64, 0, 1, 0, 0, 1, 0, 1.0), "p in"),
    ]
    # (each call's message is overwritten by the next: check the codes here, the messages one call at a time below)
    assert [rc for rc, _ in refused] == [-1] * len(refused)
    assert L.t2l_blk_gemm_nn(n, n, n, 64, 24, 64, 0, 2, 0) == -1 and b"multiple of 16" in L.t2l_blk_last_error()
    assert L.t2l_blk_attn_fwd(n, n, n, 1, 33, 64, 1, 0, 0.0) == -1 and b"S > 32" in L.t2l_blk_last_error()
    assert L.t2l_blk_gemm_tn(n, n, n, n, 64, 48, 64, 0, 0) == -1 and b"multiple of 32" in L.t2l_blk_last_error()


def test_row_kernel_wrappers_name_the_reason_they_refuse(blocks):
    """LayerNorm at the widths the steps build (128, 256, 1024), F.normalize at 128 and 256, the element-wise dropout pair: every
    refusal is -1 with its reason, before any launch"""
    L = blocks
    n = None
    x = ctypes.c_void_p(256)  # a non-null pointer that is never followed: the shape checks come first

    def refused(rc, reason):
        assert rc == -1 and reason in L.t2l_blk_last_error(), (rc, reason, L.t2l_blk_last_error())

    for D in (0, 64, 192, 512, 2048):
        refused(L.t2l_blk_ln_fwd(x, x, 4, D, x, x, x, x, x, 1, 0, 0.0), b"D 128, 256 or 1024")
        refused(L.t2l_blk_ln_bwd(x, x, x, 4, D, 4, x, x, x, x, x, 1, 0, 0.0), b"(D, waves)")
    for D, waves in ((128, 16), (1024, 16), (256, 8), (128, 0)):
        refused(L.t2l_blk_ln_bwd(x, x, x, 4, D, waves, x, x, x, x, x, 1, 0, 0.0), b"(D, waves)")
    for D in (128, 256, 1024):
        refused(L.t2l_blk_ln_fwd(x, x, 0, D, x, x, x, x, x, 1, 0, 0.0), b"T >= 1")
        refused(L.t2l_blk_ln_bwd(x, x, x, -1, D, 4, x, x, x, x, x, 1, 0, 0.0), b"T >= 1")
        for p in (-0.1, 1.0, float("nan")):
            refused(L.t2l_blk_ln_fwd(x, x, 4, D, x, x, x, x, x, 1, 0, p), b"p must be in [0, 1)")
            refused(L.t2l_blk_ln_bwd(x, x, x, 4, D, 4, x, x, x, x, x, 1, 0, p), b"p must be in [0, 1)")
        refused(L.t2l_blk_ln_fwd(n, n, 4, D, n, n, n, n, n, 1, 0, 0.0), b"null pointer")
        refused(L.t2l_blk_ln_bwd(n, n, n, 4, D, 4, n, n, n, n, n, 1, 0, 0.0), b"null pointer")
    for D in (0, 64, 192, 512, 1024):
        refused(L.t2l_blk_rownorm_fwd(x, 4, D, x, 1024, x), b"D must be 128 or 256")
        refused(L.t2l_blk_rownorm_bwd(x, x, 1024, x, 4, D, x), b"D must be 128 or 256")
    for D in (128, 256):
        for M in (0, -3):
            refused(L.t2l_blk_rownorm_fwd(x, M, D, x, D, x), b"M >= 1")
            refused(L.t2l_blk_rownorm_bwd(x, x, D, x, M, D, x), b"M >= 1")
        for ld in (D - 1, 0, -D):
            refused(L.t2l_blk_rownorm_fwd(x, 4, D, x, ld, x), b"ld < D")
            refused(L.t2l_blk_rownorm_bwd(x, x, ld, x, 4, D, x), b"ld < D")
        for args in ((n, 4, D, x, D, x), (x, 4, D, n, D, x), (x, 4, D, x, D, n)):
            refused(L.t2l_blk_rownorm_fwd(*args), b"null pointer")
        for args in ((n, x, D, x, 4, D, x), (x, n, D, x, 4, D, x), (x, x, D, n, 4, D, x), (x, x, D, x, 4, D, n)):
            refused(L.t2l_blk_rownorm_bwd(*args), b"null pointer")
    for cnt in (0, -1):
        refused(L.t2l_blk_drop_fwd(x, cnt, x, 1, 0, 0.1), b"n >= 1")
        refused(L.t2l_blk_relu_drop_bwd(x, x, cnt, 1, 0, 0.1), b"n >= 1")
    for p in (-0.1, 1.0, float("nan")):
        refused(L.t2l_blk_drop_fwd(x, 8, x, 1, 0, p), b"p must be in [0, 1)")
        refused(L.t2l_blk_relu_drop_bwd(x, x, 8, 1, 0, p), b"p must be in [0, 1)")
    refused(L.t2l_blk_drop_fwd(n, 8, x, 1, 0, 0.1), b"null pointer")
    refused(L.t2l_blk_drop_fwd(x, 8, n, 1, 0, 0.1), b"null pointer")
    refused(L.t2l_blk_relu_drop_bwd(n, x, 8, 1, 0, 0.1), b"null pointer")
    refused(L.t2l_blk_relu_drop_bwd(x, n, 8, 1, 0, 0.1), b"null pointer")


def test_wrappers_refuse_null_pointers_at_legal_shapes(blocks):
    L = blocks
    n = None
    assert L.t2l_blk_gemm_nt(n, n, n, n, n, 33, 64, 128, 0, 0, 0, 0, 1, 0, 0.0) == -1
    assert b"null pointer" in L.t2l_blk_last_error()
    assert L.t2l_blk_gemm_nn(n, n, n, 33, 64, 128, 0, 0, 0) == -1
    assert L.t2l_blk_gemm_tn(n, n, n, n, 33, 64, 128, 0, 0) == -1
    assert L.t2l_blk_gemm_tn_nn(n, n, n, n, n, n, 33, 64, 128, 0, n, 0, 0, 1, 0, 0.0) == -1
    assert L.t2l_blk_gemm_nt_multi(2, n, n, n, n, 33, 256, 64, 0) == -1
    assert L.t2l_blk_gemm_tn_nn_multi(2, n, n, n, n, n, n, 33, 256, 64, 0) == -1
    assert L.t2l_blk_attn_fwd(n, n, n, 1, 28, 64, 1, 0, 0.0) == -1
    assert L.t2l_blk_attn_bwd(n, n, n, n, 1, 9, 256, 1, 0, 0.0) == -1
    assert L.t2l_blk_ln_fwd(n, n, 5, 256, n, n, n, n, n, 1, 0, 0.0) == -1
    assert L.t2l_blk_ln_bwd(n, n, n, 5, 256, 16, n, n, n, n, n, 1, 0, 0.0) == -1
    assert L.t2l_blk_pool_norm_fwd(n, n, n, n, n, 1) == -1
    assert L.t2l_blk_pool_norm_bwd(n, n, n, n, n, 1) == -1
    assert L.t2l_blk_seq_max_fwd(n, n, 2, 6, 256, n, n) == -1
    assert L.t2l_blk_seq_max_bwd(n, n, 2, 6, 256, n) == -1
    assert b"null pointer" in L.t2l_blk_last_error()
