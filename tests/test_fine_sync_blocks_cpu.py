"""CPU half of the phased-BatchNorm block tier (tests/fine_sync_blocks.py): the references and bounds hold without the library — the
kernels' arithmetic restated in numpy (float64 sums per part, the exchange, float32 apply) stays inside the bound of the WHOLE row set
for every split, the derived one-pass terms stay a small share of the bounds they are added to, and the mutants a wrong kernel would
be (no exchange, a local row count, float32 one-pass sums, gradients from the first part only) leave it."""
import numpy as np
import pytest

from tests import fine_sync_blocks as S
from tests import fine_train_blocks as B

CASES = [(M, rows, N, kind) for M, splits in S.SPLITS.items() for rows in splits for N in S.COLS for kind in S.KINDS]


def worst(got, ref):
    return max(B.ratio(got[k], *ref[k]) for k in ref)


@pytest.mark.parametrize("M,rows,N,kind", CASES)
def test_the_restated_kernels_stay_inside_the_whole_set_bound(M, rows, N, kind):
    assert sum(rows) == M
    Y, g, b, rm, rv = B.bn_case(M, N, kind)
    ref = S.sync_fwd_ref(Y, g, b, rm, rv)
    got = S.phased_fwd(Y, rows, g, b, rm, rv)
    assert set(got) == set(ref) == {"xhat", "out", "rstd", "rm", "rv"}
    assert worst(got, ref) <= 1.0
    base, add = B.bn_fwd_ref(Y, g, b, rm, rv), S.onepass_terms(Y, g, rv)
    for k, a in add.items():
        assert np.all(a <= S.ONEPASS_SHARE * base[k][1]), k
    dout, o, xh, rs, g, dg0, db0 = B.bn_bwd_case(M, N, kind)
    ref = S.sync_bwd_ref(dout, o, xh, rs, g, dg0, db0, rows)
    got = S.phased_bwd(dout, o, xh, rs, g, dg0, db0, rows)
    assert set(got) == set(ref) == {"dy", "dg", "db"}
    assert worst(got, ref) <= 1.0
    if len(rows) == 1:  # one part: the gradient bound is inside the one-launch kernel's
        one = B.bn_bwd_ref(dout, o, xh, rs, g, dg0, db0)
        assert np.all(ref["dg"][1] <= one["dg"][1] * (1 + 1e-12)) and np.all(ref["db"][1] <= one["db"][1] * (1 + 1e-12))


@pytest.mark.parametrize("rows", [(64, 64), (127, 1), (3, 1, 124)])
def test_the_bounds_catch_what_a_wrong_kernel_would_do(rows):
    M, N = 128, 128
    Y, g, b, rm, rv = B.bn_case(M, N, "plain")
    ref = S.sync_fwd_ref(Y, g, b, rm, rv)
    for mut in ("no_exchange", "local_count"):
        assert worst(S.phased_fwd(Y, rows, g, b, rm, rv, mut), ref) > 10.0, mut
    dout, o, xh, rs, g2, dg0, db0 = B.bn_bwd_case(M, N, "plain")
    bref = S.sync_bwd_ref(dout, o, xh, rs, g2, dg0, db0, rows)
    for mut in ("no_exchange", "first_part_grads"):
        assert worst(S.phased_bwd(dout, o, xh, rs, g2, dg0, db0, rows, mut), bref) > 10.0, mut
    Yo, g, b, rm, rv = B.bn_case(M, N, "offset")  # |mean| = 100 std: E[y²] - mean² in float32 loses the variance
    assert worst(S.phased_fwd(Yo, rows, g, b, rm, rv, "f32_sums"), S.sync_fwd_ref(Yo, g, b, rm, rv)) > 10.0


def test_constant_columns_normalise_to_zero_whatever_the_split():
    for rows in S.SPLITS[128]:
        Y, g, b, rm, rv = B.bn_case(128, 64, "constant")
        got = S.phased_fwd(Y, rows, g, b, rm, rv)
        assert not np.any(got["xhat"][:, ::2])
        assert np.allclose(got["rstd"][::2], 1.0 / np.sqrt(np.float32(B.BN_EPS)), rtol=1e-6)
