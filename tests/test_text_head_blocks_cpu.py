"""CPU half of the text-head block tier (tests/text_head_blocks.py; GPU half: tests/test_gpu_text_head_blocks.py).

What is proven here, without a GPU: the numpy T16 / T32 layouts round-trip and agree with the index formula element by element; a
float32 ``numpy.matmul`` of the modelled operands stays inside the derived bound in every Gaussian case (a correct
float32-accumulating kernel passes); the exact cases' float32 gather equals the float64 product of the planes; the selection
matrices pick from every k-step of every k-part; the case lists reach the job counts and k-splits the issue names; and every
mutant of the REFERENCE leaves the bound or breaks bit-equality in every case it applies to — ``SEEN_BY`` says which of the two
kinds of case sees it."""
import numpy as np
import pytest

from oracle import arith
from tests import text_head_blocks as T

ARMS = [(epi, single) for epi in range(4) for single in (0, 1)]


# ---- layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(32, 8), (64, 64), (256, 96), (288, 1024)])
def test_t16_and_t32_round_trip_and_match_the_index_formula(rows, cols):
    a = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    m, k = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    for pack, unpack, index in ((T.t16_pack, T.t16_unpack, T.t16_index), (T.t32_pack, T.t32_unpack, T.t32_index)):
        flat = pack(a)
        assert np.array_equal(unpack(flat, rows, cols), a)
        assert np.array_equal(flat[index(m, k, cols)], a)  # element (m, k) sits where the kernels' formula says
        assert sorted(index(m, k, cols).ravel().tolist()) == list(range(rows * cols))
    assert not np.array_equal(T.t16_unpack_swapped(T.t16_pack(a), rows, cols), a) or cols == 8


def test_split_and_bf16_bits_are_what_the_kernels_declare():
    v = T.gauss32(1, 4096) * np.float32(3.0)
    hi, lo = T.split_f16(v)
    assert hi.dtype == lo.dtype == np.float16 and (lo != 0).mean() > 0.9
    assert np.abs(T.join64(hi, lo) - v.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(v).max()
    h, l = arith.split_bf16(v)
    assert np.array_equal(T.bf16_values(T.bf16_bits(h)), h) and np.array_equal(T.bf16_values(T.bf16_bits(l)), l)


# ---- the case lists reach what they are for -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 96, 1024, 4096])
def test_selection_picks_from_every_k_step_in_every_n_tile(K):
    pi, sign = T.selection(768, K)
    for t in range(3):
        steps = set((pi[t * 256:(t + 1) * 256] // 16).tolist())
        assert steps == set(range(K // 16))
    assert set(sign.tolist()) == {-1.0, 1.0} and pi.max() < K
    W = T.selection_matrix(768, K)
    assert not T.split_f16(W)[1].any() and (np.abs(W).sum(axis=1) == 1).all()


@pytest.mark.parametrize("Kc,ks", [(1024, 8), (1152, 4), (256, 2), (32, 1)])
def test_selection_reaches_the_first_and_last_step_of_every_k_part(Kc, ks):
    pi, _ = T.selection(256, Kc)
    part = T.ceil_to(Kc, 64) // ks
    picked = set((pi // 16).tolist())
    for kp in range(ks):
        lo, hi = kp * part // 16, min((kp + 1) * part, Kc) // 16 - 1
        assert lo in picked and hi in picked


@pytest.mark.parametrize("epi", range(4))
def test_jobs_per_workgroup_reached(epi):
    """host-side, from the shapes: per epilogue a workgroup with >= 3 jobs (the cross-tile prefetch), one with exactly 1, and a job
    list that ends at the `break` (m_tiles % 8 != 0 with more than one round); 256 stands for the device's CU count"""
    jobs = [T.jobs_per_workgroup(c.cus or 256, c.m_tiles, c.n_tiles) for c in T.gemm_cases(epi, 0, "gauss")]
    assert any(max(j) >= 3 for j in jobs) and any(1 in j for j in jobs)
    nine = [j for c, j in zip(T.gemm_cases(epi, 0, "gauss"), jobs) if c.m_tiles == 9 and c.cus == 8]
    assert nine and nine[0][0] == 6 and nine[0][1:] == [3] * 7  # workgroups 1..7: their second m tile (9..15) does not exist
    assert all(sum(j) == c.m_tiles * c.n_tiles for c, j in zip(T.gemm_cases(epi, 0, "gauss"), jobs))


def test_fast_case_list_hits_every_k_split_and_the_ring_minimum():
    assert tuple(T.fast_ks(*s) for s in T.FAST_SHAPES) == T.FAST_KS and set(T.FAST_KS) == {1, 2, 4, 8}
    cs = T.fast_cases("gauss")
    assert {c.ks for c in cs if c.mode == "plain_acc"} == {1, 2, 4, 8}  # bias + ReLU + accumulate behind every reduction
    assert {c.Kc for c in cs if c.k_pad > c.Kc} == {32, 96, 160}
    assert all((c.k_pad // 16) // c.ks >= 4 for c in cs) and min((c.k_pad // 16) // c.ks for c in cs) == 4
    assert all(c.Mo % 4 == 0 for c in cs if c.a_trans) and {c.cus for c in cs if c.ks > 1} == {8, None}


# ---- a correct float32 kernel passes; the exact references are exact --------------------------------------------------------------
def _f32(a):
    return np.asarray(a).astype(np.float32)


@pytest.mark.parametrize("epi,single", ARMS)
def test_float32_matmul_stays_inside_the_gemm_bound(epi, single):
    for c in T.gemm_cases(epi, single, "gauss"):
        ref, tol = T.gemm_model(c)
        acc = _f32(c.xh) @ _f32(c.wh).T
        if not single:
            acc = acc + _f32(c.xh) @ _f32(c.wl).T + _f32(c.xl) @ _f32(c.wh).T
        v = acc + c.bias
        if epi == T.EPI_RESID:
            v = v + (_f32(c.rh) + _f32(c.rl))
        if epi == T.EPI_RELU16 or (epi == T.EPI_ROW and c.relu):
            v = np.maximum(v, np.float32(0))
        if epi == T.EPI_ROW:
            v = v[:, :c.n_real] + (c.C0 if c.acc else np.float32(0))
        r = np.abs(v.astype(np.float64) - ref) / tol
        assert r.max() <= 1.0, (c.name, r.max())


def test_float32_matmul_stays_inside_the_fast_gemm_bound():
    for c in T.fast_cases("gauss"):
        ref, tol = T.fast_model(c)
        f = lambda x: np.asarray(x).astype(np.float32)
        if c.single:
            acc = f(arith.bf16_rne(c.A2)) @ f(arith.bf16_rne(c.B2))
        else:
            (ah, al), (bh, bl) = arith.split_bf16(c.A2), arith.split_bf16(c.B2)
            acc = f(ah) @ f(bh) + f(ah) @ f(bl) + f(al) @ f(bh)
        v = acc + (c.bias if c.has_bias else np.float32(0))
        if c.relu:
            v = np.maximum(v, np.float32(0))
        if c.acc:
            v = v + c.C0
        r = np.abs(v.astype(np.float64) - ref) / tol
        assert r.max() <= 1.0, (c.name, r.max())


@pytest.mark.parametrize("epi,single", ARMS)
def test_exact_gemm_reference_is_the_float64_product(epi, single):
    for c in T.gemm_cases(epi, single, "exact"):
        if c.M > 300:
            continue
        pi, sign = T.selection(c.N, c.K)
        gather = (_f32(c.xh)[:, pi] + (0 if single else _f32(c.xl)[:, pi])) * _f32(sign)
        assert np.array_equal(gather.astype(np.float64), T.gemm_product64(c)), c.name
        ref, tol = T.gemm_model(c)  # and the float32 epilogue stays within the Gaussian bound's form of the float64 one
        assert (np.abs(T.gemm_exact32(c).astype(np.float64) - ref) <= tol + 4 * T.U * np.abs(ref)).all(), c.name


def test_exact_fast_reference_is_the_float64_product():
    for c in T.fast_cases("exact"):
        hi, lo = arith.split_bf16(c.A2)
        assert not arith.split_bf16(c.B2)[1].any()
        pi, sign = T.selection(c.No, c.Kc)
        gather = (_f32(hi)[:, pi] + (0 if c.single else _f32(lo)[:, pi])) * _f32(sign)
        assert np.array_equal(gather.astype(np.float64), arith.product(c.A2.astype(np.float64), c.B2.astype(np.float64), c.ar)), c.name


# ---- mutants of the reference ---------------------------------------------------------------------------------------------------
# which kind of case sees the mutant in EVERY case it applies to ("either": each case is seen by at least one of the two)
SEEN_BY = {
    "drop_last_kstep": "both",   # 16 of K terms are gone: far outside any bound, and the exact case picks from the last k-step
    "no_lohi": "exact",          # a 2^-12 relative term: invisible to a 3 K-rounding bound at K = 1024, a whole plane to ==
    "resid_no_lo": "exact",      # the same for the residual's lo plane
    "t16_swapped": "both",
    "quad_shift": "both",
    "bias_per_part": "both",     # fast_gemm with ks > 1 and a bias
    "relu_per_slab": "gauss",    # fast_gemm with ks > 1 and ReLU (the exact case's slabs but one are zero: not modelled there)
}


def _seen(model, exact32, cg, ce, mut):
    ref, tol = model(cg)
    got, _ = model(cg, mut)
    g = bool((np.abs(got - ref) > tol).any())
    e = None if exact32 is None else not np.array_equal(exact32(ce, mut), exact32(ce))
    return g, e


def _hold(mut, g, e, name):
    want = SEEN_BY[mut]
    if want in ("both", "gauss"):
        assert g, (mut, name, "the Gaussian bound does not see it")
    if want in ("both", "exact"):
        assert e, (mut, name, "bit-equality does not see it")
    assert g or e


@pytest.mark.parametrize("mut", ["drop_last_kstep", "no_lohi", "resid_no_lo", "t16_swapped", "quad_shift"])
@pytest.mark.parametrize("epi,single", ARMS)
def test_gemm_reference_mutants_are_seen(epi, single, mut):
    applies = not ((mut == "no_lohi" and single) or (mut == "resid_no_lo" and epi != T.EPI_RESID))
    n = 0
    for cg, ce in zip(T.gemm_cases(epi, single, "gauss"), T.gemm_cases(epi, single, "exact")):
        if not applies or cg.M > 300 or (mut == "quad_shift" and cg.n_real < 16):  # (the 9-tile shapes repeat the 2-tile ones' operands' form)
            continue
        g, e = _seen(T.gemm_model, T.gemm_exact32, cg, ce, mut)
        _hold(mut, g, e, cg.name)
        n += 1
    assert n >= 4 or not applies


@pytest.mark.parametrize("mut", ["drop_last_kstep", "no_lohi", "quad_shift", "bias_per_part", "relu_per_slab"])
def test_fast_gemm_reference_mutants_are_seen(mut):
    n = 0
    for cg, ce in zip(T.fast_cases("gauss"), T.fast_cases("exact")):
        if mut == "no_lohi" and cg.single:
            continue
        if mut == "bias_per_part" and not (cg.ks > 1 and cg.has_bias):
            continue
        if mut == "relu_per_slab" and not (cg.ks > 1 and cg.relu):
            continue
        g, e = _seen(T.fast_model, None if mut == "relu_per_slab" else T.fast_exact32, cg, ce, mut)
        _hold(mut, g, e, cg.name)
        n += 1
    assert n >= 4


# ---- layer references -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", T.ATTN_L)
def test_attention_reference_is_a_softmax_and_stays_in_the_logit_range(L):
    n_sent = T.attn_sentences(L)
    qkv = T.gauss32((T.SEED, 3, L), n_sent * L, 3 * T.DM).astype(np.float64)
    o, tol, zmin = T.attn_reference(qkv, n_sent, L)
    assert zmin >= -T.FB.LOGIT_RANGE and (tol > 0).all() and tol.max() < 1e-2
    if L == 1:  # one key: the output is the value row
        assert np.allclose(o, qkv[:, 2 * T.DM:], rtol=0, atol=1e-15)
    G = 32 // L
    assert n_sent % G != 0 or G == 1  # the last group is partial
    # float32 run of the same function: a correct float32 kernel passes
    q32 = qkv.astype(np.float32).reshape(n_sent, L, 3, T.HEADS, T.HD)
    s = np.einsum("slhd,smhd->shlm", q32[:, :, 0], q32[:, :, 1]) * np.float32(1 / 16)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    o32 = np.einsum("shlm,smhd->slhd", p, q32[:, :, 2]).reshape(n_sent * L, T.DM)
    assert (np.abs(o32.astype(np.float64) - o) <= tol).all()


@pytest.mark.parametrize("L", T.POOL_L)
def test_pool_fixture_reaches_negative_maxima_and_mixed_partial_signs(L):
    n_sent = 96 // L + 2
    M = n_sent * L
    gamma, beta = T.pool_params(L)
    rows, tol = T.ln_reference(T.ln_input(M, L), gamma, beta)
    pooled = T.pool_reference(rows, n_sent, L)
    assert (pooled < 0).any() and (pooled > 0).any() and tol < 1e-3
    if L in (5, 13, 17):  # a sentence that straddles two 32-row tiles, with partial maxima of different sign in some column
        mixed = False
        for s in range(n_sent):
            a, b = s * L, (s + 1) * L
            cut = (a // 32 + 1) * 32
            if cut < b:
                p0, p1 = rows[a:cut].max(axis=0), rows[cut:b].max(axis=0)
                mixed = mixed or bool(((p0 < 0) != (p1 < 0)).any())
        assert mixed
