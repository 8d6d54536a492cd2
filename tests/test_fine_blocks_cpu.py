"""CPU tier of the fine-match block tests: proves the float64 references, the derived bounds and the fixtures of
tests/fine_blocks.py before a GPU sees them (tests/test_gpu_fine_blocks.py; profiles/fine_blocks.md).

* ``cross_match64`` reproduces the reference's own runs (the goldens) and the float32 oracle;
* the tiled, group-masked reference equals the per-pair one EXACTLY;
* mutants: each fault, applied to the reference of the stage it lives in, against the unmutated reference at that stage's f32 and
  split bounds. ASSERTED mutants must exceed the bound (err / tol > 1) on this file's fixture (seeded weights of tests/fine_blocks.py,
  four pairs of seed 1 without junk rows; the GPU tier runs the same weights on other seeds, with junk rows) or, for the dropped lo
  plane, on ``FB.lo_fixture``, which the GPU tier runs too; the ones no bound of this tier sees are listed in NOT_ASSERTED with their
  figures and only reported — no test holds them."""
import functools

import numpy as np
import pytest

from oracle import t2l_oracle_fine as OF
from tests import fine_blocks as FB
from text2loc_amd import synth

F32 = np.float32


def float32_tol(n_layers):
    """An ESTIMATE, not a bound, of what a float32 evaluation of CrossMatch differs by from float64 through float32 round-off: a pair
    passes through max(1, 2 n_layers) decoder passes, a pass is 10 rounded operations in sequence (in-projection, logits, softmax, P V,
    out-projection, LayerNorm, twice; the two feed-forward products and the last LayerNorm), each taken to perturb its O(1) output by
    sqrt(K) u (K = 128 terms, random-walk growth) — the LayerNorms renormalise, so the perturbations are added up, not multiplied.
    (The derived worst-case bound of the whole match, FB.cross_match_bound, saturates and cannot serve here; a structural mistake in
    cross_match64 moves the offsets by 1e-3 and more, the figures measured against the goldens and the oracle are 1e-7 to 2e-7.)"""
    return max(1, 2 * n_layers) * 10 * np.sqrt(128.0) * FB.U


@pytest.mark.parametrize("name,n_layers", [("fine_embed", 2), ("fine_pn", 2), ("fine_embed_l0", 0)])
def test_cross_match64_reproduces_the_reference_runs(golden, name, n_layers):
    g = golden(name)
    sd = synth.make_fine_weights(int(g["weight_seed"]), num_layers=n_layers)
    off = FB.cross_match64(g["object_encodings"], g["hint_encodings"], sd, n_layers)
    err = float(np.abs(off - g["offsets_out"]).max())
    assert err < float32_tol(n_layers), (err, float32_tol(n_layers))


@pytest.mark.parametrize("n_layers", [0, 1, 2])
def test_cross_match64_agrees_with_the_float32_oracle(n_layers):
    sd = FB.weights(n_layers)
    for n_hints in (1, 6):
        o, h = FB.pairs(5, n_hints, 10 + n_hints)
        err = float(np.abs(FB.cross_match64(o, h, sd, n_layers) - OF.cross_match(o, h, sd, n_layers=n_layers)).max())
        assert 0 < err < float32_tol(n_layers), (n_hints, err)


def per_pair_hints(o, h, sd, n_layers):
    out = []
    for d0, d1 in zip(o.astype(np.float64), h.astype(np.float64)):
        if n_layers == 0:
            d1 = FB.decoder_layer(d1, d0, sd, "cross_hints")
        for i in range(n_layers):
            d0 = FB.decoder_layer(d0, d1, sd, f"cross_objects.{i}")
            d1 = FB.decoder_layer(d1, d0, sd, f"cross_hints.{i}")
        out.append(d1)
    return np.stack(out)


@pytest.mark.parametrize("n_hints", [1, 5, 6, 8])
def test_the_tiled_reference_equals_the_per_pair_reference_exactly(n_hints):
    """four pairs (two in each object tile, the hint tile attending both) through every pass of a two-layer model and through the
    single cross_hints layer: the same bits as pair by pair without tiles, masks or neighbours"""
    for n_layers in (2, 0):
        sd = FB.weights(n_layers)
        o, h = FB.pairs(4, n_hints, 20 + n_hints)
        off, _, tile, _ = FB.workgroup_b(o, h, sd, n_layers, "f32")
        want = per_pair_hints(o, h, sd, n_layers)
        assert np.array_equal(tile.reshape(4, 8, 128)[:, :n_hints], want), (n_layers, n_hints)
        assert np.array_equal(off, FB.cross_match64(o, h, sd, n_layers))
    o3, h3 = o[:3], h[:3]  # a tail workgroup duplicates its last pair
    off3 = FB.workgroup_b(o3, h3, sd, 0, "f32")[0]
    assert np.array_equal(off3[:3], off[:3]) and np.array_equal(off3[3], off3[2])


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
N_HINTS = 5
ARMS2 = ("f32", "split")
ASSERTED = ("mask_le", "neighbour", "head_cols", "shared_zero", "drop_lo", "sa_for_ca", "ffn_bias", "max_all8")
# what no bound of this tier sees (figures: profiles/fine_blocks.md, the mutant table); drop_lo_q: the lo plane dropped from the QUERY
# projection's operand, behind the softmax
NOT_ASSERTED = ("shared_resplit", "drop_lo_q", "ln_onepass")


@functools.lru_cache(maxsize=None)
def fixture(big_mean=False):
    sd = FB.weights(2)
    o, h = FB.pairs(4, N_HINTS, 1, big_mean=big_mean)
    A, B, H = [t.astype(np.float64) for t in FB.tiles_of(o, h, N_HINTS)]
    return sd, A, B, H


Z = np.zeros((32, 128))


def attention_mutant(mut, arm):
    """attention block alone. mask_le / neighbour: object tile B over the hint tile; the rest: the hint tile over both object tiles"""
    sd, A, B, H = fixture()
    if mut == "drop_lo":  # object tile B over a one-row hint tile (p = 1, o = v), the hint rows lo-aligned
        _, B, H = [t.astype(np.float64) for t in FB.lo_fixture(sd)]
        g = FB._get(sd, "cross_objects.0")
        args = (B, Z, [(H, Z)], FB.GB, [FB.ghint(1)], g(".multihead_attn.in_proj_weight"), g(".multihead_attn.in_proj_bias"), arm, False)
    elif mut in ("mask_le", "neighbour"):
        g = FB._get(sd, "cross_objects.0")
        args = (B, Z, [(H, Z)], FB.GB, [FB.ghint(N_HINTS)], g(".multihead_attn.in_proj_weight"), g(".multihead_attn.in_proj_bias"), arm, False)
    else:
        g = FB._get(sd, "cross_hints.0")
        args = (H, Z, [(A, Z), (B, Z)], FB.ghint(N_HINTS), [FB.GA, FB.GB], g(".multihead_attn.in_proj_weight"), g(".multihead_attn.in_proj_bias"), arm, True)
    good, tol = FB.attention_tiles_b(*args)
    bad, _ = FB.attention_tiles_b(*args, mut=mut)
    return FB.ratio(bad, good, tol)


BIG_ROW = 8 * 3 + N_HINTS - 1  # the large-mean hint row of fixture(big_mean=True)


def decoder_mutant(mut, arm, stage, big_mean=False, rows=slice(None)):
    """stage 0..2 of the hint tile's pass of layer 0, fed the unmutated reference's own taps (exact inputs: nothing compounds)"""
    sd, A, B, H = fixture(big_mean)
    args = (H, Z, [(A, Z), (B, Z)], FB.ghint(N_HINTS), [FB.GA, FB.GB], sd, "cross_hints.0", arm)
    own = FB.decoder_stages_b(*args)
    taps = (own[0][0], own[1][0])
    good = FB.decoder_stages_b(*args, taps=taps)
    bad = FB.decoder_stages_b(*args, taps=taps, mut=mut)
    return FB.ratio(bad[stage][0][rows], good[stage][0][rows], good[stage][1][rows])


def pooling_mutant(arm):
    sd, A, B, H = fixture()
    o, h = FB.pairs(4, N_HINTS, 1)
    good, _, tile, _ = FB.workgroup_b(o, h, sd, 2, arm)
    tol = FB.mlp_b(FB.pool(tile, N_HINTS), 0.0 * FB.pool(tile, N_HINTS), sd)[1]  # the stage's own bound: the tile taken as exact
    bad = FB.mlp_offsets(FB.pool(tile, N_HINTS, all8=True), sd)
    assert (tile.reshape(4, 8, 128)[:, N_HINTS:].max(axis=1) > FB.pool(tile, N_HINTS)).any()  # a padding row can win the max
    return FB.ratio(bad, good, tol)


def mutant_ratio(mut, arm):
    if mut in ("mask_le", "neighbour", "head_cols", "shared_zero", "shared_resplit", "drop_lo", "drop_lo_q"):
        return attention_mutant(mut, arm)
    if mut == "sa_for_ca":
        return decoder_mutant(mut, arm, 1)
    if mut == "ffn_bias":
        return decoder_mutant(mut, arm, 2)
    if mut == "ln_onepass":
        return decoder_mutant(mut, arm, 0, big_mean=True)
    assert mut == "max_all8"
    return pooling_mutant(arm)


@pytest.mark.parametrize("mut", ASSERTED)
def test_asserted_mutants_leave_their_stage_bound(mut):
    r = {arm: mutant_ratio(mut, arm) for arm in ARMS2}
    print(f"FINEMUTANT {mut} " + " ".join(f"{a}={v:.4g}" for a, v in r.items()))
    assert all(v > 1.0 for v in r.values()), r


@pytest.mark.parametrize("mut", NOT_ASSERTED)
def test_report_the_mutants_the_worst_case_bounds_cannot_see(mut):
    """reported, not asserted above 1 (profiles/fine_blocks.md says why each stays below); they must still be other computations
    where the fault changes a value at all, and they must not have become visible unnoticed"""
    arms = ("split",) if mut == "drop_lo_q" else ARMS2
    r = {arm: mutant_ratio(mut, arm) for arm in arms}
    print(f"FINEMUTANT {mut} (not asserted) " + " ".join(f"{a}={v:.4g}" for a, v in r.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in r.values()), f"{mut} is visible now: move it to ASSERTED ({r})"
    if mut != "shared_resplit":  # (a re-split changes which neighbour is hi, never the value hi + lo)
        assert all(v > 0.0 for v in r.values()), r
    if mut == "ln_onepass":  # on the large-mean row itself: every product bound of the stage grows with that mean (K u mag)
        big = {arm: decoder_mutant(mut, arm, 0, big_mean=True, rows=slice(BIG_ROW, BIG_ROW + 1)) for arm in arms}
        print(f"FINEMUTANT {mut} (not asserted) on the large-mean row " + " ".join(f"{a}={v:.4g}" for a, v in big.items()))


def test_fixture_conditions():
    sd, A, B, H = fixture()
    for n in (0, 1, 2):
        w = FB.weights(n)
        for k, v in w.items():
            if ".norm" in k and k.startswith("cross_"):
                assert (np.abs(v - 1.0).min() > 0.05) if k.endswith("weight") else (np.abs(v).mean() > 0.05), k
    g1, g2, g3 = (np.asarray(sd[f"cross_hints.0.norm{i}.weight"]) for i in (1, 2, 3))
    assert g1.min() > g2.max() > g2.min() > g3.max()  # the three gains cannot be confused
    hint_rows = H.reshape(4, 8, 128)[:, :N_HINTS]
    assert (hint_rows.max(axis=1) < 0).any() and np.all(H.reshape(4, 8, 128)[:, N_HINTS:] == 0)  # a zero padding row could win a max
    assert np.linalg.norm(FB.junk(np.random.default_rng(0), (3, 128)), axis=1).max() < FB.GUARD
    # the logits' spread stays inside the range over which EPS_EXP was measured (keys further down add EXP_TAIL instead)
    g = FB._get(sd, "cross_hints.0")
    s = FB.logit_spread(H, H, FB.ghint(N_HINTS), FB.ghint(N_HINTS), g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias"))
    assert 0 < s < FB.LOGIT_RANGE, s


def test_the_split_of_a_float32_value_is_what_the_planes_hold():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(4096) * np.exp(rng.uniform(-12, 8, 4096))).astype(F32)
    hi, lo = FB.split(v)
    err = np.abs(FB.join64(hi, lo) - v.astype(np.float64))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
    assert (FB.store_err(v.astype(np.float64), 0.0, True) >= err).all()
