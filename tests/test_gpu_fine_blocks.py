"""GPU tier of the fine-match block tests: one attention block and one decoder pass of csrc/fine.hip at a time through the dev library
(csrc/fine_blocks.hip; contexts made through libt2l_blocks.so, weights packed by their own t2l_fine_load_weights), every element of
every tile against the float64 references and derived bounds of tests/fine_blocks.py, each stage fed the kernel's own input; then the
chain of stage calls against the product's own t2l_fine_match, the norm guard, and the whole match against float64.

Tiles are carved between NaN halos (tests/guards.py). Each test prints `FINEBLOCK stage arm case worst-err/tol` lines (pytest -s); the
MI355X figures are in profiles/fine_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import fine_blocks as FB
from tests import guards

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
ARMS = ("f32", "split", "f16")
ARM_OPTIONS = {"split": (0, 0), "f16": (0, 1), "f32": (1, 0)}  # (encoder_f32, encoder_f16)
HINTS = (1, 5, 6, 8)


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return FB.load_blocks()


@pytest.fixture(scope="module")
def models(lib):
    """{n_layers: (engine made through the blocks library, state dict)} for 0, 1 and 2 decoder layers"""
    from text2loc_amd.engine import Engine

    out = {}
    for n in (0, 1, 2):
        e = Engine(0, lib=lib)
        sd = FB.weights(n)
        e.fine_load_weights(sd, class_embed=True, color_embed=True, num_layers=n)
        out[n] = (e, sd)
    yield out
    for e, _ in out.values():
        e.close()


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


# ---- tiles in the arm's own storage: (f32 rows,) or (hi plane, lo plane), numpy [n_wg, 32, 128] -------------------------------
def store(arm, v):
    v = np.ascontiguousarray(v, dtype=F32).reshape(-1, 32, 128)
    return (v,) if arm == "f32" else FB.split(v)


def value(st):
    return st[0].astype(np.float64) if len(st) == 1 else FB.join64(*st)


def up(st):
    import torch

    return [guards.guarded(torch.from_numpy(np.ascontiguousarray(a)).cuda(), guards.NAN) for a in st]


def ptrs(ts):
    """(a, b) pointers of an uploaded tile (b null for the f32 arm), (None, None) for no tile"""
    if ts is None:
        return [None, None]
    return [ctypes.c_void_p(t.data_ptr()) for t in ts] + [None] * (2 - len(ts))


def groups(g):
    return None if g is None else (ctypes.c_int32 * 4)(*g)


def down(ts):
    return tuple(t.cpu().numpy() for t in ts)


def run_attention(lib, eng, arm, which, layer, ca, form, x, gx, mem, gm, mem2, gm2, init):
    dx, dm, dm2, do = up(x), (up(mem) if mem else None), (up(mem2) if mem2 else None), up(init)
    n_wg = x[0].shape[0]
    ok(lib, lib.t2l_blk_fine_attention(eng._h, FB.ARM_ID[arm], n_wg, which, layer, ca, form, *ptrs(dx), groups(gx), *ptrs(dm), groups(gm),
                                       *ptrs(dm2), groups(gm2), *ptrs(do)))
    guards.check_halos(*dx, *(dm or []), *(dm2 or []), *do)
    return down(do)


def run_decoder(lib, eng, arm, which, layer, x, gx, mem, gm, mem2=None, gm2=None, taps=True):
    """-> (x tile out, tap 1, tap 2) in the arm's storage"""
    import torch

    dx, dm, dm2 = up(x), up(mem), (up(mem2) if mem2 else None)
    outs = [[guards.guarded(torch.zeros_like(t), guards.NAN) for t in dx] for _ in range(3 if taps else 1)]
    n_wg = x[0].shape[0]
    tap_ptrs = ptrs(outs[1]) + ptrs(outs[2]) if taps else [None] * 4
    ok(lib, lib.t2l_blk_fine_decoder(eng._h, FB.ARM_ID[arm], n_wg, which, layer, *ptrs(dx), groups(gx), *ptrs(dm), groups(gm), *ptrs(dm2),
                                     groups(gm2), *ptrs(outs[0]), *tap_ptrs))
    guards.check_halos(*dx, *dm, *(dm2 or []), *[t for o in outs for t in o])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(down(dx), x))  # the input tile is not written
    return [down(o) for o in outs]


def report(stage, arm, case, r):
    print(f"FINEBLOCK {stage} {arm} {case} {r:.4g}")
    return r


def tiles(n_hints, seed, junk_rows=True, obj_count=16):
    """object tiles A, B and the hint tile of four pairs (float32 [32, 128] each); unused rows (hint padding, objects >= obj_count)
    hold large finite junk instead of zeros"""
    o, h = FB.pairs(4, n_hints, seed)
    A, B, H = FB.tiles_of(o, h, n_hints)
    if junk_rows:
        rng = np.random.default_rng(seed)
        pad = (np.arange(32) & 7) >= n_hints
        H[pad] = FB.junk(rng, (int(pad.sum()), 128))
        cut = (np.arange(32) & 15) >= obj_count
        A[cut], B[cut] = FB.junk(rng, (int(cut.sum()), 128)), FB.junk(rng, (int(cut.sum()), 128))
    return A, B, H


# ---- attention alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ARMS)
def test_attention_block_alone(lib, models, arm):
    """every element of obuf inside the bound — the rows a call must leave as they were (or must write as zeros) exactly so; keys
    behind the mask hold +-4 junk and must not leak"""
    eng, sd = models[2]
    rng = np.random.default_rng(11)
    init32 = rng.standard_normal((1, 32, 128)).astype(F32)
    worst = {}

    def hold(case, which, layer, ca, form, x, gx, mems, gms):
        name = ("cross_hints" if which else "cross_objects") + f".{layer}" + (".multihead_attn" if ca else ".self_attn")
        W, b = sd[name + ".in_proj_weight"], sd[name + ".in_proj_bias"]
        sx, smem, init = store(arm, x), [store(arm, m) for m in mems], store(arm, init32)
        got = run_attention(lib, eng, arm, which, layer, ca, form, sx, gx, smem[0] if smem else None, gms[0] if gms else None,
                            smem[1] if len(smem) > 1 else None, gms[1] if len(gms) > 1 else None, init)
        vx = value(sx)[0]
        z = np.zeros((32, 128))
        ref_mems = [(value(m)[0], z) for m in smem] if smem else [(vx, z)]
        ref, tol = FB.attention_tiles_b(vx, z, ref_mems, gx, gms if gms else [gx], W, b, arm, shared=form != 0, init=value(init)[0])
        worst[case] = report("attention", arm, case, FB.ratio(value(got)[0], ref, tol))
        return value(got)[0], value(init)[0]

    for n in HINTS:
        A, B, H = tiles(n, 30 + n)
        hold(f"hint-self n={n}", 1, 1, 0, 0, H, FB.ghint(n), [], [])
        hold(f"obj-hint n={n}", 0, n % 2, 1, 0, A if n % 2 else B, FB.GA if n % 2 else FB.GB, [H], [FB.ghint(n)])
        hold(f"hint-obj2 n={n}", 1, n % 2, 1, 1, H, FB.ghint(n), [A, B], [FB.GA, FB.GB])
    A, B, H = tiles(6, 40)
    hold("obj-self A", 0, 0, 0, 0, A, FB.GA, [], [])
    hold("obj-self B", 0, 1, 0, 0, B, FB.GB, [], [])
    # the first shared pass alone: the rows of pairs 2, 3 find no key in tile A — planes keep what obuf held, the f32 form writes zeros
    got, init = hold("hint-objA-only", 1, 0, 1, 2, H, FB.ghint(6), [A], [FB.GA])
    assert np.array_equal(got[16:], init[16:] if arm != "f32" else np.zeros((16, 128)))
    got, _ = hold("hint-objB form0", 1, 0, 1, 0, H, FB.ghint(6), [B], [FB.GB])  # one tile, not shared: the keyless rows are zeros
    assert np.array_equal(got[:16], np.zeros((16, 128)))
    # one key per pair, its lo residues aligned to one value-projection row: where a dropped lo plane shows (CPU tier: drop_lo)
    _, Bl, Hl = FB.lo_fixture(sd)
    hold("obj-hint n=1 lo-aligned", 0, 0, 1, 0, Bl, FB.GB, [Hl], [FB.ghint(1)])
    # object counts below 16 (masking only): rows >= count of both object tiles hold junk
    for cnt in (1, 11, 15):
        A, B, H = tiles(5, 50 + cnt, obj_count=cnt)
        hold(f"hint-obj2 count={cnt}", 1, 1, 1, 1, H, FB.ghint(5), [A, B], [(4, cnt, 32, 0), (4, cnt, 32, 2)])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- one decoder pass, with its two in-layer taps ------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ARMS)
def test_decoder_pass_stage_by_stage(lib, models, arm):
    """obj and hint decoders of layers 0 and 1 of the 2-layer model and cross_hints of the 0-layer model: the x tile after each of the
    three residual + LayerNorms inside its stage's bound; stages 2 and 3 are fed the kernel's own tap of the stage before"""
    worst = {}
    z = np.zeros((32, 128))
    for n_layers, which, layer, n in ((2, 0, 0, 5), (2, 0, 1, 8), (2, 1, 0, 6), (2, 1, 1, 1), (0, 1, 0, 5)):
        eng, sd = models[n_layers]
        A, B, H = tiles(n, 60 + 10 * n_layers + 2 * layer + which)
        if which:
            x, gx, mems, gms = H, FB.ghint(n), [A, B], [FB.GA, FB.GB]
        else:
            x, gx, mems, gms = (B, FB.GB, [H], [FB.ghint(n)]) if layer else (A, FB.GA, [H], [FB.ghint(n)])
        sx, smem = store(arm, x), [store(arm, m) for m in mems]
        out, t1, t2 = run_decoder(lib, eng, arm, which, layer, sx, gx, smem[0], gms[0], smem[1] if which else None, gms[1] if which else None)
        stages = FB.decoder_stages_b(value(sx)[0], z, [(value(m)[0], z) for m in smem], gx, gms, sd, FB.prefix_of(which, layer, n_layers), arm,
                                     taps=(value(t1)[0], value(t2)[0]))
        for k, got in enumerate((t1, t2, out)):
            case = f"{FB.prefix_of(which, layer, n_layers)} n={n} ln{k + 1}"
            worst[case] = report("decoder", arm, case, FB.ratio(value(got)[0], *stages[k]))
        alone = run_decoder(lib, eng, arm, which, layer, sx, gx, smem[0], gms[0], smem[1] if which else None, gms[1] if which else None, taps=False)[0]
        assert all(np.array_equal(a, b) for a, b in zip(alone, out))  # the taps change nothing
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- the chain of stage calls is the product ---------------------------------------------------------------------------------------
def chain(lib, eng, arm, n_layers, obj, hints, ci, hi, n_pairs):
    """the product's tile arrangement (fine_match_kernel: four pairs per workgroup, tail pairs duplicated) through the decoder wrapper in
    the product's order -> the last hint tile, float64 [n_wg, 32, 128]"""
    n_hints = hints.shape[1]
    n_wg = (n_pairs + 3) // 4
    pair = np.minimum(np.arange(4 * n_wg), n_pairs - 1)
    c = pair if ci is None else ci[pair]
    h = pair if hi is None else hi[pair]
    o = obj[c].reshape(n_wg, 64, 128)
    hint = np.zeros((n_wg, 4, 8, 128), F32)
    hint[:, :, :n_hints] = hints[h].reshape(n_wg, 4, n_hints, 128)
    t = {"A": store(arm, o[:, :32]), "B": store(arm, o[:, 32:]), "H": store(arm, hint.reshape(n_wg, 32, 128))}
    gr = {"A": FB.GA, "B": FB.GB, "H": FB.ghint(n_hints)}
    for xn, which, layer in FB.passes(n_layers):
        if xn == "H":
            t[xn] = run_decoder(lib, eng, arm, which, layer, t["H"], gr["H"], t["A"], FB.GA, t["B"], FB.GB, taps=False)[0]
        else:
            t[xn] = run_decoder(lib, eng, arm, which, layer, t[xn], gr[xn], t["H"], gr["H"], taps=False)[0]
    return value(t["H"])


def product(eng, arm, obj, hints, ci, hi):
    import torch

    f32, f16 = ARM_OPTIONS[arm]
    eng.set_option("encoder_f32", f32)
    eng.set_option("encoder_f16", f16)
    dev = lambda a, dt=None: None if a is None else guards.guarded(torch.from_numpy(np.ascontiguousarray(a)).cuda(), guards.NAN if dt is None else 0)
    d = [dev(obj), dev(hints), dev(ci, "i"), dev(hi, "i")]
    off = eng.fine_match(d[0], d[1], d[2], d[3])
    guards.check_halos(*[t for t in d if t is not None])
    return off.cpu().numpy()


def chain_vs_product(lib, models, arm, n_layers, n_pairs, indexed, seed, perm=None):
    eng, sd = models[n_layers]
    rng = np.random.default_rng([seed, n_pairs])
    n_hints = (6, 5, 8, 1)[n_pairs % 4]
    obj, hints = FB.pairs(9, n_hints, seed)
    ci = rng.integers(0, 9, n_pairs).astype(np.int32) if indexed else None
    hi = rng.integers(0, 9, n_pairs).astype(np.int32) if indexed else None
    if perm is not None:
        ci, hi = perm.astype(np.int32), perm.astype(np.int32)
    if not indexed and perm is None:
        obj, hints = obj[:n_pairs], hints[:n_pairs]
    got = product(eng, arm, obj, hints, ci, hi)
    tile = chain(lib, eng, arm, n_layers, obj, hints, ci, hi, n_pairs)
    pooled = np.concatenate([FB.pool(t, n_hints) for t in tile])[:n_pairs]
    ref, tol = FB.mlp_b(pooled, np.zeros_like(pooled), sd)  # the two small linears in plain float32: K = 128, 64
    return got, ref, tol


@pytest.mark.parametrize("n_layers", [0, 1, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_the_chain_of_stage_calls_is_the_product(lib, models, arm, n_layers):
    """the wrapper chained in the product's order leaves the product's hint tile: max-pooled and put through mlp_offsets in float64 it
    meets the offsets of the product's own t2l_fine_match within the float32 bound of the two small linears — one to three workgroups,
    tail duplication, with and without index arrays, every pair in each of the four places"""
    worst = {}
    for n_pairs in (1, 3, 4, 5, 9):
        for indexed in (False, True):
            got, ref, tol = chain_vs_product(lib, models, arm, n_layers, n_pairs, indexed, 70 + n_layers)
            worst[f"pairs={n_pairs} idx={int(indexed)}"] = FB.ratio(got, ref, tol)
    first = None
    for shift in range(4):  # pairs 0..3 rotated through the four places of the workgroup
        perm = np.roll(np.arange(4), shift)
        got, ref, tol = chain_vs_product(lib, models, arm, n_layers, 4, True, 80, perm)
        worst[f"rotate {shift}"] = FB.ratio(got, ref, tol)
        first = got if first is None else first
        assert np.array_equal(got[np.argsort(perm)], first), shift  # a pair's offsets do not depend on its place
    case = max(worst, key=worst.get)
    report("chain", arm, f"layers={n_layers} {case}", worst[case])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- the norm guard ----------------------------------------------------------------------------------------------------------------
def test_guard_routes_whole_workgroups_to_the_f32_arm(lib, models):
    """nine pairs, one hint row of pair 5 above kFGuardNorm: workgroup 1 (pairs 4..7) is served by the f32 arm — held at the f32 arm's
    bound and bit-equal to an encoder_f32 run —, the others by the split arm — held at the split arm's bound; workgroup 0's eight floats
    are not the f32 arm's bits (the tail workgroup's two floats may coincide: the arms differ by a few ulp)."""
    eng, sd = models[1]
    obj, hints = FB.pairs(9, 5, 90)
    hints[5, 2] *= F32(10.0)  # norm ~ 110
    assert np.linalg.norm(hints[5, 2]) > 1.5 * FB.GUARD and np.linalg.norm(hints.reshape(-1, 128), axis=1)[np.arange(45) != 27].max() < FB.GUARD / 2
    got = product(eng, "split", obj, hints, None, None)
    all32 = product(eng, "f32", obj, hints, None, None)
    r32 = FB.ratio(got[4:8], *FB.cross_match_bound(obj[4:8], hints[4:8], sd, 1, "f32"))
    rs = max(FB.ratio(got[s], *FB.cross_match_bound(obj[s], hints[s], sd, 1, "split")) for s in (slice(0, 4), slice(8, 9)))
    report("guard", "f32", "flagged workgroup", r32)
    report("guard", "split", "other workgroups", rs)
    assert r32 <= 1.0 and rs <= 1.0
    assert np.array_equal(got[4:8], all32[4:8]) and not np.array_equal(got[:4], all32[:4])


def test_guard_threshold_is_the_comparison_the_kernel_states(lib, models):
    """a row of norm exactly 64 (ss = 4096 <= 64^2: not flagged) and the next float32 above (ss = 4096 + 2^-10: flagged), one non-zero
    component each so that the float32 ss is unambiguous"""
    eng, sd = models[1]
    obj, hints = FB.pairs(8, 5, 91)
    at, above = F32(64.0), np.nextafter(F32(64.0), F32(128.0))
    assert F32(above * above) > F32(4096.0) and F32(at * at) == F32(4096.0)
    hints[1, 3] = 0
    hints[1, 3, 17] = at
    hints[6, 0] = 0
    hints[6, 0, 90] = -above
    got = product(eng, "split", obj, hints, None, None)
    all32 = product(eng, "f32", obj, hints, None, None)
    rs = FB.ratio(got[:4], *FB.cross_match_bound(obj[:4], hints[:4], sd, 1, "split"))
    r32 = FB.ratio(got[4:], *FB.cross_match_bound(obj[4:], hints[4:], sd, 1, "f32"))
    report("guard", "split", "norm = 64", rs)
    report("guard", "f32", "norm = nextafter(64)", r32)
    assert rs <= 1.0 and r32 <= 1.0
    assert np.array_equal(got[4:], all32[4:]) and not np.array_equal(got[:4], all32[:4])  # which arm really served which workgroup


# ---- the whole match against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [0, 1, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_the_whole_match_against_float64(lib, models, arm, n_layers):
    """t2l_fine_match against cross_match64 at the compounded bound (chained worst cases through every pass: it saturates at the
    LayerNorms' range and is orders of magnitude above the 5e-5 bar of tests/test_gpu_fine.py, which stays; profiles/fine_blocks.md)"""
    eng, sd = models[n_layers]
    obj, hints = FB.pairs(4, 6, 95 + n_layers)
    got = product(eng, arm, obj, hints, None, None)
    ref, tol = FB.cross_match_bound(obj, hints, sd, n_layers, arm)
    assert np.array_equal(ref, FB.cross_match64(obj, hints, sd, n_layers))
    err = float(np.abs(got - ref).max())
    report("match", arm, f"layers={n_layers} (bound {tol.min():.3g}..{tol.max():.3g}, err {err:.3g})", FB.ratio(got, ref, tol))
    assert FB.ratio(got, ref, tol) <= 1.0


# ---- the three float32 forms the bounds take from a measurement ------------------------------------------------------------------
def probe(lib, x):
    import torch

    d = guards.guarded(torch.from_numpy(x).cuda(), guards.NAN)
    outs = [guards.guarded(torch.zeros_like(d), guards.NAN) for _ in range(3)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ok(lib, lib.t2l_blk_fine_probe(p(d), *[p(o) for o in outs], x.size))
    guards.check_halos(d, *outs)
    return [o.cpu().numpy().astype(np.float64) for o in outs]


def probe_errors(lib):
    """worst errors of __expf (relative on [-LOGIT_RANGE, 0], absolute on [-2^17, -LOGIT_RANGE]), 1.0f / sqrtf and 1.f / x (relative)"""
    rng = np.random.default_rng(1)
    n = 1 << 20
    near = -rng.uniform(0, FB.LOGIT_RANGE, n).astype(F32)
    near[:4] = (0.0, -FB.LOGIT_RANGE, -1.0, -0.5)
    e = probe(lib, near)[0]
    want = np.exp(near.astype(np.float64))
    eps_exp = float(np.abs(e / want - 1).max())
    far = -np.exp(rng.uniform(np.log(FB.LOGIT_RANGE), np.log(2.0 ** 17), n)).astype(F32)
    tail = float(np.abs(probe(lib, far)[0] - np.exp(far.astype(np.float64))).max())
    pos = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), n)).astype(F32)  # LayerNorm variances + eps and softmax sums lie well inside
    _, rs, rc = probe(lib, pos)
    p64 = pos.astype(np.float64)
    return eps_exp, tail, float(np.abs(rs * np.sqrt(p64) - 1).max()), float(np.abs(rc * p64 - 1).max())


def test_the_measured_constants_hold(lib):
    eps_exp, tail, eps_rs, eps_rc = probe_errors(lib)
    print(f"FINEBLOCK probe - __expf rel {eps_exp:.4g} tail abs {tail:.4g} rsqrt rel {eps_rs:.4g} rcp rel {eps_rc:.4g}")
    assert eps_exp <= FB.EPS_EXP and tail <= FB.EXP_TAIL and eps_rs <= FB.EPS_RSQRT and eps_rc <= FB.EPS_RCP


# ---- the wrappers refuse what is outside their contract ------------------------------------------------------------------------------
def test_the_wrappers_refuse_before_they_launch(lib, models):
    eng, _ = models[2]
    eng0, _ = models[0]
    A, B, H = tiles(5, 99)
    x, mem = up(store("split", H)), up(store("split", A))
    out = up(store("split", np.full((1, 32, 128), 7.0, F32)))
    before = down(out)
    att = lambda e, arm, n_wg, which, layer, ca, form, gx, gm: lib.t2l_blk_fine_attention(
        e._h, arm, n_wg, which, layer, ca, form, *ptrs(x), groups(gx), *ptrs(mem), groups(gm), None, None, None, *ptrs(out))
    for args, msg in (((eng, 1, 1, 1, 0, 1, 0, (3, 9, 32, 0), FB.GA), b"gx is none"), ((eng, 1, 1, 1, 0, 1, 0, (3, 0, 32, 0), FB.GA), b"gx is none"),
                      ((eng, 1, 1, 1, 0, 1, 0, FB.ghint(5), (4, 16, 32, 1)), b"gm is none"), ((eng, 1, 1, 1, 0, 1, 0, FB.ghint(5), (4, 17, 32, 0)), b"gm is none"),
                      ((eng, 1, 1, 1, 0, 1, 0, FB.ghint(5), (4, 16, 16, 0)), b"gm is none"), ((eng, 3, 1, 1, 0, 1, 0, FB.ghint(5), FB.GA), b"arm 0..2"),
                      ((eng, 1, 0, 1, 0, 1, 0, FB.ghint(5), FB.GA), b"n_wg"), ((eng, 1, 1, 1, 2, 1, 0, FB.ghint(5), FB.GA), b"no such decoder"),
                      ((eng0, 1, 1, 0, 0, 1, 0, FB.ghint(5), FB.GA), b"no such decoder"), ((eng, 1, 1, 1, 0, 1, 1, FB.ghint(5), FB.GA), b"mem2")):
        assert att(*args) == -1 and msg in lib.t2l_blk_last_error(), (args[1:], lib.t2l_blk_last_error())
    dec = lambda gx, gm, m2, gm2: lib.t2l_blk_fine_decoder(eng._h, 1, 1, 1, 0, *ptrs(x), groups(gx), *ptrs(mem), groups(gm), *ptrs(m2), groups(gm2),
                                                           *ptrs(out), None, None, None, None)
    assert dec(FB.ghint(5), FB.GA, None, None) == -1 and b"object tile A (mem) and object tile B" in lib.t2l_blk_last_error()
    assert dec(FB.ghint(5), FB.GB, mem, FB.GA) == -1 and b"object tile A (mem) and object tile B" in lib.t2l_blk_last_error()
    assert dec(FB.GA, FB.GA, None, None) == -1 and b"attends the hint tile alone" in lib.t2l_blk_last_error()
    assert lib.t2l_blk_fine_attention(None, 1, 1, 1, 0, 1, 0, *ptrs(x), groups(FB.ghint(5)), *ptrs(mem), groups(FB.GA), None, None, None, *ptrs(out)) == -1
    guards.check_halos(*x, *mem, *out)
    assert all(np.array_equal(a, b) for a, b in zip(down(out), before))  # a refused call launched nothing
