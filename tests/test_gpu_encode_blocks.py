"""GPU tier of the encoder-layer block tests: ONE call of planes_layer (csrc/encode.hip) at a time through the dev library's door
(csrc/encode_blocks.hip; contexts made through libt2l_blocks.so, weights packed by their own t2l_load_weights /
t2l_text_head_load_weights), every element of every stage — the attention output, the planes behind LayerNorm 1, the hidden planes of
every feed-forward pass, the result — against the float64 references, derived bounds and exact float32 models of
tests/encode_blocks.py, each stage fed the kernel's own predecessor; then the door's result against the product's own t2l_text_inter,
bit for bit.

Planes are carved between NaN halos (tests/guards.py). Each test prints `ENCBLOCK stage arm case worst-err/tol` lines (pytest -s); the
MI355X figures are in profiles/encode_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import encode_blocks as EB
from tests import guards

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
TEXT_SHAPES = sorted(EB.TEXT)
TEXT_IDS = [f"d{D}_h{h}" for D, h in TEXT_SHAPES]


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return EB.load_blocks()


@pytest.fixture(scope="module")
def engines(lib):
    """engine(('cell', kind)) / engine(('text', D, heads, kind)) -> (engine made through the blocks library, state dict), cached"""
    from text2loc_amd.engine import Engine

    made = {}

    def get(key):
        if key not in made:
            e = Engine(0, lib=lib)
            if key[0] == "cell":
                sd = EB.cell_weights(key[1])
                e.load_weights(sd, class_embed=True, color_embed=True)
            else:
                sd = EB.text_weights(key[1], key[2], key[3])
                e.text_head_load_weights(sd, inter_num_heads=key[2])
            made[key] = (e, sd)
        return made[key]

    yield get
    for e, _ in made.values():
        e.close()


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


def report(stage, arm, case, r):
    print(f"ENCBLOCK {stage} {arm} {case} {r:.4g}")
    return r


def run_layer(lib, eng, geo, arm, layer, S, last_to_f32, xh, xl, taps=True):
    """one t2l_blk_enc_layer call on planes xh, xl (f16 [n_wg, 2, 32, D]) -> dict of numpy arrays: att, x1, out (hi, lo), hid (hi, lo)
    [n_wg, ffp, 2, 32, D], out_f (float32, last_to_f32), bad [n_wg]"""
    import torch

    n_wg, D = xh.shape[0], geo.D
    dev = lambda a: guards.guarded(torch.from_numpy(np.ascontiguousarray(a)).cuda(), guards.NAN)
    new = lambda shape, dt: guards.guarded(torch.zeros(shape, dtype=dt, device="cuda"), guards.NAN)
    dx = [dev(xh), dev(xl)]
    pl = lambda: [new((n_wg, 2, 32, D), torch.float16) for _ in range(2)]
    att, x1, out = pl(), pl(), pl()
    hid = [new((n_wg, geo.ffp, 2, 32, D), torch.float16) for _ in range(2)]
    out_f = new((n_wg, 2, 32, D), torch.float32)
    bad = guards.guarded(torch.full((n_wg,), -1, dtype=torch.int32, device="cuda"), 7)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    tp = [p(t) for t in att + x1 + hid] if taps else [None] * 6
    res = [None, None, p(out_f)] if last_to_f32 else [p(out[0]), p(out[1]), None]
    ok(lib, lib.t2l_blk_enc_layer(eng._h, geo.inst, EB.ARM_ID[arm], n_wg, layer, S, int(last_to_f32), p(dx[0]), p(dx[1]), *tp, *res, p(bad)))
    guards.check_halos(*dx, *att, *x1, *out, *hid, out_f, bad)
    assert np.array_equal(dx[0].cpu().numpy(), xh) and np.array_equal(dx[1].cpu().numpy(), xl)  # the input planes are not written
    n = lambda ts: tuple(t.cpu().numpy() for t in ts)
    return {"att": n(att), "x1": n(x1), "hid": n(hid), "out": n(out), "out_f": out_f.cpu().numpy(), "bad": bad.cpu().numpy()}


def tile_taps(geo, got, w, t):
    return {"att": (got["att"][0][w, t], got["att"][1][w, t]), "x1": (got["x1"][0][w, t], got["x1"][1][w, t]),
            "hid": [(got["hid"][0][w, c, t], got["hid"][1][w, c, t]) for c in range(geo.ffp)]}


def tile_value(geo, got, stage, w, t, last_to_f32):
    if stage == "out":
        return got["out_f"][w, t].astype(np.float64) if last_to_f32 else EB.join64(got["out"][0][w, t], got["out"][1][w, t])
    if stage.startswith("hid"):
        c = int(stage[3:])
        return EB.join64(got["hid"][0][w, c, t], got["hid"][1][w, c, t])
    return EB.join64(got[stage][0][w, t], got[stage][1][w, t])


def hold_bounds(lib, eng, sd, prefix, geo, arm, layer, S, last_to_f32, x32, vis, case, worst):
    """one call on the tiles x32 (float32 [n_wg, 2, 32, D], split here), every stage of every tile inside its derived bound"""
    xh, xl = EB.split(x32)
    got = run_layer(lib, eng, geo, arm, layer, S, last_to_f32, xh, xl)
    assert not got["bad"].any(), (case, got["bad"])
    for w in range(xh.shape[0]):
        for t in range(2):
            ref = EB.layer_stages(geo, sd, prefix, xh[w, t], xl[w, t], vis, arm, last_to_f32, taps=tile_taps(geo, got, w, t))
            for stage, (val, tol) in ref.items():
                name = "hid" if stage.startswith("hid") else stage
                r = EB.ratio(tile_value(geo, got, stage, w, t, last_to_f32), val, tol)
                worst[name] = max(worst.get(name, 0.0), r) if r == r else float("nan")
    return got


def finish(worst, arm, case):
    for stage, r in worst.items():
        report(stage, arm, case, r)
    assert worst and all(r < 1.0 for r in worst.values()), worst


# ---- the measured constants -----------------------------------------------------------------------------------------------------
def probe(lib, x):
    import torch

    d = guards.guarded(torch.from_numpy(x).cuda(), guards.NAN)
    outs = [guards.guarded(torch.zeros_like(d), guards.NAN) for _ in range(3)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ok(lib, lib.t2l_blk_enc_probe(p(d), *[p(o) for o in outs], x.size))
    guards.check_halos(d, *outs)
    return [o.cpu().numpy().astype(np.float64) for o in outs]


def test_the_measured_constants_hold(lib):
    """__expf (relative on [-16, 0], absolute on [-2^17, -16]), 1.0f / sqrtf and 1.f / x (relative) as encode_blocks.hip compiles them"""
    rng = np.random.default_rng(1)
    n = 1 << 20
    rng_ = EB.FB.LOGIT_RANGE
    near = -rng.uniform(0, rng_, n).astype(F32)
    near[:4] = (0.0, -rng_, -1.0, -0.5)
    e = probe(lib, near)[0]
    assert e[0] == 1.0  # __expf(0): the p = 1 of the S = 1 cases
    eps_exp = float(np.abs(e / np.exp(near.astype(np.float64)) - 1).max())
    far = -np.exp(rng.uniform(np.log(rng_), np.log(2.0 ** 17), n)).astype(F32)
    tail = float(np.abs(probe(lib, far)[0] - np.exp(far.astype(np.float64))).max())
    pos = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), n)).astype(F32)
    pos[0] = 1.0
    _, rs, rc = probe(lib, pos)
    assert rc[0] == 1.0  # 1.f / 1.f
    p64 = pos.astype(np.float64)
    eps_rs, eps_rc = float(np.abs(rs * np.sqrt(p64) - 1).max()), float(np.abs(rc * p64 - 1).max())
    print(f"ENCBLOCK probe - __expf rel {eps_exp:.4g} tail abs {tail:.4g} rsqrt rel {eps_rs:.4g} rcp rel {eps_rc:.4g}")
    P = EB.PROBE
    assert eps_exp <= P["EPS_EXP"] and tail <= P["EXP_TAIL"] and eps_rs <= P["EPS_RSQRT"] and eps_rc <= P["EPS_RCP"]


# ---- Gaussian weights: every stage inside its derived bound -------------------------------------------------------------------------
@pytest.mark.parametrize("arm", EB.ARMS)
def test_cell_layer_stages_inside_their_bounds(lib, engines, arm):
    """the cell encoder's instance <SG, 256, 64, 2, false>, mask j < 28: two cells of different contents, a pair whose second tile is
    all zero, a second layer's rows; both values of last_to_f32"""
    eng, sd = engines(("cell", "gauss"))
    vis = EB.vis_cell()
    for case, layer, last, x in (("two_cells", 0, False, EB.cell_tiles(1)), ("second_zero", 0, False, EB.cell_tiles(2, second_zero=True)),
                                 ("layer1_f32", 1, True, EB.cell_tiles_wide(3)), ("layer1_planes", 1, False, EB.cell_tiles_wide(4))):
        worst = {}
        hold_bounds(lib, eng, sd, EB.CELL_PREFIX.format(layer), EB.CELL, arm, layer, 0, last, x, vis, case, worst)
        finish(worst, arm, case)


@pytest.mark.parametrize("arm", EB.ARMS)
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=TEXT_IDS)
def test_text_layer_stages_inside_their_bounds(lib, engines, shape, arm):
    """the text layer's instance <SG, D, HD, 4, true>, mask grp[i] == grp[j]: S = 1 .. 32 (S = 5: six descriptions and a partial
    group of two zero rows; S = 32: the tail workgroup's second tile has no description at all), two workgroups each"""
    D, heads = shape
    geo = EB.TEXT[shape]
    eng, sd = engines(("text", D, heads, "gauss"))
    for S in EB.TEXT_S:
        sent, n_desc = EB.text_sentences(D, S, 10 + S)
        x = EB.text_pack(sent, n_desc, S)
        for last in ((True, False) if S in (5, 32) else (True,)):
            worst = {}
            case = f"{geo}_S{S}_{'f32' if last else 'planes'}"
            hold_bounds(lib, eng, sd, EB.TEXT_PREFIX, geo, arm, 0, S, last, x, EB.vis_text(S), case, worst)
            finish(worst, arm, case)


# ---- selection weights: the exact models ----------------------------------------------------------------------------------------
def hold_selection(lib, eng, sd, prefix, geo, arm, layer, S, last, x32, kind, case):
    """every tap of one call on selection weights: the stages the selection makes known against their exact models, and the attention
    tap, where q and k are Gaussian and nothing is exact (every case but the text layer's S = 1), inside the derived attention bound of
    layer_stages on the same weights"""
    xh, xl = EB.split(x32)
    vis = EB.vis_text(S) if geo.text else EB.vis_cell()
    got = run_layer(lib, eng, geo, arm, layer, S, last, xh, xl)
    assert not got["bad"].any(), (case, got["bad"])
    worst, exact = {}, 0
    for w in range(xh.shape[0]):
        for t in range(2):
            taps = tile_taps(geo, got, w, t)
            ref = EB.selection_stages(geo, sd, prefix, xh[w, t], xl[w, t], taps, arm, last, tilt=kind == "tilt", S=S if geo.text else None)
            if "att" not in ref:
                ref["att"] = ("tol",) + EB.attention_stage(geo, EB.join64(xh[w, t], xl[w, t]), sd, prefix, vis, arm)
            assert set(ref) == set(EB.stage_names(geo)), (case, sorted(ref))  # no tap is left out
            for stage, (how, val, tol) in ref.items():
                if how == "bits":
                    c = int(stage[3:])
                    assert np.array_equal(val[0], got["hid"][0][w, c, t]) and np.array_equal(val[1], got["hid"][1][w, c, t]), (case, stage, w, t)
                    exact += 1
                else:
                    name = "hid" if stage.startswith("hid") else stage
                    r = EB.ratio(tile_value(geo, got, stage, w, t, last), val, tol)
                    worst[name] = max(worst.get(name, 0.0), r) if r == r else float("nan")
    print(f"ENCBLOCK exact {arm} {case} {exact} hidden tiles bit for bit")
    finish(worst, arm, case)


@pytest.mark.parametrize("arm", EB.ARMS)
@pytest.mark.parametrize("kind", ("sel", "tilt", "mean", "small"))
def test_cell_layer_on_selection_weights(lib, engines, kind, arm):
    eng, sd = engines(("cell", kind))
    scale = 0.25 if kind == "mean" else 1.0
    for case, layer, last, x in ((f"{kind}_layer0", 0, False, EB.cell_tiles(5, scale=scale)), (f"{kind}_layer1", 1, True, EB.cell_tiles_wide(6, scale=scale))):
        hold_selection(lib, eng, sd, EB.CELL_PREFIX.format(layer), EB.CELL, arm, layer, 0, last, x, kind, case)


@pytest.mark.parametrize("arm", EB.ARMS)
@pytest.mark.parametrize("kind", ("sel", "tilt", "mean", "small"))
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=TEXT_IDS)
def test_text_layer_on_selection_weights(lib, engines, shape, kind, arm):
    """S = 1: every row its own key, the attention tap is v; S = 6: the product's shape"""
    D, heads = shape
    geo = EB.TEXT[shape]
    eng, sd = engines(("text", D, heads, kind))
    for S, last in ((1, True), (6, False)):
        sent, n_desc = EB.text_sentences(D, S, 20 + S, scale=0.25 if kind == "mean" else 1.0)
        hold_selection(lib, eng, sd, EB.TEXT_PREFIX, geo, arm, 0, S, last, EB.text_pack(sent, n_desc, S), kind, f"{geo}_{kind}_S{S}")


# ---- the door against the product ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", EB.ARMS)
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=TEXT_IDS)
def test_the_door_reproduces_text_inter_bit_for_bit(lib, engines, shape, arm):
    """planes packed the way text_inter_fused2_kernel packs `sent` -> one door call (last_to_f32) -> the kernel's epilogue in float32
    numpy (x + y, max over the sentences) == t2l_text_inter of the same sentences: ties the ARRANGEMENT (tiles, groups, the two
    tiles of a workgroup, the tail) to the blocks; the arithmetic is tied by the stages above"""
    import torch

    D, heads = shape
    geo = EB.TEXT[shape]
    eng, _ = engines(("text", D, heads, "gauss"))
    eng.set_option("encoder_f16", 1 if arm == "f16" else 0)
    try:
        for S in (1, 5, 6, 17, 32):
            sent, n_desc = EB.text_sentences(D, S, 30 + S, n_wg=3)
            out, bad = eng.text_inter(torch.from_numpy(sent).cuda(), n_desc)
            xh, xl = EB.split(EB.text_pack(sent, n_desc, S))
            got = run_layer(lib, eng, geo, arm, 0, S, True, xh, xl, taps=False)
            assert not bad and not got["bad"].any()
            assert np.array_equal(EB.text_unpack_max(got["out_f"], sent, n_desc, S), out.cpu().numpy()), (shape, arm, S)
    finally:
        eng.set_option("encoder_f16", 0)


def test_the_taps_change_no_bit_and_the_arms_differ(lib, engines):
    """a call without taps returns the same planes as one with them (layer 0), and layer 1 on those planes — the product's order —
    gives finite f32 tiles that differ between the split and the plain-f16 arm (the arm argument reaches the kernel)"""
    eng, _ = engines(("cell", "gauss"))
    xh, xl = EB.split(EB.cell_tiles(7))
    res = {}
    for arm in EB.ARMS:
        a = run_layer(lib, eng, EB.CELL, arm, 0, 0, False, xh, xl)
        b = run_layer(lib, eng, EB.CELL, arm, 0, 0, False, xh, xl, taps=False)
        assert np.array_equal(a["out"][0], b["out"][0]) and np.array_equal(a["out"][1], b["out"][1])
        res[arm] = run_layer(lib, eng, EB.CELL, arm, 1, 0, True, *a["out"])["out_f"]
        assert np.isfinite(res[arm]).all()
    assert not np.array_equal(res["split"], res["f16"])


# ---- the row stages outside planes_layer ----------------------------------------------------------------------------------------------
def run_rows(lib, x, call):
    import torch

    d = guards.guarded(torch.from_numpy(np.ascontiguousarray(x)).cuda(), guards.NAN)
    ok(lib, call(ctypes.c_void_p(d.data_ptr())))
    guards.check_halos(d)
    return d.cpu().numpy()


def test_normalise_rows_inside_their_bound(lib):
    """normalize_rows (encode.hip, 256 wide) and normalize_rows_d<128 / 256> (encode_shaped.hip) ONE call each: every element within
    NORM_REL of the float64 F.normalize, rows >= nvalid and the zero row exactly zero; nvalid 0, 1, 27, 28 and 32"""
    for name, D, call in (("normalize_rows", 256, lambda p, nv: lib.t2l_blk_enc_normalize(2, p, nv)),
                          ("normalize_rows_d", 128, lambda p, nv: lib.t2l_blk_encs_rows(0, 128, 2, p, None, None, nv)),
                          ("normalize_rows_d", 256, lambda p, nv: lib.t2l_blk_encs_rows(0, 256, 2, p, None, None, nv))):
        worst = 0.0
        for nvalid in EB.ROW_NVALID:
            x = EB.row_tiles(D, 3 + nvalid)
            got = run_rows(lib, x, lambda p: call(p, nvalid))
            for w in range(2):
                val, tol = EB.normalize_rows_b(x[w], nvalid)
                worst = max(worst, EB.ratio(got[w], val, tol))
                assert not got[w, nvalid:].any() and not got[w, 5].any()
        report(name, "f32", f"D{D}", worst)
        assert worst < 1.0


@pytest.mark.parametrize("D", (128, 256))
def test_layer_norm_rows_inside_their_bound(lib, D):
    """layer_norm_rows_d<D> ONE call: every element within the LayerNorm's own roundings of the float64 LayerNorm of the float32 rows,
    rows 1000 sigma off zero and rows of variance 4e-4 among them"""
    import torch

    x = EB.row_tiles(D, 8)
    g, b = EB.row_gain(D, 8)
    dg, db = [guards.guarded(torch.from_numpy(a).cuda(), guards.NAN) for a in (g, b)]
    got = run_rows(lib, x, lambda p: lib.t2l_blk_encs_rows(1, D, 2, p, ctypes.c_void_p(dg.data_ptr()), ctypes.c_void_p(db.data_ptr()), 0))
    guards.check_halos(dg, db)
    worst = max(EB.ratio(got[w], *EB.layer_norm_rows_b(x[w], g, b)) for w in range(2))
    report("layer_norm_rows_d", "f32", f"D{D}", worst)
    assert worst < 1.0


# ---- the products of the one-cell kernel: mm_tiles, one product per call ------------------------------------------------------------
@pytest.fixture(scope="module")
def shaped(lib):
    """(width, kind) -> (engine made through the blocks library with shaped_weights loaded by t2l_load_weights_shaped, state dict)"""
    from text2loc_amd.engine import Engine

    made = {}

    def get(D, kind):
        if (D, kind) not in made:
            e = Engine(0, lib=lib)
            sd = EB.shaped_weights(D, kind)
            e.load_weights(sd, class_embed=True, color_embed=False, embed_dim=D, num_heads=EB.SHAPED[D])
            made[(D, kind)] = (e, sd)
        return made[(D, kind)]

    yield get
    for e, _ in made.values():
        e.close()


def run_product(lib, eng, arm, which, layer, sub, x, N):
    import torch

    dx = guards.guarded(torch.from_numpy(np.ascontiguousarray(x)).cuda(), guards.NAN)
    do = guards.guarded(torch.zeros((x.shape[0], 32, N), device="cuda"), guards.NAN)
    ok(lib, lib.t2l_blk_encs_product(eng._h, arm, which, layer, sub, x.shape[0], ctypes.c_void_p(dx.data_ptr()), ctypes.c_void_p(do.data_ptr())))
    guards.check_halos(dx, do)
    return do.cpu().numpy()


@pytest.mark.parametrize("kind", ("gauss", "sel", "tilt"))
@pytest.mark.parametrize("D", sorted(EB.SHAPED))
def test_one_cell_products_through_mm_tiles(lib, shaped, D, kind):
    """q^T, k^T (transposed products), v, out_proj, linear1, both passes of linear2, the four slots of mlp_merge and the second layer
    of the pos and num encoders, each ONE mm_tiles call on the loader's packing, in the f32, split-f16 and (width 256) plain-f16 arm,
    layers 0 and 1. Gaussian weights: every element inside the product bound. Selection weights: EQUAL to +-x (f32), +-(hi + lo) of the
    split x, +-f16(x); tilted: within 4 u |x|"""
    eng, sd = shaped(D, kind)
    for arm in ((0, 1, 2) if D == 256 else (0, 1)):
        worst, exact = 0.0, 0
        for which, sub in EB.PRODUCTS:
            if which == 7 and arm != 0:
                continue
            layer = (which + sub) % 2
            W, folded = EB.product_matrix(sd, D, which, layer, sub)
            x = EB.product_input(D, which, 40 + which)
            got = run_product(lib, eng, arm, which, layer, sub, x, W.shape[0])
            # (the product runs mlp_merge split-f16 under the plain-f16 option too, and so does the door)
            name = EB.PRODUCT_ARMS[1 if (which == 6 and arm == 2) else arm]
            for w in range(x.shape[0]):
                val, tol = EB.product_b(x[w], W, folded, name)
                if not tol.any():
                    assert np.array_equal(got[w].astype(np.float64), val), (D, kind, arm, which, sub)
                    exact += 1
                else:
                    worst = max(worst, EB.ratio(got[w], val, tol))
        report("mm_tiles", EB.PRODUCT_ARMS[arm], f"D{D}_{kind}", worst)
        print(f"ENCBLOCK exact {EB.PRODUCT_ARMS[arm]} D{D}_{kind} {exact} product tiles equal")
        assert worst < 1.0
        assert exact > 0 or kind != "sel"


def test_feature_branches_through_small_mlp(lib, shaped):
    """pos, color and num encoder of the two-cell kernel, ONE small_mlp call each (hidden layer, gemm32 on the loader's folded and
    packed weights, normalize_rows): every element inside the derived bound, rows >= nobj exactly zero; nobj 0, 1, 27, 28, 32"""
    import torch

    eng, sd = shaped(256, "gauss")
    for sub in (0, 1, 2):
        worst = 0.0
        for nobj in EB.ROW_NVALID:
            x = EB.small_mlp_input(sub, 50 + nobj)
            dx = guards.guarded(torch.from_numpy(x).cuda(), guards.NAN)
            do = guards.guarded(torch.full((x.shape[0], 32, 256), 7.0, device="cuda"), guards.NAN)
            ok(lib, lib.t2l_blk_enc_small_mlp(eng._h, sub, x.shape[0], ctypes.c_void_p(dx.data_ptr()), nobj, ctypes.c_void_p(do.data_ptr())))
            guards.check_halos(dx, do)
            got = do.cpu().numpy()
            for w in range(x.shape[0]):
                val, tol = EB.small_mlp_b(sd, sub, x[w], nobj)
                worst = max(worst, EB.ratio(got[w], val, tol))
                assert not got[w, nobj:].any()
        report("small_mlp", "f32", EB.SMALL_NAMES[sub], worst)
        assert worst < 1.0
    x = guards.guarded(torch.zeros((1, 32, 3), device="cuda"), guards.NAN)
    o = guards.guarded(torch.full((1, 32, 256), 7.0, device="cuda"), guards.NAN)
    px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(o.data_ptr())
    e128, _ = shaped(128, "gauss")
    for args in ((None, 0, 1, px, 4, po), (e128._h, 0, 1, px, 4, po), (eng._h, 3, 1, px, 4, po), (eng._h, 0, 0, px, 4, po), (eng._h, 0, 1, None, 4, po),
                 (eng._h, 0, 1, px, 33, po), (eng._h, 0, 1, px, -1, po), (eng._h, 0, 1, px, 4, None)):
        assert lib.t2l_blk_enc_small_mlp(*args) == -1 and lib.t2l_blk_last_error(), args[1:]
    guards.check_halos(x, o)
    assert bool((o == 7.0).all())  # a refused call launched nothing


def test_the_product_door_refuses_before_it_launches(lib, shaped, engines):
    import torch

    from text2loc_amd.engine import Engine

    eng, _ = shaped(128, "gauss")
    x = guards.guarded(torch.zeros((1, 32, 128), device="cuda"), guards.NAN)
    o = guards.guarded(torch.full((1, 32, 256), 7.0, device="cuda"), guards.NAN)
    px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(o.data_ptr())
    empty = Engine(0, lib=lib)
    try:
        for args in ((None, 0, 3, 0, 0, 1, px, po), (empty._h, 0, 3, 0, 0, 1, px, po), (eng._h, 3, 3, 0, 0, 1, px, po), (eng._h, 0, 8, 0, 0, 1, px, po),
                     (eng._h, 0, 3, 0, 0, 0, px, po), (eng._h, 0, 3, 0, 0, 1, None, po), (eng._h, 0, 3, 0, 0, 1, px, None), (eng._h, 2, 3, 0, 0, 1, px, po),
                     (eng._h, 0, 3, 2, 0, 1, px, po), (eng._h, 0, 5, 0, 2, 1, px, po), (eng._h, 0, 6, 0, 4, 1, px, po), (eng._h, 1, 7, 0, 0, 1, px, po),
                     (eng._h, 0, 7, 0, 3, 1, px, po)):
            assert lib.t2l_blk_encs_product(*args) == -1 and lib.t2l_blk_last_error(), args[1:6]
    finally:
        empty.close()
    guards.check_halos(x, o)
    assert bool((o == 7.0).all())  # a refused call launched nothing


def test_the_row_doors_refuse_before_they_launch(lib):
    import torch

    x = guards.guarded(torch.full((1, 32, 256), 7.0, device="cuda"), guards.NAN)
    p = ctypes.c_void_p(x.data_ptr())
    for rc in (lib.t2l_blk_enc_normalize(0, p, 4), lib.t2l_blk_enc_normalize(1, None, 4), lib.t2l_blk_enc_normalize(1, p, 33), lib.t2l_blk_enc_normalize(1, p, -1),
               lib.t2l_blk_encs_rows(2, 256, 1, p, None, None, 4), lib.t2l_blk_encs_rows(0, 192, 1, p, None, None, 4), lib.t2l_blk_encs_rows(0, 256, 0, p, None, None, 4),
               lib.t2l_blk_encs_rows(0, 256, 1, None, None, None, 4), lib.t2l_blk_encs_rows(0, 256, 1, p, None, None, 33), lib.t2l_blk_encs_rows(1, 256, 1, p, None, p, 0),
               lib.t2l_blk_encs_rows(1, 256, 1, p, p, None, 0)):
        assert rc == -1 and lib.t2l_blk_last_error()
    guards.check_halos(x)
    assert bool((x == 7.0).all())  # a refused call launched nothing


# ---- the wrapper refuses what is outside its contract -----------------------------------------------------------------------------
def test_the_wrapper_refuses_before_it_launches(lib, engines):
    import torch

    from text2loc_amd.engine import Engine

    eng, _ = engines(("cell", "gauss"))
    teng, _ = engines(("text", 128, 4, "gauss"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = [guards.guarded(torch.zeros((1, 2, 32, 256), dtype=torch.float16, device="cuda"), guards.NAN) for _ in range(2)]
    o = [guards.guarded(torch.full((1, 2, 32, 256), 7.0, dtype=torch.float16, device="cuda"), guards.NAN) for _ in range(2)]
    bad = guards.guarded(torch.full((1,), -1, dtype=torch.int32, device="cuda"), 7)
    call = lambda h, inst, arm, n_wg, layer, S, last, xs=x, tap=None, os_=o, f=None, b=bad: lib.t2l_blk_enc_layer(
        h, inst, arm, n_wg, layer, S, last, p(xs[0]) if xs else None, p(xs[1]) if xs else None, tap, None, None, None, None, None,
        p(os_[0]) if os_ else None, p(os_[1]) if os_ else None, f, p(b) if b is not None else None)
    empty = Engine(0, lib=lib)
    try:
        for args, kw, msg in (((None, 0, 1, 1, 0, 0, 0), {}, b"no context"), ((eng._h, 2, 1, 1, 0, 0, 0), {}, b"inst 0 / 1"),
                              ((eng._h, 0, 0, 1, 0, 0, 0), {}, b"arm 1"), ((eng._h, 0, 3, 1, 0, 0, 0), {}, b"arm 1"),
                              ((eng._h, 0, 1, 0, 0, 0, 0), {}, b"n_wg"), ((eng._h, 0, 1, 1, 0, 0, 2), {}, b"last_to_f32"),
                              ((eng._h, 0, 1, 1, 2, 0, 0), {}, b"no such layer"), ((eng._h, 0, 1, 1, -1, 0, 0), {}, b"no such layer"),
                              ((eng._h, 0, 1, 1, 0, 6, 0), {}, b"has no S"), ((eng._h, 0, 1, 1, 0, 0, 0), {"xs": None}, b"null x"),
                              ((eng._h, 0, 1, 1, 0, 0, 0), {"b": None}, b"null x"), ((eng._h, 0, 1, 1, 0, 0, 0), {"tap": p(o[0])}, b"both planes"),
                              ((eng._h, 0, 1, 1, 0, 0, 0), {"os_": None}, b"null result"), ((eng._h, 0, 1, 1, 0, 0, 1), {}, b"null result"),
                              ((empty._h, 0, 1, 1, 0, 0, 0), {}, b"not loaded"), ((empty._h, 1, 1, 1, 0, 6, 0), {}, b"no text head"),
                              ((eng._h, 1, 1, 1, 0, 6, 0), {}, b"no text head"), ((teng._h, 1, 1, 1, 1, 6, 0), {}, b"one inter layer"),
                              ((teng._h, 1, 1, 1, 0, 0, 0), {}, b"1 <= S <= 32"), ((teng._h, 1, 1, 1, 0, 33, 0), {}, b"1 <= S <= 32")):
            assert call(*args, **kw) == -1 and msg in lib.t2l_blk_last_error(), (args[1:], kw.keys(), lib.t2l_blk_last_error())
        assert lib.t2l_blk_enc_probe(None, None, None, None, 4) == -1
    finally:
        empty.close()
    guards.check_halos(*x, *o, bad)
    assert all(bool((t == 7.0).all()) for t in o) and int(bad[0]) == -1  # a refused call launched nothing
