"""CPU half of the encoder-layer block tier (tests/encode_blocks.py; the GPU half is tests/test_gpu_encode_blocks.py): the float64
stage references against the float32 oracle, the float32 selection models against the float64 product of the planes, the fixtures'
own premises (logit spread, selection coverage, the high-mean rows), and the mutant table of profiles/encode_blocks.md: every mutant
is a change of the reference, judged against the bound of the stage it sits in, that stage fed exact inputs (the taps an exact kernel
would leave). `pytest -s` prints one `ENCMUTANT` line per mutant."""
import numpy as np
import pytest

from oracle import t2l_oracle as O
from tests import encode_blocks as EB
from tests import fine_blocks as FB

F32, F64 = np.float32, np.float64
T256 = EB.TEXT[(256, 4)]


def chain(geo, sd, prefixes, x32, vis):
    """x32 float32 [32, D] through the layers, stage values only, each layer fed the float32 rounding of the one before"""
    for p in prefixes:
        xh, xl = EB.split(x32)
        x32 = EB.layer_stages(geo, sd, p, xh, xl, vis, "split", True)["out"][0].astype(F32)
    return x32


# ---- the references are the oracle's layer --------------------------------------------------------------------------------------
def test_the_cell_stages_are_the_oracles_encoder_layers():
    from text2loc_amd import synth

    sd = EB.cell_weights("gauss")
    cells = synth.make_cells(3, seed=12, min_obj=1, max_obj=40)
    _, _, stages = O.encode_cells(cells, sd, True, True, return_stages=True)  # stages [l]: [28, B, 256]
    for b in range(3):
        x = np.zeros((32, 256), F32)
        x[:28] = stages[0][:, b]
        x[28:] = 0.3  # dead rows: no key
        for l in range(2):
            x = chain(EB.CELL, sd, [EB.CELL_PREFIX.format(l)], x, EB.vis_cell())
            err = np.abs(x[:28] - stages[l + 1][:, b]).max()
            assert err < 2e-5 * max(1.0, np.abs(stages[l + 1]).max()), (b, l, err)


@pytest.mark.parametrize("shape", sorted(EB.TEXT))
def test_the_text_stages_are_the_oracles_encoder_layer(shape):
    D, heads = shape
    geo = EB.TEXT[shape]
    sd = EB.text_weights(D, heads)
    for S in (1, 5, 32):
        sent, n_desc = EB.text_sentences(D, S, 3, n_wg=1)
        x = EB.text_pack(sent, n_desc, S)
        y = np.stack([chain(geo, sd, [EB.TEXT_PREFIX], x[0, t], EB.vis_text(S)) for t in range(2)])[None]
        got = EB.text_unpack_max(y, sent, n_desc, S)
        xs = np.ascontiguousarray(sent.reshape(n_desc, S, D).transpose(1, 0, 2))
        ref = (xs + O.encoder_layer(xs, sd, EB.TEXT_PREFIX, heads)).max(axis=0)
        assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), (shape, S)


def test_the_probe_constants_are_no_larger_than_the_imported_bounds_assume():
    assert all(EB.PROBE[k] <= getattr(FB, k) for k in EB.PROBE)


# ---- the fixtures' premises -----------------------------------------------------------------------------------------------------------
def test_the_visible_logits_stay_inside_the_softmax_bounds_range():
    sd = EB.cell_weights("gauss")
    for layer, x in ((0, EB.cell_tiles(1)), (0, EB.cell_tiles(2, second_zero=True)), (1, EB.cell_tiles_wide(3)), (1, EB.cell_tiles_wide(4))):
        for t in range(2):
            assert EB.logit_spread(EB.CELL, x[0, t].astype(F64), sd, EB.CELL_PREFIX.format(layer), EB.vis_cell()) < FB.LOGIT_RANGE
    for (D, heads), geo in EB.TEXT.items():
        sd = EB.text_weights(D, heads)
        for S in EB.TEXT_S:
            sent, n_desc = EB.text_sentences(D, S, 10 + S)
            x = EB.text_pack(sent, n_desc, S)
            worst = max(EB.logit_spread(geo, x[w, t].astype(F64), sd, EB.TEXT_PREFIX, EB.vis_text(S)) for w in range(x.shape[0]) for t in range(2))
            assert worst < FB.LOGIT_RANGE, (D, heads, S, worst)
    # the selection fixtures keep Gaussian q and k blocks: their attention taps are held to the same softmax bound
    for kind in ("sel", "tilt", "mean", "small"):
        sd, scale = EB.cell_weights(kind), 0.25 if kind == "mean" else 1.0
        for layer, x in ((0, EB.cell_tiles(5, scale=scale)), (1, EB.cell_tiles_wide(6, scale=scale))):
            for t in range(2):
                assert EB.logit_spread(EB.CELL, x[0, t].astype(F64), sd, EB.CELL_PREFIX.format(layer), EB.vis_cell()) < FB.LOGIT_RANGE
        for (D, heads), geo in EB.TEXT.items():
            sent, n_desc = EB.text_sentences(D, 6, 26, scale=scale)
            x = EB.text_pack(sent, n_desc, 6)
            sd = EB.text_weights(D, heads, kind)
            assert max(EB.logit_spread(geo, x[w, t].astype(F64), sd, EB.TEXT_PREFIX, EB.vis_text(6)) for w in range(x.shape[0]) for t in range(2)) < FB.LOGIT_RANGE


@pytest.mark.parametrize("geo", [EB.CELL] + [EB.TEXT[k] for k in sorted(EB.TEXT)], ids=repr)
def test_a_selection_draws_from_every_k_step(geo):
    """every 32-row output tile draws from every k-step of its product and from both lane halves (K / 16 <= 32 steps); the text layer's
    linear2 at D = 256 (64 steps): the first and the last step of every feed-forward pass in every tile, every step over the tiles"""
    for key, (pi, sign) in EB.selection_of(geo).items():
        K = geo.FF if key == "linear2" else geo.D
        steps = K // 16
        step, half = (pi % (K // 2)) // 8, pi // (K // 2)
        assert pi.min() >= 0 and pi.max() < K and set(np.unique(sign)) == {-1.0, 1.0}
        for t in range(len(pi) // 32):
            s, h = step[32 * t:32 * t + 32], half[32 * t:32 * t + 32]
            assert set(h) == {0, 1}, (key, t)
            if steps <= 32:
                assert set(s) == set(range(steps)), (key, t)
            else:
                per = steps // geo.ffp
                assert {c * per for c in range(geo.ffp)} | {(c + 1) * per - 1 for c in range(geo.ffp)} <= set(s), (key, t)
        assert set(step) == set(range(steps)), key
        if key == "linear2":  # the first and the last step of every pass, in every tile
            per = steps // geo.ffp
            for t in range(len(pi) // 32):
                assert {c * per for c in range(geo.ffp)} | {(c + 1) * per - 1 for c in range(geo.ffp)} <= set(step[32 * t:32 * t + 32])


@pytest.mark.parametrize("arm", EB.ARMS)
def test_the_selection_models_are_the_float64_product_of_the_planes(arm):
    """sel_acc32 == (hi + lo) W^T (plain f16: hi W^T) evaluated in float64 and rounded once — it is exact, so no rounding happens; the
    tilted model sits within its 4 u |x| of the float64 product of the split operands without lo lo"""
    rng = np.random.default_rng(4)
    geo = T256
    sd_sel, sd_tilt = EB.text_weights(256, 4, "sel"), EB.text_weights(256, 4, "tilt")
    for key, K in (("v", 256), ("out_proj", 256), ("linear1", 256), ("linear2", 1024)):
        hi, lo = EB.split((rng.standard_normal((32, K)) * np.exp(rng.uniform(-6, 3, (32, K)))).astype(F32))
        pi, sign = EB.selection_of(geo)[key]
        name = {"v": ".self_attn.in_proj_weight"}.get(key, f".{'self_attn.' if key == 'out_proj' else ''}{key}.weight")
        W = np.asarray(sd_sel[EB.TEXT_PREFIX + name], F64)[512 if key == "v" else 0:]
        a = EB.join64(hi, lo) if arm == "split" else hi.astype(F64)
        assert np.array_equal(EB.sel_acc32(hi, lo, pi, sign, arm).astype(F64), a @ W.T), key
        Wt = np.asarray(sd_tilt[EB.TEXT_PREFIX + name], F32)[512 if key == "v" else 0:]
        wh, wl = EB.split(Wt)
        assert set(np.unique(np.abs(wh.astype(F64)))) == {0.0, 1.0} and set(np.unique(np.abs(wl.astype(F64)))) == {0.0, 2.0 ** -12}
        val, tol = EB.sel_acc64(hi, lo, pi, sign, arm, True)
        h, l, whh, wll = hi.astype(F64), lo.astype(F64), wh.astype(F64), wl.astype(F64)
        prod = h @ whh.T + (h @ wll.T + l @ whh.T if arm == "split" else 0.0)
        assert np.all(np.abs(val - prod) <= tol + 0.0), key


def high_mean_rows(geo, sd, prefix, x32, vis):
    """(|mean| / std of the rows entering LayerNorm 1, of those entering LayerNorm 2) on the reference, smallest over the rows"""
    g = lambda k: np.asarray(sd[prefix + k], F64)
    xh, xl = EB.split(x32)
    st = EB.layer_stages(geo, sd, prefix, xh, xl, vis, "split", True)
    y1 = EB.join64(xh, xl) + FB.linear(st["att"][0], g(".self_attn.out_proj.weight"), g(".self_attn.out_proj.bias"))
    h = np.zeros((32, geo.FF))
    for c in range(geo.ffp):
        h[:, geo.units(c)] = st[f"hid{c}"][0]
    y2 = st["x1"][0] + FB.linear(h, g(".linear2.weight"), g(".linear2.bias"))
    return [float((np.abs(y.mean(axis=1)) / y.std(axis=1)).min()) for y in (y1, y2)]


def test_the_high_mean_fixture_has_rows_a_hundred_deviations_off_zero():
    sd = EB.cell_weights("mean")
    for layer, x in ((0, EB.cell_tiles(5, scale=0.25)), (1, EB.cell_tiles_wide(6, scale=0.25))):
        for t in range(2):
            assert min(high_mean_rows(EB.CELL, sd, EB.CELL_PREFIX.format(layer), x[0, t], EB.vis_cell())) >= 100
    for (D, heads), geo in EB.TEXT.items():
        sd = EB.text_weights(D, heads, "mean")
        for S in (1, 6):
            sent, n_desc = EB.text_sentences(D, S, 20 + S, scale=0.25)
            x = EB.text_pack(sent, n_desc, S)
            assert min(min(high_mean_rows(geo, sd, EB.TEXT_PREFIX, x[w, t], EB.vis_text(S))) for w in range(x.shape[0]) for t in range(2)) >= 100


# ---- the mutant table -----------------------------------------------------------------------------------------------------------------
def sel_ratio(geo, sd, prefix, x32, vis, arm, stage, what, tilt=False, S=None, last=False):
    """worst |mutant - model| / bound of ``stage`` on selection weights, the stage fed the taps an exact kernel would leave; a stage
    demanded bit for bit is judged against the smallest bound any stage has, one split's max(2^-22 |v|, 2^-25)"""
    xh, xl = EB.split(x32)
    taps = EB.reference_taps(geo, sd, prefix, xh, xl, vis, arm)
    clean = EB.selection_stages(geo, sd, prefix, xh, xl, taps, arm, last, tilt=tilt, S=S)
    mut = EB.selection_stages(geo, sd, prefix, xh, xl, taps, arm, last, tilt=tilt, S=S, mut=(stage, what))
    how, ref, tol = clean[stage]
    got = mut[stage][1]
    if how == "bits":
        ref, got = EB.join64(*ref), EB.join64(*got)
    if how == "bits" or not np.any(tol):  # (the S = 1 attention tap is demanded as a value: bound 0)
        tol = np.maximum(2.0 ** -22 * np.abs(ref), 2.0 ** -25)
    return EB.ratio(got, ref, tol)


def gauss_ratio(geo, sd, prefix, x32, vis, arm, stage, mut=None, vis_mut=None):
    xh, xl = EB.split(x32)
    taps = EB.reference_taps(geo, sd, prefix, xh, xl, vis, arm)
    clean = EB.layer_stages(geo, sd, prefix, xh, xl, vis, arm, False, taps=taps)
    m = EB.layer_stages(geo, sd, prefix, xh, xl, vis, arm, False, taps=taps, mut=mut, vis_mut=vis_mut)
    return EB.ratio(m[stage][0], clean[stage][0], clean[stage][1])


def test_the_mutant_table():
    rows = []
    sent1, n1 = EB.text_sentences(256, 1, 21, n_wg=1)
    x_s1 = EB.text_pack(sent1, n1, 1)[0, 0]
    sent6, n6 = EB.text_sentences(256, 6, 26, n_wg=1)
    x_s6 = EB.text_pack(sent6, n6, 6)[0, 0]
    xc0, xc1 = EB.cell_tiles(5)[0, 0], EB.cell_tiles_wide(6)[0, 0]
    sel_t, tilt_t = EB.text_weights(256, 4, "sel"), EB.text_weights(256, 4, "tilt")
    sel_c, tilt_c, mean_c, small_c = EB.cell_weights("sel"), EB.cell_weights("tilt"), EB.cell_weights("mean"), EB.cell_weights("small")
    gauss_c, gauss_t = EB.cell_weights("gauss"), EB.text_weights(256, 4, "gauss")
    P0, P1, PT = EB.CELL_PREFIX.format(0), EB.CELL_PREFIX.format(1), EB.TEXT_PREFIX
    vc, v1, v6 = EB.vis_cell(), EB.vis_text(1), EB.vis_text(6)
    add = lambda name, r, asserted=True: rows.append((name, r, asserted))

    # a dropped lo plane, activation side (selection) and weight side (tilted selection), in the four chosen products
    add("act lo dropped: v projection (text S = 1)", sel_ratio(T256, sel_t, PT, x_s1, v1, "split", "att", "act_lo", S=1))
    add("act lo dropped: out_proj (cell layer 1)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "x1", "act_lo"))
    add("act lo dropped: linear1 (cell layer 1)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "hid1", "act_lo"))
    add("act lo dropped: linear2 (cell layer 1)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "out", "act_lo"))
    add("act lo dropped: linear2 (text S = 6)", sel_ratio(T256, sel_t, PT, x_s6, v6, "split", "out", "act_lo"))
    add("weight lo dropped: v projection (text S = 1)", sel_ratio(T256, tilt_t, PT, x_s1, v1, "split", "att", "w_lo", tilt=True, S=1))
    add("weight lo dropped: out_proj (cell layer 1)", sel_ratio(EB.CELL, tilt_c, P1, xc1, vc, "split", "x1", "w_lo", tilt=True))
    add("weight lo dropped: linear1 (cell layer 1)", sel_ratio(EB.CELL, tilt_c, P1, xc1, vc, "split", "hid0", "w_lo", tilt=True))
    add("weight lo dropped: linear2 (cell layer 1)", sel_ratio(EB.CELL, tilt_c, P1, xc1, vc, "split", "out", "w_lo", tilt=True))
    # wiring
    add("last k-step dropped: linear1 (cell layer 1)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "hid1", "kstep"))
    add("last k-step dropped: linear2 (text S = 6)", sel_ratio(T256, sel_t, PT, x_s6, v6, "split", "out", "kstep"))
    add("last k-step dropped: out_proj (cell layer 0, Gaussian)", gauss_ratio(EB.CELL, gauss_c, P0, xc0, vc, "split", "x1", "kstep:out_proj"))
    add("a pass reads the other pass's hidden units (cell)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "out", "pass_swap"))
    add("a pass reads the other pass's hidden units (text)", sel_ratio(T256, sel_t, PT, x_s6, v6, "split", "out", "pass_swap"))
    add("bias slice of the neighbouring tile (cell)", sel_ratio(EB.CELL, sel_c, P1, xc1, vc, "split", "hid0", "bias_tile"))
    add("bias slice of the neighbouring tile (text, Gaussian)", gauss_ratio(T256, gauss_t, PT, x_s6, v6, "split", "hid3", "bias_tile"))
    add("head 0's output in head 1's columns (cell)", gauss_ratio(EB.CELL, gauss_c, P0, xc0, vc, "split", "att", "head_cols"))
    add("head 0's output in head 1's columns (text)", gauss_ratio(T256, gauss_t, PT, x_s6, v6, "split", "att", "head_cols"))
    add("key mask j <= 28 (cell)", gauss_ratio(EB.CELL, gauss_c, P0, xc0, vc, "split", "att", vis_mut=EB.vis_cell("mask_le")))
    add("a query sees the neighbouring description's keys (text S = 6)",
        gauss_ratio(T256, gauss_t, PT, x_s6, v6, "split", "att", vis_mut=EB.vis_text(6, "neighbour")))
    # LayerNorm
    xm = EB.cell_tiles_wide(6, scale=0.25)[0, 0]
    add("one-pass variance: LayerNorm 1 (high-mean rows)", sel_ratio(EB.CELL, mean_c, P1, xm, vc, "split", "x1", "ln_onepass"))
    add("one-pass variance: LayerNorm 2 (high-mean rows)", sel_ratio(EB.CELL, mean_c, P1, xm, vc, "split", "out", "ln_onepass", last=True))
    add("LayerNorm eps 1e-6: LayerNorm 1 (cell layer 0)", sel_ratio(EB.CELL, sel_c, P0, xc0, vc, "split", "x1", "ln_eps"))
    add("LayerNorm eps 1e-6: LayerNorm 2 (cell layer 0, small first LayerNorm)", sel_ratio(EB.CELL, small_c, P0, xc0, vc, "split", "out", "ln_eps", last=True))
    # behind the softmax: reported, asserted only where they reach 2. The case: a second layer's rows scaled until the visible logits
    # spread as far as the bound allows (just inside FB.LOGIT_RANGE)
    scale, spread = 1.0, 0.0
    for s in np.arange(1.0, 12.0, 0.25):
        sp = EB.logit_spread(EB.CELL, (s * xc1).astype(F64), gauss_c, P1, vc)
        if sp >= FB.LOGIT_RANGE:
            break
        scale, spread = s, sp
    xq = (scale * xc1).astype(F32)
    rq = gauss_ratio(EB.CELL, gauss_c, P1, xq, vc, "split", "att", "act_lo:q")
    rk = gauss_ratio(EB.CELL, gauss_c, P1, xq, vc, "split", "att", "act_lo:k")
    add(f"act lo dropped: q projection (rows x {scale:g}, logit spread {spread:.1f})", rq, rq >= 2)
    add(f"act lo dropped: k projection (rows x {scale:g}, logit spread {spread:.1f})", rk, rk >= 2)
    for name, lo_mut in (("v projection", "act_lo:v"), ("out_proj", "act_lo:out_proj"), ("linear1", "act_lo:linear1"), ("linear2", "act_lo:linear2")):
        stage = {"act_lo:v": "att", "act_lo:out_proj": "x1", "act_lo:linear1": "hid0", "act_lo:linear2": "out"}[lo_mut]
        add(f"act lo dropped: {name} (cell layer 1, Gaussian weights)", gauss_ratio(EB.CELL, gauss_c, P1, xc1, vc, "split", stage, lo_mut), False)
    # the row stages outside planes_layer (normalize_rows, normalize_rows_d, layer_norm_rows_d)
    for D in (128, 256):
        x = EB.row_tiles(D, 1)[0]
        g, b = EB.row_gain(D, 1)
        nv, nt = EB.normalize_rows_b(x, 27)
        lv, lt = EB.layer_norm_rows_b(x, g, b)
        add(f"normalise: the row behind the last object normalised too (D = {D})", EB.ratio(EB.normalize_rows_b(x, 27, "nvalid_plus")[0], nv, nt))
        add(f"normalise: the norm over half the columns (D = {D})", EB.ratio(EB.normalize_rows_b(x, 27, "half")[0], nv, nt))
        hm, sv = slice(9, 11), slice(20, 22)  # the high-mean rows, the small-variance rows
        add(f"LayerNorm rows: one-pass variance (D = {D}, rows 1000 sigma off zero)", EB.ratio(EB.layer_norm_rows_b(x, g, b, "ln_onepass")[0][hm], lv[hm], lt[hm]))
        add(f"LayerNorm rows: eps 1e-6 (D = {D}, rows of variance 4e-4)", EB.ratio(EB.layer_norm_rows_b(x, g, b, "ln_eps")[0][sv], lv[sv], lt[sv]))
        add(f"LayerNorm rows: the gain of the neighbouring column (D = {D})", EB.ratio(EB.layer_norm_rows_b(x, g, b, "gain_shift")[0], lv, lt))
    # the products of the one-cell kernel (mm_tiles), mlp_merge among them: selection / tilted weights, exact models
    floor = lambda v: np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)  # a stage demanded exactly is judged against one split's bound
    for D in (128, 256):
        sel, tilt = EB.shaped_weights(D, "sel"), EB.shaped_weights(D, "tilt")
        for label, which, sub in (("mlp_merge slot 2", 6, 2), ("out_proj", 3, 0), ("linear2 pass 1", 5, 1), ("k^T", 1, 0)):
            x = EB.product_input(D, which, 40 + which)[0]
            Ws, _ = EB.product_matrix(sel, D, which, 1, sub)
            Wt, _ = EB.product_matrix(tilt, D, which, 1, sub)
            v, _ = EB.product_b(x, Ws, False, "split")
            vt, tt = EB.product_b(x, Wt, False, "split")
            add(f"mm_tiles {label}: activation lo dropped (D = {D})", EB.ratio(EB.product_b(x, Ws, False, "split", "act_lo")[0], v, floor(v)))
            add(f"mm_tiles {label}: weight lo dropped (D = {D}, tilted)", EB.ratio(EB.product_b(x, Wt, False, "split", "w_lo")[0], vt, tt))
            add(f"mm_tiles {label}: last k-step dropped (D = {D})", EB.ratio(EB.product_b(x, Ws, False, "split", "kstep")[0], v, floor(v)))
            add(f"mm_tiles {label}: the neighbouring output tile (D = {D})", EB.ratio(EB.product_b(x, Ws, False, "split", "tile_swap")[0], v, floor(v)))
        x = EB.product_input(D, 5, 45)[0]
        v = EB.product_b(x, EB.product_matrix(sel, D, 5, 1, 1)[0], False, "split")[0]
        add(f"mm_tiles linear2: pass 1 at pass 0's k offset (D = {D})", EB.ratio(EB.product_b(x, EB.product_matrix(sel, D, 5, 1, 0)[0], False, "split")[0], v, floor(v)))
        x = EB.product_input(D, 6, 46)[0]
        v = EB.product_b(x, EB.product_matrix(sel, D, 6, 0, 1)[0], False, "split")[0]
        add(f"mm_tiles mlp_merge: slot 1 with slot 0's weights (D = {D})", EB.ratio(EB.product_b(x, EB.product_matrix(sel, D, 6, 0, 0)[0], False, "split")[0], v, floor(v)))
    # the feature branches of the two-cell kernel (small_mlp: hidden layer, gemm32, normalize_rows)
    sd256 = EB.shaped_weights(256, "gauss")
    for sub in (0, 2):
        x = EB.small_mlp_input(sub, 51)[0]
        v, t = EB.small_mlp_b(sd256, sub, x, 27)
        add(f"small_mlp {EB.SMALL_NAMES[sub]}: gemm32's last k-step dropped", EB.ratio(EB.small_mlp_b(sd256, sub, x, 27, "kstep")[0], v, t))
        add(f"small_mlp {EB.SMALL_NAMES[sub]}: the row behind the last object kept", EB.ratio(EB.small_mlp_b(sd256, sub, x, 27, "nobj_plus")[0], v, t))
    x = EB.small_mlp_input(2, 51)[0]
    v, t = EB.small_mlp_b(sd256, 2, x, 27)
    add("small_mlp num_encoder: the point count enters raw", EB.ratio(EB.small_mlp_b(sd256, 2, x, 27, "no_num_norm")[0], v, t))
    for name, r, asserted in rows:
        print(f"ENCMUTANT {'asserted' if asserted else 'reported'} {r:.4g} {name}")
    missed = [(n, r) for n, r, a in rows if a and not r >= 2]
    assert not missed, missed


def test_the_row_references_are_the_oracles():
    """normalize_rows_b is the oracle's l2_normalize on the valid rows, layer_norm_rows_b its layer_norm"""
    for D in (128, 256):
        x = EB.row_tiles(D, 2)[1]
        g, b = EB.row_gain(D, 2)
        for nvalid in EB.ROW_NVALID:
            v, _ = EB.normalize_rows_b(x, nvalid)
            assert np.abs(v[:nvalid] - O.l2_normalize(x[:nvalid])).max(initial=0.0) < 1e-6 and not v[nvalid:].any()
        keep = np.r_[0:9, 11:32]  # (the oracle's float32 LayerNorm is itself off on the rows 1000 sigma from zero)
        v, _ = EB.layer_norm_rows_b(x, g, b)
        ref = O.layer_norm(x, g, b)
        assert np.abs(v[keep] - ref[keep]).max() < 2e-5 * max(1.0, np.abs(ref[keep]).max())


def test_the_product_references_are_the_oracles_and_the_selection_is_exact():
    """product_matrix folds mlp_merge as the oracle's mlp does (one slot at a time, summed over the slots); a selection matrix has one
    entry per row and draws from every k-step; its BatchNorm is the identity in float32"""
    for D in (128, 256):
        sd = EB.shaped_weights(D, "gauss")
        rng = np.random.default_rng(D)
        x = rng.standard_normal((5, 4 * D)).astype(F32)
        W, b = EB._fold(sd, "object_encoder.mlp_merge.0.0", "object_encoder.mlp_merge.0.1")
        got = sum(x[:, s * D:(s + 1) * D].astype(F64) @ EB.product_matrix(sd, D, 6, 0, s)[0].T for s in range(4)) + b
        ref = O.mlp(x, sd, "object_encoder.mlp_merge", 1)
        assert np.abs(np.maximum(got, 0.0) - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
        sel = EB.shaped_weights(D, "sel")
        for which, sub in EB.PRODUCTS[:11]:
            Wm, _ = EB.product_matrix(sel, D, which, 1, sub)
            assert (np.count_nonzero(Wm, axis=1) <= 1).all() and set(np.unique(np.abs(Wm))) <= {0.0, 1.0}
            if which != 5:  # (a pass of linear2 sees the rows that pick from its units only)
                assert (np.count_nonzero(Wm, axis=1) == 1).all()
                for t in range(Wm.shape[0] // 32):
                    k = np.nonzero(Wm[32 * t:32 * t + 32])[1]
                    assert set((k % (D // 2)) // 8) == set(range(D // 16)) and set(k // (D // 2)) == {0, 1}, (D, which, t)


def test_the_small_mlp_reference_is_the_oracles_branch():
    sd = EB.shaped_weights(256, "gauss")
    for sub in (0, 1, 2):
        x = EB.small_mlp_input(sub, 3)[0]
        v = x if sub != 2 else ((x - F32(EB.NUM_MEAN)) / F32(EB.NUM_STD)).astype(F32)
        ref = O.l2_normalize(O.mlp(v, sd, "object_encoder." + EB.SMALL_NAMES[sub], 2))
        got, tol = EB.small_mlp_b(sd, sub, x, 32)
        assert np.abs(got - ref).max() < 2e-5 and np.isfinite(tol).all() and tol.max() < 1e-3
