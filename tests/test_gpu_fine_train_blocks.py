"""GPU tier of the fine-stage training-block tests: the nine kernels csrc/fine_train.hip brings of its own, one launch at a time through
the dev library (csrc/fine_train_blocks.hip), every element of every output against the float64 references and derived bounds of
tests/fine_train_blocks.py; then the wiring of the step — every saved activation of the product's own forward against the stage
reference fed the kernel's own saved predecessors, and one call of the product's dec_bwd per layer.

Inputs and outputs are carved between NaN halos (tests/guards.py); inputs are verified unwritten. Each test prints
`FTBLOCK stage case worst-err/tol` lines (pytest -s); the MI355X figures are in profiles/fine_train_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import fine_train_blocks as B
from tests import guards

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 5
PS = (0.0, B.P_DROP)


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return B.load_blocks()


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


def report(stage, case, r):
    print(f"FTBLOCK {stage} {case} {r:.4g}")
    return r


class Mat:
    """A [rows, w] matrix on the device between NaN halos. ``wide``: it is the middle third of a [rows, 3 w] buffer whose other columns
    hold NaN (an input read outside its view poisons the result; an output written outside it changes them). int32 for index arrays."""

    def __init__(self, a, wide=False, dtype=F32):
        import torch

        a = np.atleast_2d(np.asarray(a))
        self.w = a.shape[1]
        self.off, self.ld = (self.w, 3 * self.w) if wide else (0, self.w)
        self.host = np.full((a.shape[0], self.ld), np.nan if dtype is F32 else 0, dtype)
        self.host[:, self.off:self.off + self.w] = a
        self.t = guards.guarded(torch.from_numpy(self.host).cuda(), guards.NAN if dtype is F32 else 0)

    def ptr(self, elems=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (self.off + elems))

    def get(self):
        """the view as float64 (the columns outside it must hold what they held)"""
        full = self.t.cpu().numpy()
        out = np.ones(self.ld, bool)
        out[self.off:self.off + self.w] = False
        assert np.array_equal(full[:, out], self.host[:, out], equal_nan=True), "written outside the view"
        return full[:, self.off:self.off + self.w].astype(np.float64)

    def unwritten(self):
        return np.array_equal(self.t.cpu().numpy(), self.host, equal_nan=True)

    def freeze(self):
        """an output that becomes the next call's input: from now on it must keep what it holds"""
        self.host = self.t.cpu().numpy().copy()


def settle(inputs, outputs):
    guards.check_halos(*[m.t for m in inputs + outputs])
    assert all(m.unwritten() for m in inputs), "an input was written"


# ---- products ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", B.ROWS)
def test_products(lib, M):
    """lin_fwd (bias, ReLU, no bias), lin_dx (written / added to), lin_dw (dW and db added to non-zero contents, either one null; the
    k / v slice of a [384, 128] tensor leaves rows 0..127 alone) at every width, contiguous and inside a three times wider buffer"""
    worst = {}
    for N, K, sliced in B.WIDTHS:
        c = B.LinCase(M, N, K, sliced)
        o = B.SLICE_ROWS if sliced else 0
        for wide in (False, True):
            tag = f"N={N} K={K}{' slice' if sliced else ''}{' wide' if wide else ''}"
            X, dY, W, b = Mat(c.X, wide), Mat(c.dY, wide), Mat(c.Wfull), Mat(c.bfull)
            for bias, relu in ((True, 0), (True, 1), (False, 0)):
                Y = Mat(np.full((M, N), np.nan), wide)
                ok(lib, lib.t2l_blk_ft_lin_fwd(X.ptr(), X.ld, M, K, W.ptr(o * K), K, b.ptr(o) if bias else None, N, Y.ptr(), Y.ld, relu))
                settle([X, W, b], [Y])
                worst[f"fwd {tag} bias={int(bias)} relu={relu}"] = B.ratio(Y.get(), *B.lin_fwd_ref(c, bias=bias, relu=bool(relu)))
            for acc in (0, 1):
                dX = Mat(c.dX0, wide)
                ok(lib, lib.t2l_blk_ft_lin_dx(dY.ptr(), dY.ld, M, N, W.ptr(o * K), K, K, dX.ptr(), dX.ld, acc))
                settle([dY, W], [dX])
                worst[f"dx {tag} acc={acc}"] = B.ratio(dX.get(), *B.lin_dx_ref(c, acc))
            ref = B.lin_dw_ref(c)
            for want_w, want_b in ((True, True), (True, False), (False, True)):
                dW, db = Mat(c.dW0full), Mat(c.db0full)
                ok(lib, lib.t2l_blk_ft_lin_dw(dY.ptr(), dY.ld, X.ptr(), X.ld, M, N, K, dW.ptr(o * K) if want_w else None, K,
                                              db.ptr(o) if want_b else None))
                settle([dY, X], [dW, db])
                gw, gb = dW.get(), db.get()[0]
                assert np.array_equal(gw[:o], c.dW0full[:o]) and np.array_equal(gb[:o], c.db0full[:o])  # the rows in front of the slice
                if want_w:
                    worst[f"dw {tag} db={int(want_b)}"] = B.ratio(gw[o:], *ref["dW"])
                else:
                    assert np.array_equal(gw, c.dW0full)
                if want_b:
                    worst[f"db {tag} dw={int(want_w)}"] = B.ratio(gb[o:], *ref["db"])
                else:
                    assert np.array_equal(gb, c.db0full)
    for kind in ("fwd", "dx", "dw", "db"):
        k = max((k for k in worst if k.startswith(kind + " ")), key=worst.get)
        report(f"lin_{kind}", f"M={M} {k[len(kind) + 1:]}", worst[k])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", B.BN_ROWS)
def test_batchnorm(lib, M):
    """k_bn_fwd / k_bn_bwd: plain columns, |mean| = 100 std, exactly constant columns; running buffers and dg / db given and null; the
    backward's ReLU mask is the ``out`` it is handed (zeros in about half of it, independent of dout)"""
    worst = {}
    for N in B.BN_COLS:
        for kind in ("plain", "offset", "constant"):
            for full in (True, False):
                if not full and kind != "plain":
                    continue
                Y0, g, b, rm, rv = B.bn_case(M, N, kind)
                Y, G, Bt = Mat(Y0), Mat(g), Mat(b)
                RM, RV = (Mat(rm), Mat(rv)) if full else (None, None)
                rstd, out = Mat(np.full(N, np.nan)), Mat(np.full((M, N), np.nan))
                ok(lib, lib.t2l_blk_ft_bn_fwd(Y.ptr(), M, N, G.ptr(), Bt.ptr(), RM.ptr() if full else None, RV.ptr() if full else None,
                                              rstd.ptr(), out.ptr()))
                settle([G, Bt], [Y, rstd, out] + ([RM, RV] if full else []))
                ref = B.bn_fwd_ref(Y0, g, b, rm if full else None, rv if full else None)
                got = {"xhat": Y.get(), "out": out.get(), "rstd": rstd.get()[0]}
                if full:
                    got.update(rm=RM.get()[0], rv=RV.get()[0])
                assert set(got) == set(ref)
                for k in ref:
                    worst[f"fwd {k} N={N} {kind} run={int(full)}"] = B.ratio(got[k], *ref[k])
                dout, o, xh, rs, g, dg0, db0 = B.bn_bwd_case(M, N, kind)
                ins = [Mat(a) for a in (dout, o, xh, rs, g)]
                DG, DB, dy = Mat(dg0), Mat(db0), Mat(np.full((M, N), np.nan))
                ok(lib, lib.t2l_blk_ft_bn_bwd(*[m.ptr() for m in ins], M, N, DG.ptr() if full else None, DB.ptr() if full else None, dy.ptr()))
                settle(ins, [DG, DB, dy])
                ref = B.bn_bwd_ref(dout, o, xh, rs, g, dg0 if full else None, db0 if full else None)
                got = {"dy": dy.get(), "dg": DG.get()[0], "db": DB.get()[0]}
                if not full:
                    assert DG.unwritten() and DB.unwritten()
                for k in ref:
                    worst[f"bwd {k} N={N} {kind} grads={int(full)}"] = B.ratio(got[k], *ref[k])
    for kind in ("fwd", "bwd"):
        k = max((k for k in worst if k.startswith(kind + " ")), key=worst.get)
        report(f"bn_{kind}", f"M={M} {k[4:]}", worst[k])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq,Tk", B.ATTN_SHAPES)
def test_attention(lib, Tq, Tk):
    """k_attn_fwd / k_attn_bwd at 1 and 3 pairs, p = 0 and 0.1, in the product's two layouts: packed qkv (row stride 384; Tq == Tk) and
    q at stride 128 with k / v at stride 256. The backward is fed the forward kernel's own P."""
    worst = {}
    for pairs in B.ATTN_PAIRS:
        Q, K, V, dO = B.attn_case(pairs, Tq, Tk)
        for p in PS:
            for packed in ((True, False) if Tq == Tk else (False,)):
                tag = f"pairs={pairs} p={p:.1f} {'packed' if packed else 'q+kv'}"
                if packed:
                    A = Mat(np.concatenate([Q, K, V], axis=1))
                    src = [(A, 0), (A, 128), (A, 256)]
                    G = Mat(np.full((pairs * Tq, 384), np.nan))
                    dst = [(G, 0), (G, 128), (G, 256)]
                else:
                    Aq, Akv = Mat(Q), Mat(np.concatenate([K, V], axis=1))
                    src = [(Aq, 0), (Akv, 0), (Akv, 128)]
                    Gq, Gkv = Mat(np.full((pairs * Tq, 128), np.nan)), Mat(np.full((pairs * Tk, 256), np.nan))
                    dst = [(Gq, 0), (Gkv, 0), (Gkv, 128)]
                qkv = [x for m, o in src for x in (m.ptr(o), m.ld)]
                Pm, Om, dOm = Mat(np.full((pairs * 4 * Tq, Tk), np.nan)), Mat(np.full((pairs * Tq, 128), np.nan)), Mat(dO)
                ok(lib, lib.t2l_blk_ft_attn_fwd(*qkv, Tq, Tk, pairs, Pm.ptr(), Om.ptr(), Om.ld, SEED, 2, p))
                ins = list({id(m): m for m, _ in src}.values())
                settle(ins, [Pm, Om])
                f = B.attn_factor(SEED, 2, p, pairs, Tq, Tk)
                ref, spread = B.xattn_fwd_ref(Q, K, V, pairs, Tq, Tk, f)
                assert spread <= B.LOGIT_RANGE
                Pk = Pm.get().reshape(pairs, 4, Tq, Tk)
                Pm.freeze()
                worst[f"fwd P {tag}"], worst[f"fwd O {tag}"] = B.ratio(Pk, *ref["P"]), B.ratio(Om.get(), *ref["O"])
                ok(lib, lib.t2l_blk_ft_attn_bwd(*qkv, Pm.ptr(), dOm.ptr(), dOm.ld, *[x for m, o in dst for x in (m.ptr(o), m.ld)], Tq, Tk, pairs,
                                                SEED, 2, p))
                outs = list({id(m): m for m, _ in dst}.values())
                settle(ins + [Pm, dOm], outs)
                refb = B.xattn_bwd_ref(Q, K, V, Pk, dO, pairs, Tq, Tk, f)
                for (m, o), k in zip(dst, ("dQ", "dK", "dV")):
                    worst[f"bwd {k} {tag}"] = B.ratio(m.get()[:, o:o + 128], *refb[k])
    for kind in ("fwd", "bwd"):
        k = max((k for k in worst if k.startswith(kind + " ")), key=worst.get)
        report(f"attn_{kind}", f"Tq={Tq} Tk={Tk} {k[4:]}", worst[k])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- gather / scatter / num_in ------------------------------------------------------------------------------------------------------------
def test_gather_scatter_num_in(lib):
    """indices 0 (padding: the row is read, gets no gradient), negative, == rows, beyond, and one heavily duplicated row"""
    rows = 23
    table = B.gauss((1, 2), rows, 128)
    once = twice = True  # bit-equal to the exact quotient rounded once / to the two float32 operations
    worst = 0.0
    for M in (1, 16, 272, 513):
        idx = B.index_case(M, rows)
        T, I, out = Mat(table), Mat(idx, dtype=np.int32), Mat(np.full((M, 128), np.nan))
        ok(lib, lib.t2l_blk_ft_gather(T.ptr(), rows, I.ptr(), M, out.ptr()))
        settle([T, I], [out])
        assert np.array_equal(out.get(), B.gather_ref(table, idx)), M
        dY, g0 = B.gauss((3, M), M, 128), B.gauss((4, M), rows, 128)
        Dy, G = Mat(dY), Mat(g0)
        ok(lib, lib.t2l_blk_ft_scatter_add(Dy.ptr(), rows, I.ptr(), M, G.ptr()))
        settle([Dy, I], [G])
        report("scatter_add", f"M={M} (row {rows // 2} x{int((idx == rows // 2).sum())})", r := B.ratio(G.get(), *B.scatter_ref(dY, idx, g0)))
        assert r <= 1.0
        n = np.random.default_rng(M).integers(25, 60000, M).astype(np.float64)
        Nn, o = Mat(n), Mat(np.full(M, np.nan))
        ok(lib, lib.t2l_blk_ft_num_in(Nn.ptr(), M, o.ptr()))
        settle([Nn], [o])
        ref, tol = B.num_in_ref(n)
        got = o.get()[0]
        once &= np.array_equal(got.astype(F32), ref.astype(F32))
        twice &= np.array_equal(got.astype(F32), (n.astype(F32) - F32(B.NUM_MEAN)) / F32(B.NUM_STD))
        worst = max(worst, B.ratio(got, ref, tol))
        assert worst <= 1.0
    report("num_in", f"bit-equal to the once-rounded quotient: {bool(once)}, to the two float32 operations: {bool(twice)};", worst)


# ---- the step's wiring: every saved activation of the product's forward, one layer's backward -----------------------------------------
FROZEN = {0: ("multihead_attn.in_proj_weight",), 1: ("norm2.weight", "linear1.bias")}  # per cascade layer: tensors bound without a gradient


class Step:
    """One forward of the product on a context made through the blocks library; saved[(layer, field)] float64."""

    def __init__(self, lib, cfg, p):
        import torch

        from text2loc_amd.engine import Engine

        self.lib, self.cfg, self.p = lib, cfg, p
        self.sd, self.inp = B.problem(cfg)
        self.eng = Engine(0, lib=lib)
        self.frozen = {f"{cfg.layers[li][0]}.{n}" for li, names in FROZEN.items() if li < len(cfg.layers) for n in names}
        self.tensors, self.g0 = {}, {}
        for k, v in self.sd.items():
            if k.startswith(("language_encoder.", "object_encoder.pointnet.")) or k.endswith("num_batches_tracked"):
                continue
            t = Mat(np.asarray(v, F32).reshape(1, -1))
            g = None
            if "running_" not in k and k not in self.frozen:
                g = Mat(B.gauss((SEED, 1, len(self.tensors)), 1, t.w))
                self.g0[k] = g.get().reshape(np.asarray(v).shape)
            self.tensors[k] = (t, g)
        bound = {k: (t.t.view(np.asarray(self.sd[k]).shape), None if g is None else g.t.view(np.asarray(self.sd[k]).shape))
                 for k, (t, g) in self.tensors.items()}
        self.eng.fine_train_bind(bound, class_embed=cfg.embed, color_embed=cfg.embed, use_features=cfg.use, num_layers=cfg.L)
        dev = lambda a, fill: guards.guarded(torch.from_numpy(np.ascontiguousarray(a)).cuda(), fill)
        self.packed = {k: dev(self.inp[k], 0 if self.inp[k].dtype.kind == "i" else guards.NAN)
                       for k in ("offsets", "class_idx", "color_idx", "rgb", "center", "n_pts")}
        self.hints = dev(self.inp["hints"], guards.NAN)
        self.pn = None if self.inp["pn"] is None else dev(self.inp["pn"], guards.NAN)
        off = self.eng.fine_train_forward(self.packed, self.pn, self.hints, dropout_p=p, seed=SEED)
        torch.cuda.synchronize()
        self.offsets = off.cpu().numpy().astype(np.float64)
        self.bwd_done, self._saved = False, None

    def field(self, layer, name, cap=None):
        """(rc, array or None, numel) of t2l_blk_ft_saved"""
        n = ctypes.c_int64(-1)
        rc = self.lib.t2l_blk_ft_saved(self.eng._h, layer, name.encode(), None, 0, ctypes.byref(n))
        if rc != 0:
            return rc, None, n.value
        dst = Mat(np.zeros(n.value), dtype=np.int32 if name == "arg" else F32)
        rc = self.lib.t2l_blk_ft_saved(self.eng._h, layer, name.encode(), dst.ptr(), n.value if cap is None else cap, ctypes.byref(n))
        guards.check_halos(dst.t)
        return rc, (dst.get()[0] if name != "arg" else dst.t.cpu().numpy()[0]), n.value

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def steps(lib):
    made = {}

    def get(ci, p):
        if (ci, p) not in made:
            made[(ci, p)] = Step(lib, B.CONFIGS[ci], p)
        return made[(ci, p)]

    yield get
    for s in made.values():
        s.close()


def saved_of(lib, st):
    """{key: float64 array} of every field the references name, in the references' shapes"""
    if st._saved is not None:
        return st._saved
    cfg = st.cfg
    shapes = B.forward_chain(cfg, st.sd, st.inp, SEED, st.p)  # (chained: for the key list and the shapes only)
    saved = st._saved = {}
    for (layer, name), (ref, _) in shapes.items():
        if name == "offsets":
            saved[(layer, name)] = st.offsets
        elif name.startswith("run:"):
            saved[(layer, name)] = st.tensors[name[4:]][0].get()[0]
        else:
            rc, a, n = st.field(layer, name)
            ok(lib, rc)
            assert n == np.asarray(ref).size, (layer, name, n, np.asarray(ref).shape)  # the size the product planned
            saved[(layer, name)] = a.reshape(np.asarray(ref).shape)
    return saved


@pytest.mark.parametrize("p", PS, ids=("p0", "p01"))
@pytest.mark.parametrize("ci", range(len(B.CONFIGS)))
def test_forward_chain(lib, steps, ci, p):
    """every saved field, the offsets and the running buffers against the float64 stage reference fed the kernel's own predecessors"""
    st = steps(ci, p)
    cfg = st.cfg
    saved = saved_of(lib, st)
    refs = B.forward_chain(cfg, st.sd, st.inp, SEED, p, saved=saved)
    assert set(refs) == set(saved)
    worst = {k: B.ratio(saved[k], *refs[k]) for k in refs}
    for layer in range(-1, len(cfg.layers)):
        k = max((k for k in worst if k[0] == layer), key=worst.get)
        report("chain", f"{cfg} p={p:.1f} layer={layer} {k[1]}", worst[k])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad
    assert np.array_equal(saved[(-1, "arg")], refs[(-1, "arg")][0]) and saved[(-1, "arg")].dtype == np.int32
    guards.check_halos(*st.packed.values(), st.hints, *([st.pn] if st.pn is not None else []))
    for k, (t, g) in st.tensors.items():
        if "running_" not in k:
            assert t.unwritten(), k  # a forward writes no parameter
        assert g is None or st.bwd_done or g.unwritten(), k  # ... and no gradient
    # a field this configuration does not have is refused
    absent = [(-1, "class.raw") if not cfg.embed else (-1, "class.0.out"), (-1, "pn_only.out") if not cfg.pn_stats else (-1, "class.nrm"),
              (-1, "num.raw"), (0, "nope"), (len(cfg.layers), "qkv"), (-2, "E")]
    for layer, name in absent:
        assert st.field(layer, name)[0] == -1, (layer, name)
    assert st.field(0, "qkv", cap=1)[0] == -1 and b"too small" in lib.t2l_blk_last_error()


@pytest.mark.parametrize("p", PS, ids=("p0", "p01"))
@pytest.mark.parametrize("ci", range(len(B.CONFIGS)))
def test_one_layers_backward(lib, steps, ci, p):
    """one call of the product's dec_bwd per cascade layer: dx written, dmem and all parameter gradients added to non-zero contents (a
    frozen tensor has no gradient), under the layer rule per tensor; the in-projection gradients per element"""
    st = steps(ci, p)
    cfg = st.cfg
    saved = saved_of(lib, st)
    worst = {}
    for li, (pre, is_obj, site) in enumerate(cfg.layers):
        frozen = FROZEN.get(li, ())
        args = B.layer_args(cfg, st.sd, st.inp, saved, li, p, SEED, frozen)
        g0 = {n: st.g0[f"{pre}.{n}"] for n in B.DEC_PARAMS if n not in frozen}
        assert set(g0) == set(args[4])
        args = args[:4] + (g0,) + args[5:]
        dout, dmem0 = args[2], args[3]
        Dout, Dx, Dmem = Mat(dout), Mat(np.full(dout.shape, np.nan)), Mat(dmem0)
        ok(lib, lib.t2l_blk_ft_dec_bwd(st.eng._h, li, Dout.ptr(), Dx.ptr(), Dmem.ptr()))
        st.bwd_done = True
        settle([Dout] + [t for k, (t, _) in st.tensors.items() if "running_" not in k],
               [Dx, Dmem] + [t for k, (t, _) in st.tensors.items() if "running_" in k] + [g for _, g in st.tensors.values() if g is not None])
        bounds = B.dec_bwd_bounds(*args)
        got = {"dx": Dx.get(), "dmem": Dmem.get()}
        for n in g0:
            got[n] = st.tensors[f"{pre}.{n}"][1].get().reshape(g0[n].shape)
        got.update({k: got[k[:-3]] for k in bounds if k.endswith("/el")})
        assert set(got) == set(bounds) and len(g0) == 18 - len(frozen)
        for k in bounds:
            worst[f"{pre} {k}"] = B.ratio(got[k], *bounds[k])
        k = max((k for k in worst if k.startswith(pre + " ")), key=worst.get)
        report("dec_bwd", f"{cfg} p={p:.1f} {k}", worst[k])
    for name, (t, g) in st.tensors.items():  # the encoder's and the head's gradients keep their contents
        if g is not None and not name.startswith("cross_"):
            assert g.unwritten(), name
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- the wrappers refuse what is outside their contract ----------------------------------------------------------------------------------
def test_the_wrappers_refuse_before_they_launch(lib):
    a, o = Mat(np.ones((16, 384))), Mat(np.full((16, 384), 7.0))
    i = Mat(np.zeros(16), dtype=np.int32)
    p, q = a.ptr(), o.ptr()
    calls = [
        (lib.t2l_blk_ft_lin_fwd, (None, 128, 16, 128, p, 128, p, 128, q, 128, 0), b"null"),
        (lib.t2l_blk_ft_lin_fwd, (p, 64, 16, 128, p, 128, p, 128, q, 128, 0), b"ldx"),
        (lib.t2l_blk_ft_lin_fwd, (p, 128, 0, 128, p, 128, p, 128, q, 128, 0), b">= 1"),
        (lib.t2l_blk_ft_lin_dx, (p, 128, 16, 128, None, 128, 128, q, 128, 0), b"null"),
        (lib.t2l_blk_ft_lin_dx, (p, 128, 16, 128, p, 128, -1, q, 128, 0), b">= 1"),
        (lib.t2l_blk_ft_lin_dw, (p, 128, p, 128, 16, 128, 128, None, 128, None), b"neither"),
        (lib.t2l_blk_ft_lin_dw, (p, 128, None, 128, 16, 128, 128, q, 128, None), b"without X"),
        (lib.t2l_blk_ft_bn_fwd, (q, 16, 128, p, None, None, None, q, q), b"null"),
        (lib.t2l_blk_ft_bn_fwd, (q, 0, 128, p, p, None, None, q, q), b">= 1"),
        (lib.t2l_blk_ft_bn_bwd, (p, p, p, p, p, 16, 128, None, None, None), b"null"),
        (lib.t2l_blk_ft_attn_fwd, (p, 384, p, 384, p, 384, 17, 1, 1, q, q, 128, 1, 0, 0.0), b"1..16"),
        (lib.t2l_blk_ft_attn_fwd, (p, 384, p, 384, p, 384, 1, 0, 1, q, q, 128, 1, 0, 0.0), b"1..16"),
        (lib.t2l_blk_ft_attn_fwd, (p, 384, p, 384, p, 384, 1, 1, 0, q, q, 128, 1, 0, 0.0), b"pairs"),
        (lib.t2l_blk_ft_attn_fwd, (p, 384, p, 384, p, 384, 1, 1, 1, q, q, 128, 1, 0, 1.0), b"[0, 1)"),
        (lib.t2l_blk_ft_attn_fwd, (p, 64, p, 384, p, 384, 1, 1, 1, q, q, 128, 1, 0, 0.0), b">= 128"),
        (lib.t2l_blk_ft_attn_fwd, (p, 384, None, 384, p, 384, 1, 1, 1, q, q, 128, 1, 0, 0.0), b"null"),
        (lib.t2l_blk_ft_attn_bwd, (p, 384, p, 384, p, 384, p, p, 128, q, 128, q, 128, q, 128, 0, 16, 1, 1, 0, 0.0), b"1..16"),
        (lib.t2l_blk_ft_attn_bwd, (p, 384, p, 384, p, 384, p, p, 128, q, 128, None, 128, q, 128, 1, 1, 1, 1, 0, 0.0), b"null"),
        (lib.t2l_blk_ft_gather, (None, 23, i.ptr(), 16, q), b"without a table"),
        (lib.t2l_blk_ft_gather, (p, 0, i.ptr(), 16, q), b">= 1"),
        (lib.t2l_blk_ft_scatter_add, (p, 23, i.ptr(), 16, None), b"without a table"),
        (lib.t2l_blk_ft_scatter_add, (p, 23, None, 16, q), b"null"),
        (lib.t2l_blk_ft_num_in, (p, 0, q), b">= 1"),
        (lib.t2l_blk_ft_num_in, (None, 16, q), b"null"),
        (lib.t2l_blk_ft_dec_bwd, (None, 0, p, q, q), b"no context"),
    ]
    for fn, args, msg in calls:
        assert fn(*args) == -1 and msg in lib.t2l_blk_last_error(), (fn.__name__, args, lib.t2l_blk_last_error())
    n = ctypes.c_int64(0)
    assert lib.t2l_blk_ft_saved(None, 0, b"qkv", None, 0, ctypes.byref(n)) == -1 and b"no context" in lib.t2l_blk_last_error()
    from text2loc_amd.engine import Engine

    e = Engine(0, lib=lib)  # a context without a bound state / a forward
    assert lib.t2l_blk_ft_saved(e._h, 0, b"qkv", None, 0, ctypes.byref(n)) == -1 and lib.t2l_blk_ft_dec_bwd(e._h, 0, p, q, q) == -1
    e.close()
    guards.check_halos(a.t, o.t, i.t)
    assert a.unwritten() and o.unwritten()  # a refused call launched nothing
