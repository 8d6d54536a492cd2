"""CPU tier of the fine-stage training-block tests: proves the float64 references, the derived bounds and the case lists of
tests/fine_train_blocks.py before a GPU sees them (tests/test_gpu_fine_train_blocks.py; profiles/fine_train_blocks.md).

* the stage references chained reproduce the float64 twin (tests/fine_train_twin.py): offsets, grad_hint, every parameter gradient,
  the running buffers; ``dec_bwd_ref`` on the twin's own intermediates reproduces autograd's layer gradients;
* a float32 numpy run of every reference stays inside its bound on every case (`FTBLOCK-CPU` lines: the worst ratio per stage), and the
  logit-range precondition of the probability bound holds on every fixture;
* mutants: each fault, applied to the reference of the block it lives in, leaves that block's bound on at least one listed case."""
import functools

import numpy as np
import pytest
import torch

from tests import fine_train_blocks as B
from tests import train_blocks as TB
from tests.fine_train_twin import Twin, _drop

F32 = np.float32
SEED = 5
PS = (0.0, B.P_DROP)
CELL_KEYS = ("offsets", "class_idx", "color_idx", "rgb", "center", "n_pts")


def report(stage, case, r):
    print(f"FTBLOCK-CPU {stage} {case} {r:.4g}")
    return r


def relmax(a, b, scale=None):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(float(np.abs(b).max()) if scale is None else scale, 1e-300))


@functools.lru_cache(maxsize=None)
def lin_case(M, N, K, sliced):
    return B.LinCase(M, N, K, sliced)


@functools.lru_cache(maxsize=None)
def chain(ci, p):
    """(cfg, sd, inp, the chained float64 references) of configuration ci"""
    cfg = B.CONFIGS[ci]
    sd, inp = B.problem(cfg)
    return cfg, sd, inp, B.forward_chain(cfg, sd, inp, SEED, p)


# ---- the references are right -----------------------------------------------------------------------------------------------------
@pytest.fixture
def twin_eps(monkeypatch):
    """eps is a parameter of LayerNorm / BatchNorm: the kernels' is 1e-5f (what the references of the tier use), torch's the double 1e-5.
    Through the cancellation of a LayerNorm backward that 2.6e-13 shows at 4e-9 of a gradient's maximum, so the comparison with the
    twin runs the SAME references with the twin's eps."""
    monkeypatch.setattr(TB, "LN_EPS", 1e-5)
    monkeypatch.setattr(B, "BN_EPS", 1e-5)


@pytest.mark.parametrize("p", PS, ids=("p0", "p01"))
@pytest.mark.parametrize("ci", range(len(B.CONFIGS)))
def test_the_chained_stage_references_reproduce_the_twin(ci, p, twin_eps):
    cfg = B.CONFIGS[ci]
    sd, inp = B.problem(cfg)
    off, g, gh, run = B.step_ref(cfg, sd, inp, SEED, p)
    twin = Twin(sd, cfg.embed, cfg.embed, cfg.use, cfg.L)
    off_t, g_t, gh_t, _ = twin.step({k: inp[k] for k in CELL_KEYS}, inp["hints"], inp["gout"], inp["pn"], p, SEED)
    assert relmax(off, off_t) < 1e-9 and relmax(gh, gh_t) < 1e-9
    assert set(g) == set(g_t)
    for n in g:
        scale = None
        if n.startswith("object_encoder.") and n.endswith(".0.bias"):
            # a Linear bias in front of a BatchNorm: the true gradient is 0, both sides hold float64 cancellation noise — held at the size
            # of the BatchNorm bias's gradient
            scale = float(np.abs(g_t[n.replace(".0.bias", ".1.bias")]).max())
        assert relmax(g[n], g_t[n], scale) < 1e-9, n
    moved = {n for n, v in twin.running().items() if not np.array_equal(v, np.asarray(sd[n], np.float64))}
    assert moved == set(run) and moved
    for n in run:
        assert relmax(run[n], twin.running()[n]) < 1e-9, n


class RecTwin(Twin):
    """The twin's decoder layer with its intermediates kept (the same operations in the same order: asserted bit-equal below)."""

    def _mha(self, q_in, kv_in, prefix, p, seed, site):
        w, b = self.t[prefix + ".in_proj_weight"], self.t[prefix + ".in_proj_bias"]
        q = q_in @ w[:128].T + b[:128]
        k = kv_in @ w[128:256].T + b[128:256]
        v = kv_in @ w[256:].T + b[256:]
        heads = lambda a: a.reshape(a.shape[0], a.shape[1], 4, 32).transpose(1, 2)
        a = torch.softmax(heads(q) @ heads(k).transpose(-1, -2) / np.sqrt(32), dim=-1)
        o = (_drop(a, seed, site, p) @ heads(v)).transpose(1, 2).reshape(q_in.shape)
        self.rec.append({"q": q, "k": k, "v": v, "P": a, "o": o})
        return o @ self.t[prefix + ".out_proj.weight"].T + self.t[prefix + ".out_proj.bias"]

    def _ln(self, x, prefix):
        mu = x.mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
        self.rec.append({"xh": (x - mu) * r, "r": r[..., 0]})
        return super()._ln(x, prefix)

    def decoder_layer(self, x, mem, prefix, p, seed, site):
        self.rec = []
        t = self.t
        x1 = self._ln(x + _drop(self._mha(x, x, prefix + ".self_attn", p, seed, site), seed, site + 1, p), prefix + ".norm1")
        x2 = self._ln(x1 + _drop(self._mha(x1, mem, prefix + ".multihead_attn", p, seed, site + 2), seed, site + 3, p), prefix + ".norm2")
        h1 = torch.relu(x2 @ t[prefix + ".linear1.weight"].T + t[prefix + ".linear1.bias"])
        h = _drop(h1, seed, site + 4, p)
        f = h @ t[prefix + ".linear2.weight"].T + t[prefix + ".linear2.bias"]
        self.rec.append({"x1": x1, "x2": x2, "h1": h1, "h1d": h})
        return self._ln(x2 + _drop(f, seed, site + 5, p), prefix + ".norm3")


@pytest.mark.parametrize("p", PS, ids=("p0", "p01"))
@pytest.mark.parametrize("Tq,Tk,pairs", [(16, 5, 3), (1, 16, 1), (8, 16, 2)])
def test_dec_bwd_ref_reproduces_autograd_on_the_twins_intermediates(Tq, Tk, pairs, p, twin_eps):
    sd = B.weights(1, 3)
    pre, site = "cross_objects.0", 12
    rng = np.random.default_rng((Tq, Tk, pairs))
    x64, mem64, dout = rng.standard_normal((pairs, Tq, 128)), rng.standard_normal((pairs, Tk, 128)), rng.standard_normal((pairs * Tq, 128))
    tw = RecTwin(sd, True, True, B.BRANCHES, 1)
    x, mem = torch.tensor(x64, requires_grad=True), torch.tensor(mem64, requires_grad=True)
    out = tw.decoder_layer(x, mem, pre, p, SEED, site)
    plain = Twin(sd, True, True, B.BRANCHES, 1)
    plain.t = tw.t
    assert torch.equal(out, plain.decoder_layer(x, mem, pre, p, SEED, site))
    (out.reshape(pairs * Tq, 128) * torch.tensor(dout)).sum().backward()
    sa, ln1, ca, ln2, mid, ln3 = tw.rec
    n = lambda a: a.detach().numpy()
    rows = lambda a: n(a).reshape(-1, a.shape[-1])
    sv = {"x": rows(x), "mem": rows(mem), "qkv": np.concatenate([rows(sa["q"]), rows(sa["k"]), rows(sa["v"])], axis=1), "Ps": n(sa["P"]),
          "os": rows(sa["o"]), "xh1": rows(ln1["xh"]), "r1": n(ln1["r"]).ravel(), "x1": rows(mid["x1"]), "q2": rows(ca["q"]),
          "kv2": np.concatenate([rows(ca["k"]), rows(ca["v"])], axis=1), "Pc": n(ca["P"]), "oc": rows(ca["o"]), "xh2": rows(ln2["xh"]),
          "r2": n(ln2["r"]).ravel(), "x2": rows(mid["x2"]), "h1": rows(mid["h1"]), "h1d": rows(mid["h1d"]), "xh3": rows(ln3["xh"]),
          "r3": n(ln3["r"]).ravel()}
    W = {k: np.asarray(sd[f"{pre}.{k}"], np.float64) for k in B.DEC_PARAMS}
    dmem0 = rng.standard_normal((pairs * Tk, 128))
    g0 = {k: rng.standard_normal(W[k].shape) for k in B.DEC_PARAMS}
    dx, dmem, grads, _ = B.dec_bwd_ref(sv, W, dout, dmem0, g0, SEED, site, p, pairs, Tq, Tk)
    assert relmax(dx, rows(x.grad)) < 1e-9 and relmax(dmem - dmem0, rows(mem.grad)) < 1e-9
    assert set(grads) == set(B.DEC_PARAMS)
    for k in B.DEC_PARAMS:
        assert relmax(grads[k] - g0[k], n(tw.t[f"{pre}.{k}"].grad)) < 1e-9, k
    del g0["norm2.weight"]  # a frozen tensor: no gradient comes back
    assert "norm2.weight" not in B.dec_bwd_ref(sv, W, dout, dmem0, g0, SEED, site, p, pairs, Tq, Tk)[2]


# ---- the bounds are usable: a float32 numpy run of every reference stays inside ---------------------------------------------------------
@pytest.mark.parametrize("M", B.ROWS)
def test_float32_products_stay_inside_their_bounds(M):
    worst = 0.0
    for N, K, sliced in B.WIDTHS:
        c = lin_case(M, N, K, sliced)
        for relu in (False, True):
            ref, tol = B.lin_fwd_ref(c, relu=relu)
            worst = max(worst, B.ratio(B.f32_lin(c.X, c.W.T, bias=c.b, relu=relu), ref, tol))
        for acc in (0, 1):
            ref, tol = B.lin_dx_ref(c, acc)
            worst = max(worst, B.ratio(B.f32_lin(c.dY, c.W, C0=c.dX0 if acc else None), ref, tol))
        r = B.lin_dw_ref(c)
        worst = max(worst, B.ratio(B.f32_lin(c.dY.T, c.X, C0=c.dW0), *r["dW"]))
        worst = max(worst, B.ratio((c.db0.astype(F32) + c.dY.astype(F32).sum(axis=0, dtype=F32)).astype(np.float64), *r["db"]))
    assert report("products", f"M={M}", worst) <= 1.0


def bn_cases():
    return [(M, N, kind) for M in B.BN_ROWS for N in B.BN_COLS for kind in ("plain", "offset", "constant")]


def test_float32_batchnorm_stays_inside_its_bounds():
    wf = wb = 0.0
    for M, N, kind in bn_cases():
        Y, g, b, rm, rv = B.bn_case(M, N, kind)
        ref, r32 = B.bn_fwd_ref(Y, g, b, rm, rv), B.bn_fwd(Y, g, b, rm, rv, F32)
        wf = max([wf] + [B.ratio(r32[k], *ref[k]) for k in ref])
        args = B.bn_bwd_case(M, N, kind)
        ref, r32 = B.bn_bwd_ref(*args), B.bn_bwd(*args, F32)
        wb = max([wb] + [B.ratio(r32[k], *ref[k]) for k in ref])
    assert report("bn_fwd", "all", wf) <= 1.0 and report("bn_bwd", "all", wb) <= 1.0


def attn_cases():
    return [(pairs, Tq, Tk, p) for Tq, Tk in B.ATTN_SHAPES for pairs in B.ATTN_PAIRS for p in PS]


def test_float32_attention_stays_inside_its_bounds_and_the_logit_range_holds():
    wf = wb = spread = 0.0
    for pairs, Tq, Tk, p in attn_cases():
        Q, K, V, dO = B.attn_case(pairs, Tq, Tk)
        f = B.attn_factor(SEED, 2, p, pairs, Tq, Tk)
        ref, sp = B.xattn_fwd_ref(Q, K, V, pairs, Tq, Tk, f)
        spread = max(spread, sp)
        P32, O32, _ = B.xattn_fwd(Q, K, V, pairs, Tq, Tk, f, F32)
        wf = max(wf, B.ratio(P32, *ref["P"]), B.ratio(O32, *ref["O"]))
        P = ref["P"][0].astype(F32).astype(np.float64)
        refb = B.xattn_bwd_ref(Q, K, V, P, dO, pairs, Tq, Tk, f)
        got = B.xattn_bwd(Q, K, V, P, dO, pairs, Tq, Tk, f, F32)
        wb = max([wb] + [B.ratio(a, *refb[k]) for a, k in zip(got, ("dQ", "dK", "dV"))])
    assert spread <= B.LOGIT_RANGE, spread
    assert report("attn_fwd", f"all (logit spread {spread:.3g})", wf) <= 1.0 and report("attn_bwd", "all", wb) <= 1.0


def test_float32_gather_scatter_num_in():
    table = B.gauss((1, 2), 23, 128)
    for M in (1, 16, 272):
        idx = B.index_case(M, 23)
        assert np.array_equal(B.gather_ref(table, idx)[idx == 23], np.zeros((int((idx == 23).sum()), 128)))
        dY, g0 = B.gauss((3, M), M, 128), B.gauss((4, M), 23, 128)
        ref, tol = B.scatter_ref(dY, idx, g0)
        got = g0.astype(F32)
        for m in range(M):
            if 0 < idx[m] < 23:
                got[idx[m]] += dY[m].astype(F32)
        assert B.ratio(got, ref, tol) <= 1.0 and np.array_equal(ref[0], g0[0])
    n = np.random.default_rng(1).integers(25, 60000, 300).astype(np.float64)
    ref, tol = B.num_in_ref(n)
    got = (n.astype(F32) - F32(B.NUM_MEAN)) / F32(B.NUM_STD)
    assert report("num_in", "300 values", B.ratio(got, ref, tol)) <= 1.0


@pytest.mark.parametrize("p", PS, ids=("p0", "p01"))
@pytest.mark.parametrize("ci", range(len(B.CONFIGS)))
def test_float32_chain_and_layer_backward_stay_inside_their_bounds(ci, p):
    cfg, sd, inp, refs = chain(ci, p)
    # saved tensors as a kernel leaves them: float32 values; both runs are fed those
    saved = {k: v[0].astype(F32).astype(np.float64) if v[0].dtype.kind == "f" else v[0] for k, v in refs.items()}
    refs = B.forward_chain(cfg, sd, inp, SEED, p, saved=saved)
    r32 = B.forward_chain(cfg, sd, inp, SEED, p, saved=saved, dtype=F32)
    worst = {k: B.ratio(r32[k][0], *refs[k]) for k in refs}
    k = max(worst, key=worst.get)
    assert report("chain", f"{cfg} p={p:.1f} {k}", worst[k]) <= 1.0
    assert set(f for (l, f) in refs if l >= 0) == set(B.DEC_FIELDS)
    # the logit range on every attention of the chain
    for li in range(len(cfg.layers)):
        Tq, Tk = cfg.t(li)
        qkv, q2, kv2 = saved[(li, "qkv")], saved[(li, "q2")], saved[(li, "kv2")]
        one = np.ones((cfg.P, 4, Tq, Tq))
        assert B.xattn_fwd_ref(qkv[:, :128], qkv[:, 128:256], qkv[:, 256:], cfg.P, Tq, Tq, one)[1] <= B.LOGIT_RANGE
        assert B.xattn_fwd_ref(q2, kv2[:, :128], kv2[:, 128:], cfg.P, Tq, Tk, np.ones((cfg.P, 4, Tq, Tk)))[1] <= B.LOGIT_RANGE
    # one layer's backward: the float32 run inside the layer rule and the per-element bounds
    li = len(cfg.layers) - 1
    args = B.layer_args(cfg, sd, inp, saved, li, p, SEED)
    bounds = B.dec_bwd_bounds(*args)
    dx, dmem, grads, _ = B.dec_bwd_ref(*args, F32)
    got = dict(grads, dx=dx, dmem=dmem)
    got.update({k: grads[k[:-3]] for k in bounds if k.endswith("/el")})
    worst = {k: B.ratio(got[k], *bounds[k]) for k in bounds}
    k = max(worst, key=worst.get)
    assert report("dec_bwd", f"{cfg} p={p:.1f} {k}", worst[k]) <= 1.0
    assert sum(k.endswith("/el") for k in bounds) == 3


# ---- mutants: every one leaves its bound on at least one listed case ---------------------------------------------------------------
def leaves(got, ref, tol):
    return not B.ratio(got, ref, tol) <= 1.0


def test_product_mutants_leave_the_bound():
    c3 = lin_case(17, 64, 3, False)
    assert leaves(B.lin_fwd_ref(c3, mut="last_k_tile"), *B.lin_fwd_ref(c3))  # K = 3: the one k tile
    c272 = lin_case(272, 384, 128, False)
    assert leaves(B.lin_dw_ref(c272, "last_k_tile")["dW"], *B.lin_dw_ref(c272)["dW"])  # M = 272: the 16 rows of the last slice
    for M in (257, 272, 513):
        c = lin_case(M, 128, 512, False)
        assert leaves(B.lin_dw_ref(c, "slice_boundary")["dW"], *B.lin_dw_ref(c)["dW"]), M
        assert leaves(B.lin_dw_ref(c, "bias_on_split")["dW"], *B.lin_dw_ref(c)["dW"]), M
    for M in (1, 65):
        c = lin_case(M, 512, 128, False)
        assert leaves(B.lin_dx_ref(c, 1, mut="no_acc"), *B.lin_dx_ref(c, 1)), M
    cs = lin_case(16, 256, 128, True)
    assert leaves(B.lin_fwd_ref(cs, mut="no_slice"), *B.lin_fwd_ref(cs))


def test_attention_mutants_leave_the_bound():
    hit = {m: 0 for m in ("mask_transposed", "mask_saved", "scale_128", "head_stride")}
    for pairs, Tq, Tk, p in attn_cases():
        Q, K, V, dO = B.attn_case(pairs, Tq, Tk)
        f = B.attn_factor(SEED, 2, p, pairs, Tq, Tk)
        ref, _ = B.xattn_fwd_ref(Q, K, V, pairs, Tq, Tk, f)
        refb = B.xattn_bwd_ref(Q, K, V, ref["P"][0], dO, pairs, Tq, Tk, f)
        for m in hit:
            fm = B.attn_factor(SEED, 2, p, pairs, Tq, Tk, mut=m)
            Pm, Om, _ = B.xattn_fwd(Q, K, V, pairs, Tq, Tk, fm, mut=m)
            bm = B.xattn_bwd(Q, K, V, ref["P"][0], dO, pairs, Tq, Tk, fm, mut=m)
            out = leaves(Pm, *ref["P"]) or leaves(Om, *ref["O"])
            hit[m] += out and (m == "mask_saved" or any(leaves(a, *refb[k]) for a, k in zip(bm, ("dQ", "dK", "dV"))))
    # the scale and the head stride show on every case with more than one key resp. on every case; the mask ones where p > 0 and the
    # probability matrix has more than one element
    assert all(v > 0 for v in hit.values()), hit
    assert hit["head_stride"] == len(attn_cases()), hit


def test_batchnorm_mutants_leave_the_bound():
    Y, g, b, rm, rv = B.bn_case(256, 128, "offset")
    ref = B.bn_fwd_ref(Y, g, b, rm, rv)
    assert leaves(B.bn_fwd(Y, g, b, rm, rv, mut="onepass")["xhat"], *ref["xhat"]) and leaves(B.bn_fwd(Y, g, b, rm, rv, mut="onepass")["rstd"], *ref["rstd"])
    for M in B.BN_ROWS:
        Y, g, b, rm, rv = B.bn_case(M, 64)
        assert leaves(B.bn_fwd(Y, g, b, rm, rv, mut="biased_rv")["rv"], *B.bn_fwd_ref(Y, g, b, rm, rv)["rv"]), M
        args = B.bn_bwd_case(M, 64)
        ref = B.bn_bwd_ref(*args)
        assert leaves(B.bn_bwd(*args, mut="mask_dout")["dy"], *ref["dy"]) and leaves(B.bn_bwd(*args, mut="dg_overwrite")["dg"], *ref["dg"]), M


def test_index_mutants_leave_the_bound():
    table, idx = B.gauss((1, 2), 23, 128), B.index_case(64, 23)
    assert not np.array_equal(B.gather_ref(table, idx, mut="row_eq_rows"), B.gather_ref(table, idx))
    dY, g0 = B.gauss((3, 64), 64, 128), B.gauss((4, 64), 23, 128)
    ref, tol = B.scatter_ref(dY, idx, g0)
    assert leaves(B.scatter_ref(dY, idx, g0, mut="pad_grad")[0], ref, tol)
    assert leaves(B.scatter_ref(dY, idx, g0, mut="row_eq_rows")[0], ref, tol)


@pytest.mark.parametrize("mut,field", [("E_order", (-1, "E")), ("site_45", None), ("kv_slice", None)])
def test_chain_mutants_leave_the_bound(mut, field):
    cfg, sd, inp, refs = chain(1, B.P_DROP)
    saved = {k: v[0] for k, v in refs.items()}
    got = B.forward_chain(cfg, sd, inp, SEED, B.P_DROP, saved=saved, mut=mut)
    out = {k for k in refs if leaves(got[k][0], *refs[k])}
    if mut == "E_order":
        assert out == {(-1, "E")}
    elif mut == "site_45":
        assert out == {(li, f) for li in range(len(cfg.layers)) for f in ("h1d", "out", "xh3", "r3")}
    else:
        assert out == {(li, "kv2") for li in range(len(cfg.layers))}
