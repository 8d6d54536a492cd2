"""GPU tier of the training-block tests: every product of gemm_f32.h as the step's launchers launch it, and the
attention / LayerNorm / F.normalize / dropout / pool + normalise / seq-max kernels (the row kernels at the fine step's width 128 too),
ONE launch at a time through the dev library libt2l_blocks.so
(csrc/train_blocks.hip), each held element by element against the float64 references and derived bounds of tests/train_blocks.py.

Inputs are Gaussian from fixed seeds and sit between NaN halos (a read past an end enters the arithmetic); every output is carved from a
buffer patterned with 0xA5 (tests/guards.py): the halos — rows >= M among them — must keep their pattern and every payload word must be
written. Outputs the kernels ADD to (dW, db, dgamma, dbeta, an accumulating dX) start from non-zero prior contents between NaN halos.
Each test prints its worst err / tol as a `BLOCK ...` line (pytest -s); the MI355X figures are in profiles/train_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import guards
from tests import train_blocks as TB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")  # (the device is initialised before the dev library's first launch)
    return TB.load_blocks()


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=np.float32):
    """a guarded device copy of an input (NaN halos; an in-range value around an index array)"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).cuda()
    return guards.guarded(t, guards.NAN if dtype == np.float32 else 0)


def fresh(*shape, dtype=None):
    """an output the kernel must write whole: payload and halos hold the 0xA5 pattern"""
    import torch

    buf, lo, nbytes, view = guards._carve(shape, dtype or torch.float32, "cuda")
    buf.fill_(guards.PATTERN_BYTE)
    view._guard = guards.Guard(buf, lo, nbytes, view, "empty")
    return view


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptrs(ts):
    return (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


def check_buffers(inputs, outputs, what):
    guards.check_halos(*inputs, *outputs)
    for i, t in enumerate(outputs):
        if t._guard.kind == "empty":
            left = t._guard.unwritten_words()
            assert left == 0, f"{what}: output {i} {tuple(t.shape)}: {left} words were never written"


def ratio(got, ref, tol):
    """worst err / tol; where the bound is zero (a masked or dropped element) the value must be exactly the reference's"""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0  # (NaN propagates: a NaN fails every comparison below)


class Worst:
    def __init__(self, name):
        self.name, self.worst, self.at = name, 0.0, ""

    def hold(self, r, what):
        assert r <= 1.0, f"{self.name} {what}: err / tol = {r:.4g}"
        if r >= self.worst:
            self.worst, self.at = r, what

    def report(self):
        print(f"\nBLOCK {self.name} worst={self.worst:.4f} at {self.at}")


# ---- products -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.WIDTHS)
def test_gemm_nt(lib, N, Kp, ar):
    w = Worst(f"gemm_nt N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        c = TB.product_case("nt", M, N, Kp)
        X, W, b = dev(c.X), dev(c.W), dev(c.b)
        for bias, relu, epi, p in TB.nt_variants():
            want = TB.nt_reference(c, ar, bias, relu, epi, p)
            for block in (0, 1):
                Y, Y2 = fresh(M, N), (fresh(M, N) if epi else None)
                ok(lib, lib.t2l_blk_gemm_nt(ptr(X), ptr(W), ptr(b) if bias else None, ptr(Y), ptr(Y2), M, N, Kp, int(relu), epi, ar, block,
                                            TB.SEED, 2, p))
                what = f"M={M} bias={bias} relu={relu} epi={epi} p={p:.1f} block={block}"
                check_buffers((X, W, b), (Y, Y2) if epi else (Y,), what)
                w.hold(ratio(Y, *want["Y"]), what + " Y")
                if epi:
                    w.hold(ratio(Y2, *want["Y2"]), what + " Y2")
    w.report()


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.WIDTHS)
def test_gemm_nn(lib, N, Kp, ar):
    w = Worst(f"gemm_nn N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        c = TB.product_case("nn", M, N, Kp)
        dY, W = dev(c.dY), dev(c.W)
        for accumulate in (0, 1):
            want = TB.nn_reference(c, ar, accumulate)
            for block in (0, 1):
                dX = dev(c.C0) if accumulate else fresh(M, Kp)
                ok(lib, lib.t2l_blk_gemm_nn(ptr(dY), ptr(W), ptr(dX), M, N, Kp, accumulate, ar, block))
                what = f"M={M} accumulate={accumulate} block={block}"
                check_buffers((dY, W), (dX,), what)
                w.hold(ratio(dX, *want["dX"]), what)
    w.report()


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.WIDTHS)
def test_gemm_tn(lib, N, Kp, ar):
    w = Worst(f"gemm_tn N={N} Kp={Kp} arith={ar}")
    wb = Worst(f"gemm_tn_db N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        c = TB.product_case("tn", M, N, Kp)
        dY, X = dev(c.dY), dev(c.X)
        want = TB.tn_reference(c, ar)
        for block in (0, 1):
            dW, db = dev(c.C0), dev(c.db0)  # non-zero prior contents
            ok(lib, lib.t2l_blk_gemm_tn(ptr(dY), ptr(X), ptr(dW), ptr(db), M, N, Kp, ar, block))
            what = f"M={M} block={block}"
            check_buffers((dY, X), (dW, db), what)
            w.hold(ratio(dW, *want["dW"]), what + " dW")
            wb.hold(ratio(db, *want["db"]), what + " db")
    w.report()
    wb.report()


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.WIDTHS)
def test_gemm_tn_nn(lib, N, Kp, ar):
    """dW (+ db) and dX from ONE launch, each checked"""
    w = Worst(f"gemm_tn_nn N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        t, n = TB.product_case("tn", M, N, Kp), TB.product_case("nn", M, N, Kp)
        assert np.array_equal(t.dY, n.dY)
        dY, X, W, mask_src = dev(t.dY), dev(t.X), dev(n.W), dev(n.mask_src)
        want_t = TB.tn_reference(t, ar)
        for mask, accumulate, p in TB.tn_nn_variants():
            want_n = TB.nn_reference(n, ar, accumulate, mask, p)
            for block in (0, 1):
                dW, db = dev(t.C0), dev(t.db0)
                dX = dev(n.C0) if accumulate else fresh(M, Kp)
                ok(lib, lib.t2l_blk_gemm_tn_nn(ptr(dY), ptr(X), ptr(dW), ptr(db), ptr(W), ptr(dX), M, N, Kp, accumulate,
                                               ptr(mask_src) if mask else None, ar, block, TB.SEED, 2, p))
                what = f"M={M} mask={mask} accumulate={accumulate} p={p:.1f} block={block}"
                check_buffers((dY, X, W, mask_src), (dW, db, dX), what)
                w.hold(ratio(dW, *want_t["dW"]), what + " dW")
                w.hold(ratio(db, *want_t["db"]), what + " db")
                w.hold(ratio(dX, *want_n["dX"]), what + " dX")
    w.report()


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.MULTI_WIDTHS)
def test_gemm_nt_multi(lib, N, Kp, ar):
    """1, 2 and 3 jobs with distinct buffers in one launch: a job must not see its neighbour's data"""
    w = Worst(f"gemm_nt_multi N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        cs = [TB.ProductCase("nt", M, N, Kp, job=q) for q in range(3)]
        X, W, b = [dev(c.X) for c in cs], [dev(c.W) for c in cs], [dev(c.b) for c in cs]
        want = [TB.nt_reference(c, ar, True, False, 0, 0.0)["Y"] for c in cs]
        for n in (1, 2, 3):
            Y = [fresh(M, N) for _ in range(3)]
            ok(lib, lib.t2l_blk_gemm_nt_multi(n, ptrs(X), ptrs(W), ptrs(b), ptrs(Y), M, N, Kp, ar))
            guards.check_halos(*X, *W, *b, *Y)
            for q in range(3):
                if q < n:
                    assert Y[q]._guard.unwritten_words() == 0
                    w.hold(ratio(Y[q], *want[q]), f"M={M} jobs={n} job {q}")
                else:  # a job that was not launched is not touched
                    assert Y[q]._guard.unwritten_words() == M * N
    w.report()


@pytest.mark.parametrize("ar", TB.ARITHS)
@pytest.mark.parametrize("N,Kp", TB.MULTI_WIDTHS)
def test_gemm_tn_nn_multi(lib, N, Kp, ar):
    w = Worst(f"gemm_tn_nn_multi N={N} Kp={Kp} arith={ar}")
    for M in TB.ROWS:
        ts = [TB.ProductCase("tn", M, N, Kp, job=q) for q in range(3)]
        ns = [TB.ProductCase("nn", M, N, Kp, job=q) for q in range(3)]
        dY, X, W = [dev(c.dY) for c in ts], [dev(c.X) for c in ts], [dev(c.W) for c in ns]
        want_t = [TB.tn_reference(c, ar) for c in ts]
        want_n = [TB.nn_reference(c, ar, 0) for c in ns]
        for n in (1, 2, 3):
            dW, db = [dev(c.C0) for c in ts], [dev(c.db0) for c in ts]
            dX = [fresh(M, Kp) for _ in range(3)]
            ok(lib, lib.t2l_blk_gemm_tn_nn_multi(n, ptrs(dY), ptrs(X), ptrs(dW), ptrs(db), ptrs(W), ptrs(dX), M, N, Kp, ar))
            guards.check_halos(*dY, *X, *W, *dW, *db, *dX)
            for q in range(3):
                what = f"M={M} jobs={n} job {q}"
                if q < n:
                    assert dX[q]._guard.unwritten_words() == 0
                    w.hold(ratio(dW[q], *want_t[q]["dW"]), what + " dW")
                    w.hold(ratio(db[q], *want_t[q]["db"]), what + " db")
                    w.hold(ratio(dX[q], *want_n[q]["dX"]), what + " dX")
                else:
                    assert dX[q]._guard.unwritten_words() == M * Kp
                    assert np.array_equal(dW[q].cpu().numpy().astype(np.float64), ts[q].C0), what + ": dW of a job that was not launched"
                    assert np.array_equal(db[q].cpu().numpy().astype(np.float64), ts[q].db0)
    w.report()


# ---- attention ----------------------------------------------------------------------------------------------------------------
def f32(a):
    """the float32 a saved activation is handed on as, as exact float64"""
    return a.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("HD,sizes", [(64, (28, 1, 2, 17, 32)), (256, (1, 9, 32))])
def test_attention(lib, HD, sizes):
    """forward (P as well as O) and backward; S = 28 at HD = 64 is the compile-time instance"""
    wf, wb = Worst(f"attn_fwd HD={HD}"), Worst(f"attn_bwd HD={HD}")
    for S in sizes:
        for B in (1, 3):
            qkv, dO = TB.gauss((TB.SEED, 30, HD, S, B), B * S, 12 * HD), TB.gauss((TB.SEED, 31, HD, S, B), B * S, 4 * HD)
            d_qkv, d_dO = dev(qkv), dev(dO)
            for p in (0.0, TB.P_DROP):
                what = f"S={S} B={B} p={p:.1f}"
                fac = TB.drop_factor(TB.SEED, 4, p, (B, 4, S, S))
                (P_ref, P_tol), (O_ref, O_tol) = TB.layer_tol(TB.attn_fwd, qkv, B, S, HD, fac)
                P, O = fresh(B * 4 * S * S), fresh(B * S, 4 * HD)
                ok(lib, lib.t2l_blk_attn_fwd(ptr(d_qkv), ptr(P), ptr(O), B, S, HD, TB.SEED, 4, p))
                check_buffers((d_qkv,), (P, O), what)
                wf.hold(ratio(P, P_ref, P_tol), what + " P")
                wf.hold(ratio(O, O_ref, O_tol), what + " O")
                P_in = f32(P_ref)
                ((g_ref, g_tol),) = TB.layer_tol(TB.attn_bwd, qkv, P_in, dO, B, S, HD, fac)
                d_P, dqkv = dev(P_in.reshape(-1)), fresh(B * S, 12 * HD)
                ok(lib, lib.t2l_blk_attn_bwd(ptr(d_qkv), ptr(d_P), ptr(d_dO), ptr(dqkv), B, S, HD, TB.SEED, 4, p))
                check_buffers((d_qkv, d_P, d_dO), (dqkv,), what)
                wb.hold(ratio(dqkv, g_ref, g_tol), what + " dqkv")
    wf.report()
    wb.report()


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,waves", [(256, (16, 4)), (1024, (4,)), (128, (4,))])
def test_layernorm(lib, D, waves):
    """forward, and the backward with every LN_WAVES the step instantiates; T is not a multiple of the row stride"""
    wf, wb, wp = Worst(f"ln_fwd D={D}"), Worst(f"ln_bwd D={D}"), Worst(f"ln_bwd_dgamma_dbeta D={D}")
    for T in (1, 3, 4, 5, 140, 300):
        x, y, dout = (TB.gauss((TB.SEED, 40, D, T, k), T, D) for k in range(3))
        gamma, beta, dg0, db0 = (TB.gauss((TB.SEED, 41, D, T, k), D) for k in range(4))
        d_x, d_y, d_gamma, d_beta, d_dout = dev(x), dev(y), dev(gamma), dev(beta), dev(dout)
        for p in (0.0, TB.P_DROP):
            what = f"T={T} p={p:.1f}"
            fac = TB.drop_factor(TB.SEED, 5, p, (T, D))
            want = TB.layer_tol(TB.ln_fwd, x, y, gamma, beta, fac)
            out, xhat, rstd = fresh(T, D), fresh(T, D), fresh(T)
            ok(lib, lib.t2l_blk_ln_fwd(ptr(d_x), ptr(d_y), T, D, ptr(d_gamma), ptr(d_beta), ptr(out), ptr(xhat), ptr(rstd), TB.SEED, 5, p))
            check_buffers((d_x, d_y, d_gamma, d_beta), (out, xhat, rstd), what)
            for name, t, (ref, tol) in zip(("out", "xhat", "rstd"), (out, xhat, rstd), want):
                wf.hold(ratio(t, ref, tol), f"{what} {name}")
            xh, rs = f32(want[1][0]), f32(want[2][0])
            d_xh, d_rs = dev(xh), dev(rs)
            (res_ref, res_tol), (dy_ref, dy_tol) = TB.layer_tol(TB.ln_bwd, dout, xh, rs, gamma, fac)
            grads = TB.ln_param_grads(dout, xh, dg0, db0)
            for nw in waves:
                d_res, d_yg, dgamma, dbeta = fresh(T, D), fresh(T, D), dev(dg0), dev(db0)
                ok(lib, lib.t2l_blk_ln_bwd(ptr(d_dout), ptr(d_xh), ptr(d_rs), T, D, nw, ptr(d_gamma), ptr(d_res), ptr(d_yg), ptr(dgamma),
                                           ptr(dbeta), TB.SEED, 5, p))
                check_buffers((d_dout, d_xh, d_rs, d_gamma), (d_res, d_yg, dgamma, dbeta), f"{what} waves={nw}")
                wb.hold(ratio(d_res, res_ref, res_tol), f"{what} waves={nw} d_res")
                wb.hold(ratio(d_yg, dy_ref, dy_tol), f"{what} waves={nw} d_y")
                wp.hold(ratio(dgamma, *grads["dgamma"]), f"{what} waves={nw} dgamma")
                wp.hold(ratio(dbeta, *grads["dbeta"]), f"{what} waves={nw} dbeta")
    wf.report()
    wb.report()
    wp.report()


# ---- F.normalize of a row ------------------------------------------------------------------------------------------------------
def slot(t, D):
    """the middle D-wide slot of a [M, 3 D] tensor, as the pointer the wrapper takes"""
    return ctypes.c_void_p(t.data_ptr() + 4 * D)


def rownorm_case(lib, w, D, x, dy, wide, what):
    """forward and backward of one (x, dy) [M, D]; wide: the strided side is the middle slot of a 3 D-wide row between pre-filled
    neighbours (forward: they must come back bit-unchanged; backward: they are NaN, a read of them enters the result)"""
    M, ld = x.shape[0], (3 * D if wide else D)
    (y_ref, y_tol), (n_ref, n_tol) = TB.layer_tol(TB.rownorm_fwd, x)
    d_x, save_n = dev(x), fresh(M)
    if wide:
        side = TB.gauss((TB.SEED, 72, D, M), M, 3 * D)
        cat = dev(side)
        ok(lib, lib.t2l_blk_rownorm_fwd(ptr(d_x), M, D, slot(cat, D), ld, ptr(save_n)))
        check_buffers((d_x, cat), (save_n,), what)
        got = cat.cpu().numpy().astype(np.float64)
        assert np.array_equal(got[:, :D], side[:, :D]) and np.array_equal(got[:, 2 * D:], side[:, 2 * D:]), f"{what}: a neighbouring slot changed"
        y = cat[:, D:2 * D]
    else:
        y = fresh(M, D)
        ok(lib, lib.t2l_blk_rownorm_fwd(ptr(d_x), M, D, ptr(y), ld, ptr(save_n)))
        check_buffers((d_x,), (y, save_n), what)
    w[0].hold(ratio(y, y_ref, y_tol), what + " y")
    w[0].hold(ratio(save_n, n_ref, n_tol), what + " save_n")
    yy, n = f32(y_ref), f32(n_ref)
    ((dx_ref, dx_tol),) = TB.layer_tol(TB.rownorm_bwd, dy, yy, n)
    d_n, dx = dev(n), fresh(M, D)
    if wide:
        pad = np.full((M, D), np.nan)
        d_dy, d_yy = dev(np.concatenate([pad, dy, pad], axis=1)), dev(np.concatenate([pad, yy, pad], axis=1))
        ok(lib, lib.t2l_blk_rownorm_bwd(slot(d_dy, D), slot(d_yy, D), ld, ptr(d_n), M, D, ptr(dx)))
    else:
        d_dy, d_yy = dev(dy), dev(yy)
        ok(lib, lib.t2l_blk_rownorm_bwd(ptr(d_dy), ptr(d_yy), ld, ptr(d_n), M, D, ptr(dx)))
    check_buffers((d_dy, d_yy, d_n), (dx,), what)
    w[1].hold(ratio(dx, dx_ref, dx_tol), what + " dx")


@pytest.mark.parametrize("D", (128, 256))
def test_rownorm(lib, D):
    """the fine step's width and the coarse step's; a lone row, a ragged last workgroup (four rows each), more than one workgroup"""
    w = Worst(f"rownorm_fwd D={D}"), Worst(f"rownorm_bwd D={D}")
    for M in (1, 3, 4, 5, 33):
        x, dy = TB.gauss((TB.SEED, 70, D, M), M, D), TB.gauss((TB.SEED, 71, D, M), M, D)
        for wide in (False, True):
            rownorm_case(lib, w, D, x, dy, wide, f"M={M} ld={3 * D if wide else D}")
    w[0].report()
    w[1].report()


@pytest.mark.parametrize("D", (128, 256))
def test_rownorm_zero_rows(lib, D):
    """all-zero rows, in tensors of their own (dx = dy / 1e-12 there would widen every other row's bound): the forward clamps the norm
    at 1e-12 and returns zeros, the backward takes its n <= 1e-12 branch"""
    w = Worst(f"rownorm_zero_fwd D={D}"), Worst(f"rownorm_zero_bwd D={D}")
    rownorm_case(lib, w, D, np.zeros((2, D)), TB.gauss((TB.SEED, 73, D), 2, D), False, "zero rows")
    w[0].report()
    w[1].report()


# ---- element-wise dropout, ReLU + dropout backward -------------------------------------------------------------------------------
def test_dropout(lib):
    """one element, a workgroup less one / exactly / plus one, several workgroups; the mask source has negative and exactly-zero
    entries. A dropped or masked element is exactly the reference's zero (its bound is 0)."""
    wf, wb = Worst("drop_fwd"), Worst("relu_drop_bwd")
    for n in (1, 255, 256, 257, 1000):
        h, d = TB.gauss((TB.SEED, 80, n), n), TB.gauss((TB.SEED, 81, n), n)
        h[::7] = 0.0
        if n == 1:
            h[0] = 1.5  # (the lone element is live, so that both paths of it are seen over the two p)
        assert n == 1 or ((h < 0).any() and (h == 0).any() and (h > 0).any())
        d_h = dev(h)
        for p in (0.0, TB.P_DROP):
            what = f"n={n} p={p:.1f}"
            fac = TB.drop_factor(TB.SEED, 6, p, (n,))
            hd = fresh(n)
            ok(lib, lib.t2l_blk_drop_fwd(ptr(d_h), n, ptr(hd), TB.SEED, 6, p))
            check_buffers((d_h,), (hd,), what)
            wf.hold(ratio(hd, *TB.drop_reference(h, fac)), what)
            d_d = dev(d)  # in place: the gradient goes in, the masked gradient comes out
            ok(lib, lib.t2l_blk_relu_drop_bwd(ptr(d_d), ptr(d_h), n, TB.SEED, 6, p))
            check_buffers((d_h,), (d_d,), what)
            wb.hold(ratio(d_d, *TB.drop_reference(h, fac, d)), what)
    wf.report()
    wb.report()


# ---- pool + normalise, seq-max ------------------------------------------------------------------------------------------------
def int_equal(t, ref):
    return np.array_equal(t.cpu().numpy().reshape(ref.shape), ref)


def test_pool_norm(lib):
    import torch

    wf, wb = Worst("pool_norm_fwd"), Worst("pool_norm_bwd")
    for B in (1, 5):
        X, g = TB.gauss((TB.SEED, 50, B), B, 28, 256), TB.gauss((TB.SEED, 51, B), B, 256)
        arg_ref = TB.first_argmax(X)
        (out_ref, out_tol), (n_ref, n_tol) = TB.layer_tol(TB.pool_norm_fwd, X)
        d_X = dev(X)
        out, out2, arg, save_n = fresh(B, 256), fresh(B, 256), fresh(B, 256, dtype=torch.int32), fresh(B)
        ok(lib, lib.t2l_blk_pool_norm_fwd(ptr(d_X), ptr(out), ptr(arg), ptr(save_n), ptr(out2), B))
        check_buffers((d_X,), (out, out2, arg, save_n), f"B={B}")
        assert int_equal(arg, arg_ref), f"B={B}: pool_arg differs from the reference's"
        assert torch.equal(out, out2)
        wf.hold(ratio(out, out_ref, out_tol), f"B={B} out")
        wf.hold(ratio(save_n, n_ref, n_tol), f"B={B} save_n")
        y, n = f32(out_ref), f32(n_ref)
        ((dX_ref, dX_tol),) = TB.layer_tol(TB.pool_norm_bwd, g, y, arg_ref, n, 28)
        d_g, d_y, d_arg, d_n, dX = dev(g), dev(y), dev(arg_ref, np.int32), dev(n), fresh(B, 28, 256)
        ok(lib, lib.t2l_blk_pool_norm_bwd(ptr(d_g), ptr(d_y), ptr(d_arg), ptr(d_n), ptr(dX), B))
        check_buffers((d_g, d_y, d_arg, d_n), (dX,), f"B={B}")
        wb.hold(ratio(dX, dX_ref, dX_tol), f"B={B} dX")
    wf.report()
    wb.report()


@pytest.mark.parametrize("B,D,residual", [(3, 1024, False), (5, 256, True), (3, 128, False)])
def test_seq_max(lib, B, D, residual):
    """the text head's two calls: over the tokens of a sentence (D 1024), over the sentences of a description with the residual (D 256);
    the fine step's: over a pair's hints (D 128)"""
    import torch

    wf, wb = Worst(f"seq_max_fwd D={D}"), Worst(f"seq_max_bwd D={D}")
    for S in (1, 6, 32):
        X, g = TB.gauss((TB.SEED, 60, D, S), B, S, D), TB.gauss((TB.SEED, 61, D, S), B, D)
        R = TB.gauss((TB.SEED, 62, D, S), B, S, D) if residual else None
        V = TB.seq_values(X, R)
        arg_ref = TB.first_argmax(V)
        ((out_ref, out_tol),) = TB.layer_tol(TB.seq_max_fwd, V)
        d_X, d_R = dev(X), (dev(R) if residual else None)
        out, arg = fresh(B, D), fresh(B, D, dtype=torch.int32)
        ok(lib, lib.t2l_blk_seq_max_fwd(ptr(d_X), ptr(d_R), B, S, D, ptr(out), ptr(arg)))
        check_buffers((d_X, d_R) if residual else (d_X,), (out, arg), f"S={S}")
        assert int_equal(arg, arg_ref), f"S={S}: the seq-max argument differs from the reference's"
        wf.hold(ratio(out, out_ref, out_tol), f"S={S} out")
        ((dX_ref, dX_tol),) = TB.layer_tol(TB.seq_max_bwd, g, arg_ref, S)
        d_g, d_arg, dX = dev(g), dev(arg_ref, np.int32), fresh(B, S, D)
        ok(lib, lib.t2l_blk_seq_max_bwd(ptr(d_g), ptr(d_arg), B, S, D, ptr(dX)))
        check_buffers((d_g, d_arg), (dX,), f"S={S}")
        wb.hold(ratio(dX, dX_ref, dX_tol), f"S={S} dX")
    wf.report()
    wb.report()
