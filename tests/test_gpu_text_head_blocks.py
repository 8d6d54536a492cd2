"""GPU half of the text-head block tier: th_gemm_kernel in its four epilogues (split and single f16), fast_gemm with its
bf16 splits, k-split and slab reduction, th_split / th_split_bf16, th_attn_kernel<1024>, th_ln_kernel<false> / <true>, ONE launch at a
time through the dev library libt2l_blocks.so (csrc/text_head_blocks.hip), every output element held against the float64
references and derived bounds of tests/text_head_blocks.py — and, in the exact cases, against float32 references bit for bit.

The test packs every operand plane and unpacks every tiled output with its own numpy T16 / T32 functions. Inputs sit between NaN
halos; outputs are carved from 0xA5-patterned buffers (tests/guards.py) whose halos must keep their pattern. A CU-count override
(8, 32) makes a few hundred rows reach the ring's cross-tile prefetch and the job list's `break`. Each test prints its worst
err / tol as a `BLOCK ...` line (pytest -s); the MI355X figures are in profiles/text_head_blocks.md."""
import ctypes

import numpy as np
import pytest

from oracle import arith
from tests import guards
from tests import text_head_blocks as T
from tests import train_blocks as TB

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF16_NAN = 0x7FC0
PATTERN16 = 0xA5A5


@pytest.fixture(scope="module")
def lib():
    import torch

    from text2loc_amd import engine

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = T.declare(engine.load_library(T.blocks_path()))
    yield lib
    lib.t2l_blk_th_set_cus(0)


@pytest.fixture(scope="module")
def eng(lib):
    from text2loc_amd.engine import Engine

    e = Engine(0, lib=lib)
    yield e
    e.close()


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def dev(a):
    """a guarded device copy of an input: NaN halos for floats, a bf16 NaN pattern for 16-bit integer planes"""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    t = torch.from_numpy(a).cuda()
    return guards.guarded(t, NAN if t.dtype.is_floating_point else BF16_NAN)


def fresh(n, dtype):
    """an output of n elements: payload and halos hold the 0xA5 pattern"""
    buf, lo, nbytes, view = guards._carve((n,), dtype, "cuda")
    buf.fill_(guards.PATTERN_BYTE)
    view._guard = guards.Guard(buf, lo, nbytes, view, "empty")
    return view


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host(t):
    return t.detach().cpu().numpy()


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


def flag_tensor():
    import torch

    return torch.zeros(1, dtype=torch.int32, device="cuda")


def ratio(got, ref, tol):
    err = np.abs(got.astype(np.float64) - ref)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0  # (NaN propagates: a NaN fails every comparison)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


class Worst:
    def __init__(self, name):
        self.name, self.worst, self.at, self.exact = name, 0.0, "", 0

    def hold(self, r, what):
        assert r <= 1.0, f"{self.name} {what}: err / tol = {r:.4g}"
        if r >= self.worst:
            self.worst, self.at = r, what

    def same_bits(self, got, want, what):
        bad = bits(got) != bits(want)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{self.name} {what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {at}: "
                                 f"got {float(got[at])!r}, want {float(want[at])!r}; rows {sorted(set(np.argwhere(bad)[:, 0].tolist()))[:8]}, "
                                 f"columns {sorted(set(np.argwhere(bad)[:, -1].tolist()))[:8]}")
        self.exact += 1

    def report(self):
        print(f"\nBLOCK {self.name} worst={self.worst:.4f} at [{self.at}] bit-equal cases={self.exact}")


# ---- th_gemm ------------------------------------------------------------------------------------------------------------------
def launch_gemm(lib, c, nan_padding=False):
    """-> (out0, out1, flag value) as numpy arrays in the kernel's layout"""
    import torch

    ok(lib, lib.t2l_blk_th_set_cus(c.cus or 0))
    padx = lambda p: T.t16_pack(T.pad_rows(p, c.m_pad, np.float16(NAN) if nan_padding else 0))
    xh, xl, wh, wl = dev(padx(c.xh)), dev(padx(c.xl)), dev(T.t16_pack(c.wh)), dev(T.t16_pack(c.wl))
    bias, flag = dev(c.bias), flag_tensor()
    rh = rl = out1 = None
    if c.epi == T.EPI_RESID:
        rh, rl = dev(T.t16_pack(T.pad_rows(c.rh, c.m_pad))), dev(T.t16_pack(T.pad_rows(c.rl, c.m_pad)))
    if c.epi in (T.EPI_T32, T.EPI_RESID):
        out0 = fresh(c.m_pad * c.N, torch.float32)
    elif c.epi == T.EPI_RELU16:
        out0, out1 = fresh(c.m_pad * c.N, torch.float16), fresh(c.m_pad * c.N, torch.float16)
    else:
        out0 = dev(c.C0.reshape(-1)) if c.acc else fresh(c.M * c.n_real, torch.float32)
    ok(lib, lib.t2l_blk_th_gemm(c.epi, c.single, ptr(wh), ptr(wl), ptr(xh), ptr(xl), ptr(bias), ptr(rh), ptr(rl), ptr(out0), ptr(out1), ptr(flag),
                               c.m_tiles, c.n_tiles, c.K, c.N, c.M, c.n_real, c.relu, c.acc))
    ins = [t for t in (xh, xl, wh, wl, bias, rh, rl) if t is not None]
    guards.check_halos(*ins, out0, *([out1] if out1 is not None else []))  # nothing beyond m_pad rows / M x n_real is written
    if out0._guard.kind == "empty":
        assert out0._guard.unwritten_words() == 0, f"{c.name}: out0 has unwritten words"
    if out1 is not None:
        left = out1._guard.unwritten_words()
        assert left == (c.m_pad * c.N // 2 if c.single else 0), f"{c.name}: out1: {left} pattern words (SINGLE leaves it untouched)"
    return host(out0), (host(out1) if out1 is not None else None), int(flag.item())


def real_rows(c, out0, out1):
    """the real rows (and columns) of the kernel's output as arrays [M, .]"""
    if c.epi in (T.EPI_T32, T.EPI_RESID):
        return T.t32_unpack(out0, c.m_pad, c.N)[:c.M], None
    if c.epi == T.EPI_RELU16:
        return T.t16_unpack(out0, c.m_pad, c.N)[:c.M], T.t16_unpack(out1, c.m_pad, c.N)[:c.M]
    return out0.reshape(c.M, c.n_real), None


@pytest.mark.parametrize("single", (0, 1))
@pytest.mark.parametrize("epi", range(4))
def test_th_gemm(lib, epi, single):
    w = Worst(f"th_gemm {T.EPI_NAMES[epi]} {'single' if single else 'split'}")
    cus = lib.t2l_blk_th_cus()
    for c in T.gemm_cases(epi, single, "exact"):
        a, b = real_rows(c, *launch_gemm(lib, c)[:2])
        want = T.gemm_exact32(c)
        if epi == T.EPI_RELU16:
            hi, lo = T.split_f16(want)
            w.same_bits(a, hi, c.name + " hi")
            if not single:
                w.same_bits(b, lo, c.name + " lo")
        else:
            w.same_bits(a, want, c.name)
    for c in T.gemm_cases(epi, single, "gauss"):
        out0, out1, flag = launch_gemm(lib, c)
        a, b = real_rows(c, out0, out1)
        ref, tol = T.gemm_model(c)
        if epi == T.EPI_RELU16:
            got = a.astype(np.float64) + (0.0 if single else b.astype(np.float64))
            tol = tol + T.plane_store_tol(ref, tol, single)
            assert flag == 0, c.name
        else:
            got = a
        jobs = T.jobs_per_workgroup(c.cus or cus, c.m_tiles, c.n_tiles)
        w.hold(ratio(got, ref, tol), f"{c.name} jobs/wg max {max(jobs)} min {min(jobs)}")
        if c.M < c.m_pad:  # padding rows of X: zeros or NaNs, the real rows do not change a bit (and raise no flag)
            o0, o1, flag2 = launch_gemm(lib, c, nan_padding=True)
            a2, b2 = real_rows(c, o0, o1)
            assert np.array_equal(bits(a), bits(a2)) and flag2 == 0, c.name + ": NaN padding rows reach real rows or the flag"
            if b is not None and not single:
                assert np.array_equal(bits(b), bits(b2)), c.name
    w.report()


@pytest.mark.parametrize("single", (0, 1))
def test_th_gemm_relu_epilogue_flags_real_rows_only(lib, single):
    """a value >= 3e4 in a real row raises the flag; the same value in a padding row (m >= M) does not"""
    c = T.GemmCase(T.EPI_RELU16, single, 64, 1, 100, 8, "exact")  # M = 100 of m_pad = 256 rows
    c.bias = np.zeros_like(c.bias)
    w = np.zeros((c.N, c.K), np.float32)
    w[3, 0] = 200.0
    c.wh, c.wl = T.split_f16(w)
    for row, want in ((5, 1), (150, 0)):
        x = np.zeros((c.m_pad, c.K), np.float32)  # (all m_pad rows are given: launch_gemm's padding is then the identity)
        x[row, 0] = 200.0
        c.xh, c.xl = T.split_f16(x)
        out0, _, flag = launch_gemm(lib, c)
        hi = T.t16_unpack(out0, c.m_pad, c.N)
        assert float(hi[row, 3]) == 40000.0 and flag == want, (row, flag)


# ---- fast_gemm ----------------------------------------------------------------------------------------------------------------
def launch_fast(lib, eng, c):
    import torch

    ok(lib, lib.t2l_blk_th_set_cus(c.cus or 0))
    A, B = dev(c.A.reshape(-1)), dev(c.B.reshape(-1))
    bias = dev(c.bias) if c.has_bias else None
    out = dev(c.C0.reshape(-1)) if c.acc else fresh(c.Mo * c.No, torch.float32)
    cs = dev(c.cs0) if c.cs0 is not None else None
    ks = ctypes.c_int(0)
    ok(lib, lib.t2l_blk_fast_gemm(eng._h, ptr(A), c.a_trans, ptr(B), c.b_trans, ptr(bias), ptr(out), c.Mo, c.No, c.Kc, c.relu, c.acc, c.single,
                                 ptr(cs), ctypes.byref(ks)))
    guards.check_halos(*[t for t in (A, B, bias, out, cs) if t is not None])
    if out._guard.kind == "empty":
        assert out._guard.unwritten_words() == 0, c.name
    return host(out).reshape(c.Mo, c.No), (host(cs) if cs is not None else None), ks.value


@pytest.mark.parametrize("single", (0, 1))
@pytest.mark.parametrize("mode", T.FAST_MODES)
def test_fast_gemm(lib, eng, mode, single):
    w, wc = Worst(f"fast_gemm {mode} {'single' if single else 'split'}"), Worst(f"fast_gemm {mode} colsum")
    seen = set()
    for c in T.fast_cases("exact"):
        if c.mode == mode and c.single == single:
            out, _, ks = launch_fast(lib, eng, c)
            assert ks == c.ks, c.name
            w.same_bits(out, T.fast_exact32(c), c.name)
    for c in T.fast_cases("gauss"):
        if c.mode == mode and c.single == single:
            out, cs, ks = launch_fast(lib, eng, c)
            assert ks == c.ks, c.name
            seen.add(ks)
            w.hold(ratio(out, *T.fast_model(c)), c.name)
            if cs is not None:
                wc.hold(ratio(cs, *T.fast_colsum(c)), c.name)
    assert seen == {1, 2, 4, 8}, seen
    w.report()
    if mode == "dW":
        wc.report()


@pytest.mark.parametrize("single", (0, 1))
def test_fast_gemm_ignores_what_its_workspace_held(lib, single):
    """a larger call on huge finite values fills the context's planes and slabs; the small calls behind it (k_pad > Kc; a k-split of
    8) equal those of a fresh context bit for bit"""
    from text2loc_amd.engine import Engine

    big = T.FastCase("plain", single, 600, 512, 1152, None, "gauss")
    big.A, big.B = np.full_like(big.A, 1.0e15), np.full_like(big.B, -1.0e15)
    small = [T.FastCase("plain_acc", single, 65, 256, 32, None, "gauss"), T.FastCase("dX0", single, 64, 256, 1024, 8, "gauss")]
    outs = []
    for dirty in (True, False):
        e = Engine(0, lib=lib)
        try:
            if dirty:
                launch_fast(lib, e, big)
            outs.append([launch_fast(lib, e, c)[0] for c in small])
        finally:
            e.close()
    for c, a, b in zip(small, *outs):
        assert np.array_equal(bits(a), bits(b)), c.name


# ---- the splits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (256, 1024))
def test_th_split(lib, C):
    import torch

    n = 0
    for M in (1, 31, 32, 33, 257):
        m_pad = T.ceil_to(M, 256)
        x = T.gauss32((T.SEED, 8, M, C), M, C) * np.float32(4.0)
        x[0, :8] = [1e-3, -1e-5, 6e-8, 2.0 ** -14, 29999.0, -29999.0, 0.0, 1.0]  # (subnormal halves; the largest safe values)
        for poison, want_flag in ((None, 0), (3.0e4, 1), (-3.0e4, 1), (np.inf, 1), (np.nan, 1)):
            xx = x.copy()
            if poison is not None:
                xx[M - 1, C - 3] = poison
            X, hi, lo, flag = dev(xx.reshape(-1)), fresh(m_pad * C, torch.float16), fresh(m_pad * C, torch.float16), flag_tensor()
            ok(lib, lib.t2l_blk_th_split(ptr(X), M, C, m_pad, ptr(hi), ptr(lo), ptr(flag)))
            guards.check_halos(X, hi, lo)
            assert int(flag.item()) == want_flag, (M, poison)
            eh, el = T.split_f16(T.pad_rows(xx, m_pad))
            gh, gl = T.t16_unpack(host(hi), m_pad, C), T.t16_unpack(host(lo), m_pad, C)
            if poison is not None:  # (the flagged element itself: inf / NaN payloads are not compared)
                for a in (eh, el, gh, gl):
                    a[M - 1, C - 3] = 0
            assert np.array_equal(bits(gh), bits(eh)) and np.array_equal(bits(gl), bits(el)), (M, C, poison)
            assert not gh[M:].view(np.uint16).any() and not gl[M:].view(np.uint16).any()  # padding rows: zeros over the poison
            n += 1
    print(f"\nBLOCK th_split C={C} bit-equal cases={n}")


def _bf16_planes(a64, rows_pad, k_pad):
    hi, lo = arith.split_bf16(a64)
    full = lambda p: T.pad_rows(np.pad(T.bf16_bits(p), ((0, 0), (0, k_pad - p.shape[1]))), rows_pad)
    return full(hi), full(lo)


def _run_split_bf16(lib, trans, a, colsum0):
    import torch

    R, C = a.shape
    rows, kc = (C, R) if trans else (R, C)
    rows_pad, k_pad = T.ceil_to(rows, 256), T.ceil_to(kc, 64)
    A, hi, lo = dev(a.reshape(-1)), fresh(rows_pad * k_pad, torch.int16), fresh(rows_pad * k_pad, torch.int16)
    cs = dev(colsum0) if colsum0 is not None else None
    rp, kp = ctypes.c_int(0), ctypes.c_int(0)
    ok(lib, lib.t2l_blk_th_split_bf16(trans, ptr(A), R, C, ptr(hi), ptr(lo), rows_pad * k_pad, ptr(cs), ctypes.byref(rp), ctypes.byref(kp)))
    assert (rp.value, kp.value) == (rows_pad, k_pad)
    guards.check_halos(A, hi, lo, *([cs] if cs is not None else []))
    assert hi._guard.unwritten_words() == 0 and lo._guard.unwritten_words() == 0  # rows and k beyond the matrix: zeros over the poison
    eh, el = _bf16_planes((a.T if trans else a).astype(np.float64), rows_pad, k_pad)
    gh, gl = T.t16_unpack(host(hi).view(np.uint16), rows_pad, k_pad), T.t16_unpack(host(lo).view(np.uint16), rows_pad, k_pad)
    assert np.array_equal(gh, eh) and np.array_equal(gl, el), (trans, R, C)
    return host(cs) if cs is not None else None


def test_th_split_bf16(lib):
    n = 0
    for R, C in ((1, 32), (31, 96), (32, 160), (33, 256), (257, 96), (257, 1152)):
        _run_split_bf16(lib, 0, T.gauss32((T.SEED, 9, R, C), R, C), None)
        n += 1
    print(f"\nBLOCK th_split_bf16 bit-equal cases={n}")


def test_th_split_bf16_transposed_with_its_column_sum(lib):
    w, n = Worst("th_split_bf16<true> colsum"), 0
    Rs, Cs = (32, 63, 64, 65, 200), (4, 124, 128, 132, 260)
    for R, C in list(zip(Rs, Cs)) + [(200, 4), (32, 260), (65, 124), (63, 132)]:
        a = T.gauss32((T.SEED, 10, R, C), R, C)
        cs0 = T.gauss32((T.SEED, 10, C), C)
        got = _run_split_bf16(lib, 1, a, cs0)
        w.hold(ratio(got, *TB.colsum(a.astype(np.float64), cs0.astype(np.float64))), f"R={R} C={C}")
        _run_split_bf16(lib, 1, a, None)
        n += 2
    w.report()
    print(f"BLOCK th_split_bf16<true> bit-equal cases={n}")


# ---- attention ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", T.ATTN_L)
def test_th_attn(lib, L):
    import torch

    w = Worst(f"th_attn L={L}")
    n_sent = T.attn_sentences(L)
    M = n_sent * L
    m_pad = T.ceil_to(M, 256)
    qkv = T.gauss32((T.SEED, 3, L), M, 3 * T.DM)
    Q = dev(T.t32_pack(T.pad_rows(qkv, m_pad, np.float32(NAN))))  # padding rows hold NaN
    ohi, olo, flag = fresh(m_pad * T.DM, torch.float16), fresh(m_pad * T.DM, torch.float16), flag_tensor()
    ok(lib, lib.t2l_blk_th_attn(ptr(Q), n_sent, L, ptr(ohi), ptr(olo), ptr(flag)))
    guards.check_halos(Q, ohi, olo)
    hi, lo = T.t16_unpack(host(ohi), m_pad, T.DM), T.t16_unpack(host(olo), m_pad, T.DM)
    ref, tol, zmin = T.attn_reference(qkv.astype(np.float64), n_sent, L)
    assert zmin >= -T.FB.LOGIT_RANGE and int(flag.item()) == 0
    got = T.join64(hi[:M], lo[:M])
    assert np.isfinite(got).all()
    w.hold(ratio(got, ref, tol + T.plane_store_tol(ref, tol)), f"n_sent={n_sent}")
    assert (bits(hi[M:]) == PATTERN16).all() and (bits(lo[M:]) == PATTERN16).all(), "rows >= M of the o planes were written"
    w.report()


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
def _ln_launch(lib, pool, y, gamma, beta, M, L, m_pad, pooled=None, pooled_off=0):
    import torch

    Y, G, B, flag = dev(T.t32_pack(T.pad_rows(y, m_pad, np.float32(NAN)))), dev(gamma), dev(beta), flag_tensor()
    if pool:
        ok(lib, lib.t2l_blk_th_ln(1, ptr(Y), ptr(G), ptr(B), M, L, m_pad, None, None, ctypes.c_void_p(pooled.data_ptr() + 4 * pooled_off), ptr(flag)))
        guards.check_halos(Y, G, B, pooled)
        return None, None, int(flag.item())
    hi, lo = fresh(m_pad * T.DM, torch.float16), fresh(m_pad * T.DM, torch.float16)
    ok(lib, lib.t2l_blk_th_ln(0, ptr(Y), ptr(G), ptr(B), M, L, m_pad, ptr(hi), ptr(lo), None, ptr(flag)))
    guards.check_halos(Y, G, B, hi, lo)
    return T.t16_unpack(host(hi), m_pad, T.DM), T.t16_unpack(host(lo), m_pad, T.DM), int(flag.item())


def test_th_ln(lib):
    w = Worst("th_ln<false>")
    for M in T.LN_ROWS:
        y = T.ln_input(M, 0)
        gamma = (1.0 + 0.1 * T.gauss32((T.SEED, 12, 0), T.DM)).astype(np.float32)
        beta = (0.1 * T.gauss32((T.SEED, 12, 1), T.DM)).astype(np.float32)
        hi, lo, flag = _ln_launch(lib, 0, y, gamma, beta, M, 1, T.ceil_to(M, 256))
        ref, tol = T.ln_reference(y, gamma, beta)
        assert flag == 0, "NaN padding rows of y raised the flag (the m < M guard)"
        w.hold(ratio(T.join64(hi[:M], lo[:M]), ref, tol + T.plane_store_tol(ref, tol)), f"M={M}")
    w.report()


@pytest.mark.parametrize("L", T.POOL_L)
def test_th_ln_pool(lib, L):
    w = Worst(f"th_ln<true> L={L}")
    n_sent, s0 = 96 // L + 2, 3
    M = n_sent * L
    m_pad = T.ceil_to(M, 256)
    y = T.ln_input(M, L)
    gamma, beta = T.pool_params(L)
    pooled = dev(np.full((s0 + n_sent) * T.DM, -np.inf, np.float32))
    _ln_launch(lib, 1, y, gamma, beta, M, L, m_pad, pooled, s0 * T.DM)
    got = host(pooled).reshape(s0 + n_sent, T.DM)
    assert np.isneginf(got[:s0]).all(), "sentences in front of the offset were written"
    got = got[s0:].astype(np.float64)
    rows, tol = T.ln_reference(y, gamma, beta)
    ref = T.pool_reference(rows, n_sent, L)
    assert (ref < 0).any() and (got < 0).any()
    w.hold(ratio(got, ref, tol), f"n_sent={n_sent} offset={s0}")
    # the argument set: the pooled value is (within the rows' bound) one of the sentence's rows that can be the maximum
    r3 = rows.reshape(n_sent, L, T.DM)
    cand = (np.abs(r3 - got[:, None, :]) <= tol) & (r3 >= ref[:, None, :] - 2 * tol)
    assert cand.any(axis=1).all()
    # ... and the EXACT max of the kernel's own normalised rows, which th_ln<false> stores as planes: one split apart, + two float32
    # ulps (the two instances may contract gamma * x + beta differently)
    hi, lo, _ = _ln_launch(lib, 0, y, gamma, beta, M, L, m_pad)
    own = T.join64(hi[:M], lo[:M]).reshape(n_sent, L, T.DM).max(axis=1)
    assert (np.abs(got - own) <= 2.0 ** -22 * np.abs(own) + 2.0 ** -25 + 2 * 2.0 ** -23 * np.abs(own)).all()
    w.report()


# ---- the door: one t2l_text_head call, every saved field against its stage ----------------------------------------------------
def _saved(lib, eng, field, dtype):
    import torch

    n = ctypes.c_int64(0)
    assert lib.t2l_blk_th_saved(eng._h, field.encode(), None, 0, ctypes.byref(n)) == 0, lib.t2l_blk_last_error().decode()
    buf = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    ok(lib, lib.t2l_blk_th_saved(eng._h, field.encode(), ctypes.c_void_p(buf.data_ptr()), n.value, ctypes.byref(n)))
    return host(buf).view(dtype)


@pytest.mark.parametrize("single", (0, 1))
def test_text_head_stage_by_stage(lib, eng, single):
    import torch

    from text2loc_amd import synth
    from text2loc_amd.engine import Engine

    w = Worst(f"text_head stages {'single' if single else 'split'}")
    n_sent, L = 40, 13
    M, m_pad, sp_cap = n_sent * L, T.ceil_to(n_sent * L, 256), T.ceil_to(n_sent, 256)
    sd = synth.make_language_head_weights(3)
    hidden = synth.make_t5_hidden(n_sent, L, seed=4013)
    ok(lib, lib.t2l_blk_th_set_cus(0))
    eng.text_head_load_weights(sd)
    eng.set_option("text_head_rows", 0)
    eng.set_option("encoder_f16", single)
    try:
        out, bad = eng.text_head(torch.from_numpy(hidden).cuda())
    finally:
        eng.set_option("encoder_f16", 0)
    assert not bad
    p = "language_encoder.intra_module.0."
    f16 = lambda f, cols: T.t16_unpack(_saved(lib, eng, f, np.float16), m_pad, cols)
    f32 = lambda f, cols: T.t32_unpack(_saved(lib, eng, f, np.float32), m_pad, cols)
    # th_split: the x planes are the split of the hidden states, padding rows zero
    x = hidden.reshape(M, T.DM)
    xh, xl = f16("xh", T.DM), f16("xl", T.DM)
    eh, el = T.split_f16(T.pad_rows(x, m_pad))
    w.same_bits(xh, eh, "x hi")
    w.same_bits(xl, el, "x lo")
    # q | k | v
    qkv = f32("qkv", 3 * T.DM)[:M]
    w.hold(ratio(qkv, *T.planes_linear(xh[:M], xl[:M], sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"], single)), "qkv")
    # attention over the kernel's own qkv
    oh, ol = f16("oh", T.DM)[:M], f16("ol", T.DM)[:M]
    ref, tol, zmin = T.attn_reference(qkv.astype(np.float64), n_sent, L)
    assert zmin >= -T.FB.LOGIT_RANGE
    w.hold(ratio(T.join64(oh, ol), ref, tol + T.plane_store_tol(ref, tol)), "o")
    # x1 = LayerNorm1(x + o W_out^T + b_out): y1 is overwritten by y2, so the product's bound is carried through the LayerNorm's
    y1, ey1 = T.planes_linear(oh, ol, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], single, res=T.join64(xh[:M], xl[:M]))
    ref, tol = T.ln_propagated(y1, ey1, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    x1h, x1l = f16("x1h", T.DM)[:M], f16("x1l", T.DM)[:M]
    w.hold(ratio(T.join64(x1h, x1l), ref, tol + T.plane_store_tol(ref, tol)), "x1")
    # h = relu(x1 W_1^T + b_1)
    hh, hl = f16("hh", T.FF)[:M], f16("hl", T.FF)[:M]
    ref, tol = T.planes_linear(x1h, x1l, sd[p + "linear1.weight"], sd[p + "linear1.bias"], single, relu=True)
    w.hold(ratio(hh.astype(np.float64) + (0.0 if single else hl.astype(np.float64)), ref, tol + T.plane_store_tol(ref, tol, single)), "h")
    # y2 = x1 + h W_2^T + b_2: the residual is x1 (both planes, also under SINGLE), not x
    y2 = f32("y", T.DM)[:M]
    w.hold(ratio(y2, *T.planes_linear(hh, hl, sd[p + "linear2.weight"], sd[p + "linear2.bias"], single, res=T.join64(x1h, x1l))), "y2")
    # pooled = max over the tokens of LayerNorm2(y2)
    pooled = _saved(lib, eng, "pooled", np.float32).reshape(n_sent, T.DM)
    rows, tol = T.ln_reference(y2, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    w.hold(ratio(pooled, T.pool_reference(rows, n_sent, L), tol), "pooled")
    # its planes, and inter_mlp (Linear + BatchNorm folded by the loader) on them: pooled feeds inter_mlp
    ph = T.t16_unpack(_saved(lib, eng, "ph", np.float16), sp_cap, T.DM)
    pl = T.t16_unpack(_saved(lib, eng, "pl", np.float16), sp_cap, T.DM)
    eh, el = T.split_f16(T.pad_rows(pooled, sp_cap))
    w.same_bits(ph, eh, "pooled hi")
    w.same_bits(pl, el, "pooled lo")
    m = "language_encoder.inter_mlp.0."
    Wf, bf = T.fold_bn(sd[m + "0.weight"], sd[m + "0.bias"], sd[m + "1.weight"], sd[m + "1.bias"], sd[m + "1.running_mean"], sd[m + "1.running_var"])
    ref, tol = T.planes_linear(ph[:n_sent], pl[:n_sent], Wf, bf, single, w_known=False)
    w.hold(ratio(host(out), ref, tol + 4 * T.U * np.abs(bf)), "out")
    # the final output equals the shipped library's bits
    plain = Engine(0)
    try:
        plain.text_head_load_weights(sd)
        plain.set_option("encoder_f16", single)
        out2, bad2 = plain.text_head(torch.from_numpy(hidden).cuda())
    finally:
        plain.close()
    assert not bad2 and torch.equal(out, out2)
    w.report()


# ---- refusals: a shape below the ring's minimum is never launched -----------------------------------------------------------------
def test_wrappers_refuse_what_the_kernels_do_not_take(lib, eng):
    one = ctypes.c_void_p(256)  # (never dereferenced: every call below is refused before a launch)
    ks = ctypes.c_int(0)
    for K in (16, 32, 48, 80):
        assert lib.t2l_blk_th_gemm(0, 0, one, one, one, one, one, None, None, one, None, None, 1, 1, K, 256, 1, 256, 0, 0) == -1
        assert b"four k-steps" in lib.t2l_blk_last_error()
    assert lib.t2l_blk_th_gemm(3, 0, one, one, one, one, one, None, None, one, None, None, 1, 1, 64, 256, 1, 256, 0, 2) == -1
    assert lib.t2l_blk_th_gemm(1, 0, one, one, one, one, one, None, None, one, None, None, 1, 1, 64, 256, 1, 256, 0, 0) == -1
    assert lib.t2l_blk_th_gemm(3, 0, one, one, one, one, one, None, None, one, None, None, 1, 1, 64, 256, 1, 258, 0, 0) == -1
    assert lib.t2l_blk_th_set_cus(12) == -1 and lib.t2l_blk_th_set_cus(4) == -1
    assert lib.t2l_blk_fast_gemm(eng._h, one, 1, one, 1, None, one, 66, 256, 64, 0, 0, 0, None, ctypes.byref(ks)) == -1
    assert lib.t2l_blk_th_attn(one, 1, 33, one, one, one) == -1
    assert lib.t2l_blk_th_ln(1, one, one, one, 10, 3, 32, None, None, one, one) == -1
