"""TEST INFRASTRUCTURE — float64 references, derived tolerances, case lists and the numpy restatement of the T16 / T32 layouts of the
text-head block tier (tests/test_text_head_blocks_cpu.py, tests/test_gpu_text_head_blocks.py; profiles/text_head_blocks.md).

``csrc/text_head.hip`` is held one launch at a time through the dev library's wrappers (csrc/text_head_blocks.hip). The TEST packs
every operand plane and unpacks every tiled output with the functions below, so the layouts are held from both sides. numpy,
``oracle.arith`` and the bound forms of ``tests/train_blocks.py`` / ``tests/fine_blocks.py`` only; nothing of the product is imported.

Layouts.  T16: 2-byte elements [rows / 32][cols / 8][32][8]; T32: float32 [rows / 32][cols / 4][32][4].

Products, two kinds of case.
  exact   W is a signed selection matrix (entries 0 / +-1, so its lo plane is all zeros; output column n picks input column pi(n),
          and pi makes every n tile pick from every 16-wide k-step of every k-part). Every term but one is exactly 0 and a product
          of two half-precision values is exact in float32, so whatever the summation order the accumulator is +-(hi + lo) of ONE
          input element and the epilogue's float32 additions follow in the kernel's order, (acc + bias) + residual: the reference
          does those in float32 and the comparison is == on the bits.
  gauss   float64 reference over the planes the kernel was given, hi*hi + hi*lo + lo*hi (hi*hi alone for SINGLE), and per element

              tol = 2 (P K + 8) 2^-24 (|X| |W| + |bias| + |residual or C0|),     P = 3 split, 1 single, K the padded contraction

          (the first-order bound of any float32 summation order over the P K products, + 8 for the epilogue's additions and the
          k-part sums, 2 for second order: the form of tests/train_blocks.py and tests/fine_blocks.py). A value stored to hi / lo
          planes adds one split, max(2^-22 |v|, 2^-25); a value stored to the hi plane ALONE (SINGLE's ReLU epilogue) adds one f16
          rounding instead, 2^-11 |v| + 2^-25 (half an ulp of an 11-bit significand; half the subnormal spacing 2^-24).

Attention: the bound of ``tests/fine_blocks.attention_b`` for its f32-MFMA arm with exact inputs, the logits over K = 256 and the
value sum over 32 key slots; EPS_EXP / EXP_TAIL / EPS_RCP / LOGIT_RANGE are that module's. LayerNorm: ``train_blocks.layer_tol``,
max(16 e32, 8 * 2^-24 max|ref|), + one split for the plane output.
"""
import functools

import numpy as np

from oracle import arith
from tests import fine_blocks as FB
from tests import train_blocks as TB

U = 2.0 ** -24
F16, F32, F64 = np.float16, np.float32, np.float64
TILE = 256
DM, FF, HEADS, HD = 1024, 4096, 4, 256
EPI_T32, EPI_RESID, EPI_RELU16, EPI_ROW = 0, 1, 2, 3
EPI_NAMES = {0: "T32", 1: "ResidT32", 2: "ReluT16", 3: "RowMajor"}
F16_SAFE = 3.0e4
SEED = 11
LN_EPS = float(np.float32(1e-5))


def ceil_to(n, m):
    return (n + m - 1) // m * m


def gauss32(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------
def t16_index(m, k, cols):
    """element index of (row m, column k) in a T16 plane of ``cols`` columns — the formula, element by element"""
    return ((m >> 5) * (cols >> 3) + (k >> 3)) * 256 + (m & 31) * 8 + (k & 7)


def t32_index(m, n, cols):
    return ((m >> 5) * (cols >> 2) + (n >> 2)) * 128 + (m & 31) * 4 + (n & 3)


def _pack(a, w):
    rows, cols = a.shape
    assert rows % 32 == 0 and cols % w == 0
    return np.ascontiguousarray(a.reshape(rows // 32, 32, cols // w, w).transpose(0, 2, 1, 3)).reshape(-1)


def _unpack(flat, rows, cols, w):
    return np.ascontiguousarray(flat.reshape(rows // 32, cols // w, 32, w).transpose(0, 2, 1, 3)).reshape(rows, cols)


def t16_pack(a):
    return _pack(a, 8)


def t16_unpack(flat, rows, cols):
    return _unpack(flat, rows, cols, 8)


def t32_pack(a):
    return _pack(a, 4)


def t32_unpack(flat, rows, cols):
    return _unpack(flat, rows, cols, 4)


def t16_unpack_swapped(flat, rows, cols):
    """NEGATIVE CONTROL: a reader that takes [rows / 32][32][cols / 8][8] for the layout (row and chunk swapped)"""
    return np.ascontiguousarray(flat.reshape(rows // 32, 32, cols // 8, 8)).reshape(rows, cols)


def pad_rows(a, rows_pad, fill=0):
    out = np.full((rows_pad,) + a.shape[1:], fill, dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


def split_f16(v):
    """RNE f16 of v, then RNE f16 of the float32 remainder"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(F16)
        lo = (v - hi.astype(F32)).astype(F16)
    return hi, lo


def join64(hi, lo):
    return hi.astype(F64) + lo.astype(F64)


def bf16_bits(v):
    """uint16 bit patterns of float64 values that ARE bf16 values (arith.bf16_rne / arith.split_bf16 outputs)"""
    return (np.ascontiguousarray(np.asarray(v, F64).astype(F32)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_values(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(F32).astype(F64)


def plane_store_tol(v, e, single=False):
    """what storing v (known within e) to planes adds: one split, or one f16 rounding for the hi plane alone"""
    a = np.abs(v) + e
    return 2.0 ** -11 * a + 2.0 ** -25 if single else np.maximum(2.0 ** -22 * a, 2.0 ** -25)


# ---------------------------------------------------------------------------------------------------------------------------
# the selection matrices of the exact cases
# ---------------------------------------------------------------------------------------------------------------------------
def selection(N, K_real):
    """(pi [N], sign [N]): column n of the output picks input column pi(n) < K_real with sign +-1. Within every 256-column n tile the
    k-steps (16 wide) are visited round-robin, so a tile picks from EVERY k-step (256 >= K / 16 for K <= 4096), the first and the
    last one of every k-part among them; the index within the step moves with the round and with the tile."""
    n = np.arange(N)
    j, t = n % TILE, n // TILE
    steps = (K_real + 15) // 16
    assert steps <= TILE
    pi = 16 * (j % steps) + (j // steps + 3 * j + 5 * t) % 16
    pi = np.minimum(pi, K_real - 1)
    sign = np.where(((n * 2654435761) >> 7) & 1, -1.0, 1.0)
    return pi, sign


def selection_matrix(N, K, K_real=None):
    pi, sign = selection(N, K if K_real is None else K_real)
    W = np.zeros((N, K), F32)
    W[np.arange(N), pi] = sign
    return W


# ---------------------------------------------------------------------------------------------------------------------------
# th_gemm (the f16 instances)
# ---------------------------------------------------------------------------------------------------------------------------
def grid_of(cus, m_tiles, n_tiles, ks=1):
    """text_head.hip: th_gemm_grid. Used to CHOOSE cases and to state jobs per workgroup; no reference depends on it."""
    return min(cus // 8 * 8, ceil_to(m_tiles, 8) * n_tiles * ks)


def jobs_per_workgroup(cus, m_tiles, n_tiles, ks=1):
    """[n_my of every workgroup] by the kernel's own rule (a prefix of vb = b + i grid; an m tile beyond m_tiles ends the list)"""
    grid, n_vb = grid_of(cus, m_tiles, n_tiles, ks), ceil_to(m_tiles, 8) * n_tiles * ks
    out = []
    for b in range(grid):
        n = 0
        for vb in range(b, n_vb, grid):
            if ((vb >> 3) // (n_tiles * ks)) * 8 + (b & 7) >= m_tiles:
                break
            n += 1
        out.append(n)
    return out


class GemmCase:
    """One th_gemm launch: planes, bias, residual, prior contents; ``kind`` gauss / exact."""

    def __init__(self, epi, single, K, n_tiles, M, cus, kind, n_real=None, relu=0, acc=0):
        self.epi, self.single, self.K, self.n_tiles, self.M, self.cus, self.kind = epi, int(single), K, n_tiles, M, cus, kind
        self.m_tiles = (M + TILE - 1) // TILE
        self.m_pad, self.N = self.m_tiles * TILE, n_tiles * TILE
        self.n_real = self.N if n_real is None else n_real
        self.relu, self.acc = relu, acc
        seed = (SEED, epi, K, n_tiles, M, kind == "exact")
        X = gauss32(seed + (0,), M, K)
        W = selection_matrix(self.N, K) if kind == "exact" else (gauss32(seed + (1,), self.N, K) * F32(K ** -0.5))
        self.xh, self.xl = split_f16(X)
        self.wh, self.wl = split_f16(W)
        self.bias = gauss32(seed + (2,), self.N)
        self.rh, self.rl = split_f16(gauss32(seed + (3,), M, self.N)) if epi == EPI_RESID else (None, None)
        self.C0 = gauss32(seed + (4,), M, self.n_real) if acc else None

    @property
    def name(self):
        s = f"{EPI_NAMES[self.epi]} {'single' if self.single else 'split'} {self.kind} K={self.K} nt={self.n_tiles} M={self.M} cus={self.cus}"
        return s + (f" n_real={self.n_real} relu={self.relu} acc={self.acc}" if self.epi == EPI_ROW else "")

    @property
    def P(self):
        return 1 if self.single else 3


MUTANTS = ("drop_last_kstep", "no_lohi", "resid_no_lo", "t16_swapped", "quad_shift", "bias_per_part", "relu_per_slab")


def _gemm_operands(c, mut):
    xh, xl, wh, wl = c.xh, c.xl, c.wh, c.wl
    if mut == "drop_last_kstep":
        xh, xl = xh.copy(), xl.copy()
        xh[:, -16:], xl[:, -16:] = 0, 0
    if mut == "no_lohi" or c.single:
        xl = np.zeros_like(xl)
    if c.single:
        wl = np.zeros_like(wl)
    if mut == "t16_swapped":
        sw = lambda p: t16_unpack_swapped(t16_pack(pad_rows(p, c.m_pad)), c.m_pad, c.K)[:c.M]
        xh, xl = sw(xh), sw(xl)
    rh, rl = c.rh, c.rl
    if mut == "resid_no_lo" and rl is not None:
        rl = np.zeros_like(rl)
    return xh, xl, wh, wl, rh, rl


def _quad_shift(out):
    out = out.copy()
    out[:, 8:12] = out[:, 12:16]  # the quad at columns 8..11 stored from the registers of the next one
    return out


def gemm_model(c, mut=None):
    """(value, tol) in float64 of the OUT the epilogue stores (before any split), real rows and real columns. ``mut``: a negative
    control on the reference side."""
    xh, xl, wh, wl, rh, rl = _gemm_operands(c, mut)
    XH, XL, WH, WL = (a.astype(F64) for a in (xh, xl, wh, wl))
    prod = XH @ WH.T
    if not c.single:
        prod = prod + XH @ WL.T + XL @ WH.T
    mag = np.abs(XH + XL) @ np.abs(WH + WL).T + np.abs(c.bias.astype(F64))
    ref = prod + c.bias.astype(F64)
    if c.epi == EPI_RESID:
        res = join64(rh, rl)
        ref, mag = ref + res, mag + np.abs(res)
    if c.epi == EPI_RELU16 or (c.epi == EPI_ROW and c.relu):
        ref = np.maximum(ref, 0.0)
    if c.epi == EPI_ROW:
        ref, mag = ref[:, :c.n_real], mag[:, :c.n_real]
        if c.acc:
            ref, mag = ref + c.C0.astype(F64), mag + np.abs(c.C0.astype(F64))
    if mut == "quad_shift":
        ref = _quad_shift(ref)
    return ref, 2.0 * (c.P * c.K + 8) * U * mag


def gemm_exact32(c, mut=None):
    """float32 OUT of an exact case in the kernel's order: acc = +-(hi + lo) of one element, (acc + bias) + residual, ReLU, + C0"""
    assert c.kind == "exact" and not c.wl.any()
    xh, xl, wh, wl, rh, rl = _gemm_operands(c, mut)
    pi, sign = selection(c.N, c.K)
    acc = (xh.astype(F32)[:, pi] + xl.astype(F32)[:, pi]) * sign.astype(F32)  # (both exact in float32)
    v = acc + c.bias
    if c.epi == EPI_RESID:
        v = v + (rh.astype(F32) + rl.astype(F32))
    if c.epi == EPI_RELU16 or (c.epi == EPI_ROW and c.relu):
        v = np.maximum(v, F32(0.0))
    if c.epi == EPI_ROW:
        v = v[:, :c.n_real]
        if c.acc:
            v = v + c.C0
    if mut == "quad_shift":
        v = _quad_shift(v)
    return v.astype(F32)


def gemm_product64(c):
    """the bare product of the planes in float64 (the exact cases: equal to the float32 gather, asserted on the CPU)"""
    xh, xl, wh, wl, _, _ = _gemm_operands(c, None)
    return (xh.astype(F64) + xl.astype(F64)) @ (wh.astype(F64) + wl.astype(F64)).T


# (K, n_tiles, M, CU override or None = the device's count). m_tiles: 1, 1, 1, 2, 9, 9, 2.
#   96 x 3 x 257 @ 8 and 1024 x 3 x 257 @ 8: 16 x 3 virtual blocks on 8 workgroups -> the two that have an m tile run 3 jobs (the
#       cross-tile prefetch, the NST waits);   96 x 3 x 2100 @ 8: workgroup 0 runs 6 jobs, 1..7 run 3 and leave at the `break`;
#   1024 x 1 x 2100 @ device: 16 workgroups, nine of them with exactly one job, seven with none.
GEMM_SHAPES = ((64, 1, 1, None), (96, 3, 255, 8), (1024, 1, 256, 32), (1024, 3, 257, 8), (96, 3, 2100, 8), (1024, 1, 2100, None),
               (96, 3, 257, 32))
RESID_K4096 = (4096, 3, 257, 8)
ROW_VARIANTS = tuple((n_real, relu, acc) for n_real in (4, 128, 252, 256) for relu in (0, 1) for acc in (0, 1))


@functools.lru_cache(maxsize=None)
def gemm_cases(epi, single, kind):
    out = []
    for K, nt, M, cus in GEMM_SHAPES + ((RESID_K4096,) if epi == EPI_RESID else ()):
        if epi == EPI_ROW:
            out.append(GemmCase(epi, single, K, nt, M, cus, kind, n_real=nt * TILE if nt > 1 else 256, relu=M & 1, acc=(M >> 1) & 1))
        else:
            out.append(GemmCase(epi, single, K, nt, M, cus, kind))
    if epi == EPI_ROW:  # n_real x relu x accumulate on two m tiles of the narrowest contraction
        out += [GemmCase(epi, single, 64, 1, 257, 8, kind, n_real=n, relu=r, acc=a) for n, r, a in ROW_VARIANTS]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# fast_gemm (bf16 planes, k-split)
# ---------------------------------------------------------------------------------------------------------------------------
def fast_ks(Mo, No, Kc):
    """text_head.hip: fast_ksplit. Restated ONLY to choose cases and to place the k-parts of the negative controls."""
    m_tiles, n_tiles, kt = (Mo + TILE - 1) // TILE, No // TILE, ceil_to(Kc, 64) >> 4
    ks = 1
    while ks < 8 and m_tiles * n_tiles * ks < 192 and kt % (ks * 4) == 0 and kt // (ks * 2) >= 8:
        ks *= 2
    return ks


FAST_MODES = ("plain", "plain_acc", "dW", "dX0", "dX1")
# (Mo, No, Kc) -> ks:  8 | 1 (k_pad 64 > Kc: the ring's minimum, four k-steps) | 1 (k_pad 128 > 96) | 1 (k_pad 192 > 160) | 2 | 4 | 8
FAST_SHAPES = ((64, 256, 1024), (65, 256, 32), (128, 1024, 96), (255, 512, 160), (257, 256, 256), (600, 512, 1152), (256, 1024, 1024))
FAST_KS = (8, 1, 1, 1, 2, 4, 8)


class FastCase:
    """fast_gemm as train.hip calls it. A2 [Mo, Kc] @ B2 [Kc, No] is the product; ``A``, ``B`` are the arrays in the memory layout the
    call takes (a_trans: [Kc][Mo]; b_trans: [Kc][No], else [No][Kc]). Modes: plain = Y = X W^T + b, ReLU; plain_acc = the same onto
    prior contents (bias + ReLU + accumulate together); dW = (a_trans, b_trans, accumulate, colsum); dX0 / dX1 = b_trans, accumulate 0 / 1."""

    def __init__(self, mode, single, Mo, No, Kc, cus, kind):
        self.mode, self.single, self.No, self.Kc, self.cus, self.kind = mode, int(single), No, Kc, cus, kind
        self.a_trans, self.b_trans = int(mode == "dW"), int(mode in ("dW", "dX0", "dX1"))
        if self.a_trans and Mo % 4:
            Mo = {65: 64, 255: 256, 257: 256}[Mo]
        self.Mo = Mo
        self.relu, self.has_bias = int(mode.startswith("plain")), mode.startswith("plain")
        self.acc = int(mode in ("plain_acc", "dW", "dX1"))
        self.k_pad, self.ks = ceil_to(Kc, 64), fast_ks(Mo, No, Kc)
        seed = (SEED, 77, FAST_MODES.index(mode), Mo, No, Kc, kind == "exact")
        self.A2 = gauss32(seed + (0,), Mo, Kc)
        self.B2 = selection_matrix(No, Kc).T.copy() if kind == "exact" else gauss32(seed + (1,), Kc, No) * F32(Kc ** -0.5)
        self.bias = gauss32(seed + (2,), No) if self.has_bias else None
        self.C0 = gauss32(seed + (3,), Mo, No) if self.acc else None
        self.cs0 = gauss32(seed + (4,), Mo) if mode == "dW" else None
        self.A = np.ascontiguousarray(self.A2.T) if self.a_trans else self.A2
        self.B = self.B2 if self.b_trans else np.ascontiguousarray(self.B2.T)
        self.ar = arith.BF16 if single else arith.SPLIT

    @property
    def name(self):
        return f"fast {self.mode} {'single' if self.single else 'split'} {self.kind} {self.Mo}x{self.No}x{self.Kc} ks={self.ks} cus={self.cus}"


def fast_model(c, mut=None):
    """(value, tol) in float64; the epilogue order is the kernel's and th_reduce_parts_kernel's: (sum + bias) -> ReLU -> + C0"""
    A, B = c.A2.astype(F64), c.B2.astype(F64)
    P = 1 if c.single else 3
    bias = c.bias.astype(F64) if c.has_bias else 0.0
    if mut in ("bias_per_part", "relu_per_slab", "drop_last_kstep"):
        step = c.k_pad // c.ks
        parts = []
        for kp in range(c.ks):
            lo, hi = kp * step, min((kp + 1) * step, c.Kc)
            if mut == "drop_last_kstep" and kp == c.ks - 1:
                hi = c.Kc - 16  # (the last k-step that holds real columns: the ones behind it are padding)
            parts.append(arith.product(A[:, lo:hi], B[lo:hi], c.ar) if hi > lo else np.zeros((c.Mo, c.No)))
        if mut == "bias_per_part":
            ref = sum(parts) + c.ks * bias
        elif mut == "relu_per_slab":
            ref = sum(np.maximum(p + (bias if i == 0 else 0.0), 0.0) if c.relu else p for i, p in enumerate(parts))
            if not c.relu:
                ref = ref + bias
        else:
            ref = sum(parts) + bias
    else:
        if mut == "no_lohi" and not c.single:
            ref = arith.product(A, B, arith.SPLIT_NO_LOHI)
        else:
            ref, _ = TB.linear(A, B, c.ar)
        ref = ref + bias
    mag = np.abs(A) @ np.abs(B) + np.abs(bias)
    if c.relu and mut != "relu_per_slab":
        ref = np.maximum(ref, 0.0)
    if c.acc:
        ref, mag = ref + c.C0.astype(F64), mag + np.abs(c.C0.astype(F64))
    if mut == "quad_shift":
        ref = _quad_shift(ref)
    return ref, 2.0 * (P * c.k_pad + 8) * U * mag


def fast_exact32(c, mut=None):
    assert c.kind == "exact"
    pi, sign = selection(c.No, c.Kc)
    hi, lo = arith.split_bf16(c.A2)
    if c.single or mut == "no_lohi":
        lo = np.zeros_like(lo)
    if mut == "drop_last_kstep":
        hi, lo = hi.copy(), lo.copy()
        hi[:, c.Kc - 16:], lo[:, c.Kc - 16:] = 0, 0
    acc = (hi.astype(F32)[:, pi] + lo.astype(F32)[:, pi]) * sign.astype(F32)
    v = acc
    if c.has_bias:
        v = v + (F32(c.ks) * c.bias if mut == "bias_per_part" else c.bias)
    if c.relu:
        v = np.maximum(v, F32(0.0))
    if c.acc:
        v = v + c.C0
    if mut == "quad_shift":
        v = _quad_shift(v)
    return v.astype(F32)


def fast_colsum(c):
    """(ref, tol) of the fused column sum of dW's transposed split: colsum[m] = cs0[m] + sum_k A[k][m]"""
    return TB.colsum(c.A.astype(F64), c.cs0.astype(F64))


@functools.lru_cache(maxsize=None)
def fast_cases(kind):
    out = []
    for i, (shape, ks) in enumerate(zip(FAST_SHAPES, FAST_KS)):
        for j, mode in enumerate(FAST_MODES):
            for single in (0, 1):
                c = FastCase(mode, single, *shape, cus=8 if (i + j + single) % 2 == 0 else None, kind=kind)
                out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# attention (th_attn_kernel<1024>)
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_L = (1, 2, 5, 13, 16, 17, 31, 32)


def attn_sentences(L):
    """a count whose last group of floor(32 / L) sentences is partial; with L = 5, 13, 17, 31 groups straddle a 32-row tile"""
    G = 32 // L
    return 3 * G + 1 if G > 1 else 3


def attn_reference(qkv, n_sent, L):
    """qkv float64 [n_sent L, 3072] -> (o, tol, zmin) [n_sent L, 1024] BEFORE the store's split; zmin the lowest shifted logit.
    tests/fine_blocks.attention_b with exact inputs, the f32 arm (P = 1), logits over K = 256, values over 32 key slots."""
    C, scale = FB.C, 1.0 / 16.0
    x = qkv.reshape(n_sent, L, 3, HEADS, HD)
    o, tol, zmin = np.zeros((n_sent, L, HEADS, HD)), np.zeros((n_sent, L, HEADS, HD)), 0.0
    for h in range(HEADS):
        q, k, v = x[:, :, 0, h], x[:, :, 1, h], x[:, :, 2, h]  # [n_sent, L, HD]
        s = scale * (q @ k.transpose(0, 2, 1))
        s_abs = scale * (np.abs(q) @ np.abs(k).transpose(0, 2, 1))
        z = s - s.max(axis=-1, keepdims=True)
        zmin = min(zmin, float(z.min()))
        e = np.exp(z)
        p = e / e.sum(axis=-1, keepdims=True)
        es = C * (HD + 8) * U * s_abs + C * U * (s_abs + np.abs(z))
        delta = es.max(axis=-1)
        rho = np.exp(np.minimum(2 * delta, 50.0)) * (1 + FB.ETA) - 1
        ep = np.minimum(p * rho[..., None] + np.where(z < -FB.LOGIT_RANGE, FB.EXP_TAIL * (1 + FB.ETA), 0.0), 1.0)
        av = np.abs(v)
        o[:, :, h] = p @ v
        tol[:, :, h] = ep @ av + C * (32 + 8) * U * (p @ av)
    return o.reshape(n_sent * L, DM), tol.reshape(n_sent * L, DM), zmin


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm (th_ln_kernel<false> / <true>)
# ---------------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 31, 32, 33, 300)
POOL_L = (1, 5, 13, 17, 32)


def ln_rows(y, gamma, beta, dtype):
    a = y.astype(dtype)
    a = a - a.mean(axis=1, keepdims=True, dtype=dtype)
    rstd = dtype(1.0) / np.sqrt((a * a).mean(axis=1, keepdims=True, dtype=dtype) + dtype(LN_EPS))
    return (a * rstd * gamma.astype(dtype) + beta.astype(dtype),)


def ln_reference(y, gamma, beta):
    """(ref, tol scalar) of the normalised rows, before any split"""
    ((ref, tol),) = TB.layer_tol(ln_rows, y, gamma, beta)
    return ref, tol


def ln_input(M, seed):
    """Gaussian rows; row 1: mean = 100 std; row 2: constant (where M allows)"""
    y = gauss32((SEED, 5, M, seed), M, DM)
    if M > 2:
        y[1] = y[1] + F32(100.0)
        y[2] = F32(0.1)
    return y


def pool_params(seed):
    """gamma ~ 1; beta by column: -8 (every token negative: the pooled max is negative), -1 (partial maxima of mixed sign), 0, +2"""
    rng = np.random.default_rng((SEED, 6, seed))
    gamma = (1.0 + 0.1 * rng.standard_normal(DM)).astype(F32)
    beta = np.array([-8.0, -1.0, 0.0, 2.0], F32)[rng.integers(0, 4, DM)]
    return gamma, beta


def pool_reference(rows, n_sent, L):
    return rows.reshape(n_sent, L, DM).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the stages of one t2l_text_head call (the door: t2l_blk_th_saved), each fed the kernel's own predecessor field
# ---------------------------------------------------------------------------------------------------------------------------
def planes_linear(xh, xl, W, bias, single, res=None, relu=False, w_known=True):
    """(ref, tol) of X W^T + bias (+ res) (ReLU) over the kernel's own X planes and the planes of the float32 weight W [N, K], which
    the test splits as the loader does (``w_known``); for a weight the loader FOLDS first (inter_mlp: Linear + BatchNorm in float32,
    four roundings) W is the float64 fold and the bound takes the representation error instead: 4 * 2^-24 + one split (2^-22, or
    2^-11 for the hi plane alone) relative to |X| |W|."""
    XH, XL = xh.astype(F64), (np.zeros(xl.shape) if single else xl.astype(F64))
    if w_known:
        wh, wl = split_f16(W)
        WH, WL = wh.astype(F64), (np.zeros(wl.shape) if single else wl.astype(F64))
    else:
        WH, WL = np.asarray(W, F64), np.zeros(W.shape)
    b = np.asarray(bias, F64)
    prod = XH @ WH.T + (0.0 if single else XH @ WL.T + XL @ WH.T)
    mag = np.abs(XH + XL) @ np.abs(WH + WL).T + np.abs(b)
    ref = prod + b
    P = 1 if single else 3
    tol = 2.0 * (P * XH.shape[1] + 8) * U * mag
    if not w_known:
        tol = tol + (4 * U + (2.0 ** -11 if single else 2.0 ** -22)) * mag
    if res is not None:
        ref, tol = ref + res, tol + 2.0 * (P * XH.shape[1] + 8) * U * np.abs(res)
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, tol


def ln_propagated(y, ey, gamma, beta):
    """(ref, tol [M, 1024]) of LayerNorm(y) for y known within ey: ``ln_reference``'s bound + the Jacobian's 2-norm bound
    max|gamma| ||ey||_2 / (sigma - ||ey||_2 / sqrt(D)) of tests/fine_blocks.layer_norm_b"""
    ref, tol = ln_reference(y, gamma, beta)
    mu = y.mean(axis=1, keepdims=True)
    sig = np.sqrt(((y - mu) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
    nrm = np.sqrt((ey * ey).sum(axis=1, keepdims=True))
    return ref, tol + np.abs(gamma).max() * nrm / (sig - nrm / np.sqrt(DM)) + np.zeros_like(ref)


def fold_bn(W, b, g, beta, mean, var, eps=1e-5):
    """Linear + BatchNorm1d (eval) folded, in float64"""
    s = np.asarray(g, F64) / np.sqrt(np.asarray(var, F64) + eps)
    return np.asarray(W, F64) * s[:, None], (np.asarray(b, F64) - np.asarray(mean, F64)) * s + np.asarray(beta, F64)


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library
# ---------------------------------------------------------------------------------------------------------------------------
def blocks_path():
    import os.path as osp

    return osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "text2loc_amd", "libt2l_blocks.so")


def declare(lib):
    import ctypes as C

    p, i, l = C.c_void_p, C.c_int, C.c_int64
    ip = C.POINTER(C.c_int)
    sigs = {
        "t2l_blk_th_set_cus": [i],
        "t2l_blk_th_cus": [],
        "t2l_blk_th_grid": [i, i, i],
        "t2l_blk_th_split": [p, i, i, i, p, p, p],
        "t2l_blk_th_split_bf16": [i, p, i, i, p, p, l, p, ip, ip],
        "t2l_blk_th_gemm": [i, i, p, p, p, p, p, p, p, p, p, p, i, i, i, i, i, i, i, i],
        "t2l_blk_th_attn": [p, i, i, p, p, p],
        "t2l_blk_th_ln": [i, p, p, p, i, i, i, p, p, p, p],
        "t2l_blk_fast_gemm": [p, p, i, p, i, p, p, i, i, i, i, i, i, p, ip],
        "t2l_blk_th_saved": [p, C.c_char_p, p, l, C.POINTER(l)],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    lib.t2l_blk_last_error.restype = C.c_char_p
    lib.t2l_blk_last_error.argtypes = []
    return lib


def load_blocks():
    import ctypes as C

    return declare(C.CDLL(blocks_path()))  # OSError if it was not built: there is no fallback
