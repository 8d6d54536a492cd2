"""TEST INFRASTRUCTURE — float64 references, derived tolerances and the case lists of the fine-stage training-block tier
(tests/test_fine_train_blocks_cpu.py, tests/test_gpu_fine_train_blocks.py; profiles/fine_train_blocks.md).

The nine kernels csrc/fine_train.hip brings of its own — k_gemm behind lin_fwd / lin_dx / lin_dw, k_colsum, k_bn_fwd / k_bn_bwd,
k_attn_fwd / k_attn_bwd, k_gather / k_scatter_add / k_num_in — one launch at a time through csrc/fine_train_blocks.hip, then the wiring of
the step (which slice, site, buffer and role) through the saved activations of the product's own forward and one call of its dec_bwd.
numpy only; the arithmetic comes from ``oracle.arith`` and ``oracle.t2l_oracle_train.dropout_keep``, never from the product. Masks and
arg-max are INPUTS of every reference, taken from the tensors the kernel itself reads, so each block is a continuous function of its
inputs and no ReLU or arg-max flip can occur.  u = 2^-24; the tier's factor 2 covers second order everywhere.

Products.  ``train_blocks.linear`` / ``colsum`` as they stand: per element 2 (K + 8) u (|A| @ |B| + |bias| + |C0|), K the FULL
reduction length (for lin_dw the row count M; the split's atomics sit inside the + 8).

BatchNorm (k_bn_fwd).  Sums run in float64 (their error, M 2^-53, is nothing beside u). mean is rounded to float32 once (u |mean|);
rstd = 1.f / sqrtf((float)var + eps): the conversion and the addition perturb var + eps by 2u, i.e. rstd by u, sqrtf and the division are
correctly rounded (u each): 3u. x̂ = (y - mean) * rstd: one subtraction, one multiplication. First order

    |d x̂| <= u (rstd |mean| + 5 |x̂|) <= C_BN_FWD u (rstd (|y| + |mean|) + |x̂|),   C_BN_FWD = 5
    |d out| <= |g| |d x̂| + u |x̂ g + b|      (one fma; ReLU is 1-Lipschitz)        |d rstd| <= 3u rstd
    |d rm| <= 4u (0.9 |rm| + 0.1 |mean|)      (the float32 constants 0.1f and 1.f - 0.1f, the rounded mean, product and sum; the same for
                                               rv with the UNBIASED variance var M / (M - 1))

BatchNorm backward (k_bn_bwd), dz = dout where the out it is handed is > 0: k = g rstd / M (2u), the two sums rounded to float32 (u
each), M dz, x̂ Σdz·x̂, two subtractions and the last product:

    |d dy| <= C_BN_BWD u |k| (M |dz| + |Σ dz| + |x̂| |Σ dz x̂|),   C_BN_BWD = 7        dg, db: 2u (|dg0| + |Σ|) (rounding, addition)

Attention (k_attn_fwd / k_attn_bwd; ``__expf``).  The probability bound of tests/fine_blocks.py with its EPS_EXP, EXP_TAIL, EPS_RCP (ETA):
the logit error delta = 2 (32 + 8) u s_abs + 2 u (s_abs + |z|), p within p [e^(2 delta) (1 + ETA) - 1] (+ EXP_TAIL below -LOGIT_RANGE),
then linearly to O = (P f) V over Tk slots and, in the backward, from dP = f (dO Vᵀ) through r = Σ P dP and dS = P (dP - r) / sqrt(32) to
dQ = dS K, dK = dSᵀ Q, dV = (P f)ᵀ dO, every product under 2 (K + 8) u |.| @ |.|.

Gather is bit-equal; scatter is ``colsum`` with each row's multiplicity for its row count; k_num_in is within 2u |ref| (two correctly
rounded operations).

Stages of the chain that are ONE launch use the bounds above; stages that are two launches use the tier's layer rule
``train_blocks.layer_tol``: max(16 e32, 8 u max|ref|).
"""
import numpy as np

from oracle import arith
from oracle.t2l_oracle_train import NUM_MEAN, NUM_STD
from tests import train_blocks as TB
from tests.fine_blocks import EPS_EXP, EPS_RCP, ETA, EXP_TAIL, LOGIT_RANGE, SCALE, ratio, weights  # noqa: F401 (re-exported)

U = TB.U
C = 2.0
F32 = np.float32
EX = arith.EXACT
P_DROP = TB.P_DROP
BN_EPS = float(F32(1e-5))
BN_MOM = 0.1  # the reference's momentum; the kernel's 0.1f is inside the 4u of rm / rv
C_BN_FWD, C_BN_BWD = 5.0, 7.0
D, HEADS, HD, FF, OBJ = 128, 4, 32, 512, 16
SEED = 7
BRANCHES = ("class", "color", "position", "num")
DEC_FIELDS = ("qkv", "Ps", "os", "xh1", "r1", "x1", "q2", "kv2", "Pc", "oc", "xh2", "r2", "x2", "h1", "h1d", "xh3", "r3", "out")
DEC_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias",
              "norm3.weight", "norm3.bias")

gauss = TB.gauss


# ---------------------------------------------------------------------------------------------------------------------------
# products: lin_fwd, lin_dx, lin_dw (+ k_colsum)
# ---------------------------------------------------------------------------------------------------------------------------
# 256 / 257: the boundary of lin_dw's split over the rows; 272 and 513 leave a last slice of 16 rows and of 1 row
ROWS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 272, 513)
# (N, K, sliced): K below the 16-wide k tile | N below the 4-wide thread tile | the feed-forward pair | the packed in-projection |
# the cross-attention k / v slice: W and b start 128 * 128 / 128 elements into a [384, 128] / [384] tensor
WIDTHS = ((64, 1, False), (64, 3, False), (2, 64, False), (128, 512, False), (512, 128, False), (384, 128, False), (256, 128, True))
SLICE_ROWS = 128


class LinCase:
    """Operands of one (M, N, K): float64 arrays of exact float32 values. W is [N, K]; for the sliced case ``Wfull`` / ``bfull`` /
    ``dW0full`` / ``db0full`` are the [384, .] tensors whose rows 128.. are W, b, dW0, db0."""

    def __init__(self, M, N, K, sliced=False):
        self.M, self.N, self.K, self.sliced = M, N, K, sliced
        s = (SEED, 0xF7, M, N, K)
        rows = N + (SLICE_ROWS if sliced else 0)
        self.X, self.dY = gauss(s + (0,), M, K), gauss(s + (1,), M, N)
        self.Wfull, self.bfull = gauss(s + (2,), rows, K), gauss(s + (3,), rows)
        self.dW0full, self.db0full, self.dX0 = gauss(s + (4,), rows, K), gauss(s + (5,), rows), gauss(s + (6,), M, K)
        o = rows - N
        self.W, self.b, self.dW0, self.db0 = self.Wfull[o:], self.bfull[o:], self.dW0full[o:], self.db0full[o:]


def lin_fwd_ref(c, bias=True, relu=False, mut=None):
    X, W, b = c.X, c.W, c.b
    if mut == "no_slice":  # the k / v rows taken from the START of the [384, 128] tensor
        W, b = c.Wfull[:c.N], c.bfull[:c.N]
    if mut == "last_k_tile":  # the k tile that holds the last reduction index dropped
        k0 = (c.K - 1) // 16 * 16
        X, W = X[:, :k0], W[:, :k0]
    ref, tol = TB.linear(X, W.T, EX, bias=b if bias else None, relu=relu)
    return (ref, tol) if mut is None else ref


def lin_dx_ref(c, acc, mut=None):
    ref, tol = TB.linear(c.dY, c.W, EX, C0=c.dX0 if (acc and mut != "no_acc") else None)
    return (ref, tol) if mut is None else ref


def dw_slices(M):
    """(rows per slice, slices) of lin_dw's split: used by the negative controls only"""
    return (256, (M + 255) // 256) if M > 256 else (M, 1)


def lin_dw_ref(c, mut=None):
    """{dW, db}: dW0 + dYᵀ X over the full row count M, db0 + the column sums of dY"""
    dY, X = c.dY, c.X
    chunk, z = dw_slices(c.M)
    if mut == "last_k_tile":  # the last 16-row k tile of the last slice
        k0 = (c.M - 1) // 16 * 16
        dY, X = dY[:k0], X[:k0]
    if mut == "slice_boundary" and z > 1:  # a slice one row short: row 255 is in no slice
        keep = np.arange(c.M) != chunk - 1
        dY, X = dY[keep], X[keep]
    dW = TB.linear(dY.T, X, EX, C0=c.dW0)
    if mut == "bias_on_split" and z > 1:  # the non-split epilogue's bias add (a vector over the output's columns) run by every slice
        dW = (dW[0] + z * c.dX0[0][None, :], dW[1])
    db = TB.colsum(c.dY, c.db0)
    if mut is None:
        # the bound's K is the FULL row count whatever the operands a control drops
        return {"dW": dW, "db": db}
    return {"dW": dW[0], "db": db[0]}


def f32_lin(A, B, bias=None, C0=None, relu=False):
    """float32 numpy of the same product (what a correct float32 kernel may return), as float64"""
    out = A.astype(F32) @ B.astype(F32)
    if bias is not None:
        out = out + bias.astype(F32)
    if C0 is not None:
        out = out + C0.astype(F32)
    return (np.maximum(out, F32(0)) if relu else out).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm1d (batch statistics) + ReLU, and its backward
# ---------------------------------------------------------------------------------------------------------------------------
BN_ROWS = (16, 255, 256, 257, 528)
BN_COLS = (64, 128)


def bn_fwd(Y, g, b, rm, rv, dtype=np.float64, mut=None):
    """-> dict xhat, out, rstd, rm, rv (rm / rv None when not given), in ``dtype`` with the kernel's float64 sums. Y [M, N]."""
    M = Y.shape[0]
    Y64 = Y.astype(np.float64)
    mean = Y64.mean(axis=0)
    var = ((Y64 - mean) ** 2).mean(axis=0)
    if mut == "onepass":  # E[y^2] - mean^2 in float32
        y32 = Y.astype(F32)
        m32 = y32.mean(axis=0, dtype=F32)
        var = np.maximum(((y32 * y32).mean(axis=0, dtype=F32) - m32 * m32).astype(np.float64), 0.0)
    t = dtype
    mf = mean.astype(t)
    rstd = t(1.0) / np.sqrt(var.astype(t) + t(BN_EPS))
    xhat = (Y.astype(t) - mf) * rstd
    out = np.maximum(xhat * g.astype(t) + b.astype(t), t(0.0))
    res = {"xhat": xhat, "out": out, "rstd": rstd, "rm": None, "rv": None}
    unb = var if mut == "biased_rv" else var * M / max(M - 1, 1)
    if rm is not None:
        res["rm"] = (t(1.0) - t(BN_MOM)) * rm.astype(t) + t(BN_MOM) * mf
    if rv is not None:
        res["rv"] = (t(1.0) - t(BN_MOM)) * rv.astype(t) + t(BN_MOM) * unb.astype(t)
    return res


def bn_fwd_ref(Y, g, b, rm, rv):
    """{name: (ref, tol)} of one k_bn_fwd launch on the pre-BN rows Y"""
    M = Y.shape[0]
    r = bn_fwd(Y, g, b, rm, rv)
    mean = Y.mean(axis=0)
    var_unb = ((Y - mean) ** 2).mean(axis=0) * M / max(M - 1, 1)
    e_xh = C * C_BN_FWD * U * (r["rstd"] * (np.abs(Y) + np.abs(mean)) + np.abs(r["xhat"]))
    out = {"xhat": (r["xhat"], e_xh), "out": (r["out"], np.abs(g) * e_xh + C * U * np.abs(r["xhat"] * g + b)),
           "rstd": (r["rstd"], C * 3 * U * r["rstd"])}
    if rm is not None:
        out["rm"] = (r["rm"], C * 4 * U * ((1 - BN_MOM) * np.abs(rm) + BN_MOM * np.abs(mean)))
    if rv is not None:
        out["rv"] = (r["rv"], C * 4 * U * ((1 - BN_MOM) * np.abs(rv) + BN_MOM * var_unb))
    return out


def bn_bwd(dout, out, xhat, rstd, g, dg0, db0, dtype=np.float64, mut=None):
    """-> dict dy, dg, db (dg / db None when dg0 / db0 is): the ReLU mask is read from ``out``"""
    M = dout.shape[0]
    t = dtype
    mask = (dout if mut == "mask_dout" else out) > 0
    dz = np.where(mask, dout, 0.0)
    sd, sdx = dz.sum(axis=0), (dz * xhat).sum(axis=0)  # float64, as the kernel
    k = g.astype(t) * rstd.astype(t) / t(M)
    dy = k * (t(M) * dz.astype(t) - sd.astype(t) - xhat.astype(t) * sdx.astype(t))
    res = {"dy": dy, "dg": None, "db": None}
    if dg0 is not None:
        res["dg"] = sdx.astype(t) + (t(0.0) if mut == "dg_overwrite" else dg0.astype(t))
    if db0 is not None:
        res["db"] = sd.astype(t) + db0.astype(t)
    return res


def bn_bwd_ref(dout, out, xhat, rstd, g, dg0, db0):
    M = dout.shape[0]
    r = bn_bwd(dout, out, xhat, rstd, g, dg0, db0)
    dz = np.where(out > 0, dout, 0.0)
    sd, sdx = dz.sum(axis=0), (dz * xhat).sum(axis=0)
    k = np.abs(g * rstd) / M
    res = {"dy": (r["dy"], C * C_BN_BWD * U * k * (M * np.abs(dz) + np.abs(sd) + np.abs(xhat) * np.abs(sdx)))}
    dbl = M * 2.0 ** -52  # the float64 sums themselves
    if dg0 is not None:
        res["dg"] = (r["dg"], C * 2 * U * (np.abs(dg0) + np.abs(sdx)) + dbl * np.abs(dz * xhat).sum(axis=0))
    if db0 is not None:
        res["db"] = (r["db"], C * 2 * U * (np.abs(db0) + np.abs(sd)) + dbl * np.abs(dz).sum(axis=0))
    return res


def bn_case(M, N, kind="plain"):
    """(Y, g, b, rm, rv) float64 arrays of exact float32 values. kind 'offset': every column has |mean| = 100 std; 'constant': the even
    columns are exactly constant"""
    s = (SEED, 0xB7, M, N)
    Y = gauss(s + (0,), M, N)
    if kind == "offset":
        sign = np.where(np.arange(N) % 2, -1.0, 1.0)
        Y = (100.0 * sign + Y).astype(F32).astype(np.float64)
    if kind == "constant":
        Y[:, ::2] = gauss(s + (5,), N)[::2]
    g, b = 1.0 + 0.5 * gauss(s + (1,), N), 0.3 * gauss(s + (2,), N)
    rm, rv = gauss(s + (3,), N), 1.0 + np.abs(gauss(s + (4,), N))
    f = lambda a: a.astype(F32).astype(np.float64)
    return Y, f(g), f(b), f(rm), f(rv)


def bn_bwd_case(M, N, kind="plain"):
    """(dout, out, xhat, rstd, g, dg0, db0): ``out`` is an INPUT — zeros in about half of it, independent of dout's sign"""
    Y, g, b, _, _ = bn_case(M, N, kind)
    s = (SEED, 0xB8, M, N)
    r = bn_fwd(Y, g, b, None, None)
    f = lambda a: a.astype(F32).astype(np.float64)
    out = np.where(gauss(s + (1,), M, N) > 0, np.abs(gauss(s + (2,), M, N)), 0.0)
    return gauss(s + (0,), M, N), out, f(r["xhat"]), f(r["rstd"]), g, gauss(s + (3,), N), gauss(s + (4,), N)


# ---------------------------------------------------------------------------------------------------------------------------
# cross-attention: Tq x Tk, separate strides; factor [pairs, 4, Tq, Tk] at index ((pair * 4 + head) * Tq + i) * Tk + j
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = ((16, 16), (16, 1), (1, 16), (1, 1), (16, 8), (8, 16), (3, 5))
ATTN_PAIRS = (1, 3)


def _heads(X, pairs, T, stride=HD):
    """[pairs * T, 128] -> [pairs, 4, T, 32] (``stride``: the column distance of two heads — a control)"""
    X = X.reshape(pairs, T, D)
    return np.stack([X[:, :, h * stride:h * stride + HD] for h in range(HEADS)], axis=1)


def _rows(x):
    pairs, _, T, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(pairs * T, D)


def attn_factor(seed, site, p, pairs, Tq, Tk, mut=None):
    if mut == "mask_transposed" and p > 0:  # the factor read at j * Tq + i
        f = TB.drop_factor(seed, site, p, (pairs, HEADS, Tk, Tq))
        return np.ascontiguousarray(f.transpose(0, 1, 3, 2))
    return TB.drop_factor(seed, site, p, (pairs, HEADS, Tq, Tk))


def xattn_fwd(Q, K, V, pairs, Tq, Tk, factor, dtype=np.float64, mut=None):
    """-> (P [pairs, 4, Tq, Tk] before dropout, O [pairs * Tq, 128], z: the logits below their row's maximum)"""
    t = dtype
    stride = 16 if mut == "head_stride" else HD
    q, k, v = (_heads(a.astype(t), pairs, T, stride) for a, T in ((Q, Tq), (K, Tk), (V, Tk)))
    s = (q @ k.transpose(0, 1, 3, 2)) * t(1.0 / np.sqrt(D) if mut == "scale_128" else SCALE)
    z = s - s.max(axis=-1, keepdims=True)
    e = np.exp(z)
    P = e / e.sum(axis=-1, keepdims=True)
    O = (P * factor.astype(t)) @ v
    if mut == "mask_saved":  # the dropout applied to P before it is saved
        P = P * factor.astype(t)
    return P, _rows(O), z


def xattn_fwd_ref(Q, K, V, pairs, Tq, Tk, factor):
    """({P, O: (ref, tol)}, the logit spread)"""
    P, O, z = xattn_fwd(Q, K, V, pairs, Tq, Tk, factor)
    aq, ak, av = (_heads(np.abs(a), pairs, T) for a, T in ((Q, Tq), (K, Tk), (V, Tk)))
    s_abs = SCALE * (aq @ ak.transpose(0, 1, 3, 2))
    es = C * (HD + 8) * U * s_abs + C * U * (s_abs + np.abs(z))
    delta = es.max(axis=-1, keepdims=True)
    rho = np.exp(np.minimum(2 * delta, 50.0)) * (1 + ETA) - 1
    eP = np.minimum(P * rho + np.where(z < -LOGIT_RANGE, EXP_TAIL * (1 + ETA), 0.0), 1.0)
    eO = (eP * factor) @ av + C * (Tk + 8) * U * ((P * factor) @ av)
    return {"P": (P, eP), "O": (O, _rows(eO))}, float(-z.min())


def xattn_bwd(Q, K, V, P, dO, pairs, Tq, Tk, factor, dtype=np.float64, mut=None):
    """-> (dQ [pairs * Tq, 128], dK, dV [pairs * Tk, 128])"""
    t = dtype
    stride = 16 if mut == "head_stride" else HD
    q, k, v, go = (_heads(a.astype(t), pairs, T, stride) for a, T in ((Q, Tq), (K, Tk), (V, Tk), (dO, Tq)))
    P, m = P.astype(t), factor.astype(t)
    sc = t(1.0 / np.sqrt(D) if mut == "scale_128" else SCALE)
    dV = (P * m).transpose(0, 1, 3, 2) @ go
    dP = m * (go @ v.transpose(0, 1, 3, 2))
    r = (dP * P).sum(axis=-1, keepdims=True)
    dS = P * (dP - r) * sc
    return _rows(dS @ k), _rows(dS.transpose(0, 1, 3, 2) @ q), _rows(dV)


def xattn_bwd_ref(Q, K, V, P, dO, pairs, Tq, Tk, factor):
    dQ, dK, dV = xattn_bwd(Q, K, V, P, dO, pairs, Tq, Tk, factor)
    q, k, v, go = (_heads(a, pairs, T) for a, T in ((Q, Tq), (K, Tk), (V, Tk), (dO, Tq)))
    aq, ak, av, ago = np.abs(q), np.abs(k), np.abs(v), np.abs(go)
    T_ = lambda a: a.transpose(0, 1, 3, 2)
    pd = np.abs(P * factor)
    e_dV = C * (Tq + 8) * U * (T_(pd) @ ago)
    dP = factor * (go @ T_(v))
    e_dP = C * (HD + 8) * U * factor * (ago @ T_(av))
    r = (dP * P).sum(axis=-1, keepdims=True)
    e_r = (P * e_dP).sum(axis=-1, keepdims=True) + C * (Tk + 8) * U * np.abs(P * dP).sum(axis=-1, keepdims=True)
    dS = P * (dP - r) * SCALE
    e_dS = P * SCALE * (e_dP + e_r) + C * 3 * U * P * (np.abs(dP) + np.abs(r)) * SCALE
    e_dQ = e_dS @ ak + C * (Tk + 8) * U * (np.abs(dS) @ ak)
    e_dK = T_(e_dS) @ aq + C * (Tq + 8) * U * (T_(np.abs(dS)) @ aq)
    return {"dQ": (dQ, _rows(e_dQ)), "dK": (dK, _rows(e_dK)), "dV": (dV, _rows(e_dV))}


def attn_case(pairs, Tq, Tk):
    """(Q [pairs Tq, 128], K, V [pairs Tk, 128], dO [pairs Tq, 128])"""
    s = (SEED, 0xA7, pairs, Tq, Tk)
    return gauss(s + (0,), pairs * Tq, D), gauss(s + (1,), pairs * Tk, D), gauss(s + (2,), pairs * Tk, D), gauss(s + (3,), pairs * Tq, D)


# ---------------------------------------------------------------------------------------------------------------------------
# nn.Embedding lookup, its backward, num_encoder's input
# ---------------------------------------------------------------------------------------------------------------------------
def gather_ref(table, idx, mut=None):
    rows = table.shape[0]
    ok = (idx >= 0) & (idx <= rows if mut == "row_eq_rows" else idx < rows)
    return np.where(ok[:, None], table[np.where(ok, idx, 0) % rows], 0.0)


def scatter_ref(dY, idx, grad0, mut=None):
    """(ref, tol): grad0[r] + the sum of the rows of dY whose index is r, for 0 < r < rows (``colsum`` per table row)"""
    rows = grad0.shape[0]
    ref, tol = grad0.copy(), np.zeros_like(grad0)  # a row nothing is added to keeps its bits
    for r in range(rows):
        hit = idx == r
        if mut == "row_eq_rows" and r == rows - 1:
            hit = hit | (idx == rows)
        if (r == 0 and mut != "pad_grad") or not hit.any():
            continue
        ref[r], tol[r] = TB.colsum(dY[hit], grad0[r])
    return ref, tol


def index_case(M, rows, seed=0):
    """indices with 0 (padding), negatives, == rows, beyond, and one heavily duplicated row"""
    rng = np.random.default_rng((SEED, 0x1D, M, rows, seed))
    idx = rng.integers(-2, rows + 2, M).astype(np.int32)
    idx[rng.random(M) < 0.4] = rows // 2  # heavy duplicates
    edge = np.array([0, -1, rows, rows - 1, 1, 0, rows + 1, -(2 ** 31)], np.int64)[:M]
    idx[:edge.size] = edge
    return idx


def num_in_ref(n_pts):
    """(ref, tol): (n - mean) / std with the float32 constants of the reference"""
    ref = (n_pts - float(F32(NUM_MEAN))) / float(F32(NUM_STD))
    return ref, 2 * U * np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the step: configurations, the forward chain stage by stage, one layer's backward
# ---------------------------------------------------------------------------------------------------------------------------
class Config:
    def __init__(self, P, H, L, use, embed):
        self.P, self.H, self.L, self.use, self.embed = P, H, L, tuple(f for f in BRANCHES if f in use), embed
        self.n_feat = len(self.use)
        self.pn_stats = not embed and "class" not in self.use
        self.needs_pn = not embed
        # cascade order: (state-dict prefix, obj: the 16 objects are the target, first dropout site)
        self.layers = [("cross_hints", False, 0)] if L == 0 else [
            x for i in range(L) for x in ((f"cross_objects.{i}", True, 12 * i), (f"cross_hints.{i}", False, 12 * i + 6))]

    def __repr__(self):
        return f"P{self.P}-H{self.H}-L{self.L}-{'+'.join(self.use)}-{'embed' if self.embed else 'pn'}"

    def t(self, layer):
        """(Tq, Tk) of a cascade layer"""
        return (OBJ, self.H) if self.layers[layer][1] else (self.H, OBJ)


CONFIGS = (Config(1, 1, 0, BRANCHES, True), Config(3, 5, 1, BRANCHES, False), Config(17, 8, 2, BRANCHES, True),
           Config(3, 8, 1, ("color", "num"), False))


def problem(cfg, seed=0):
    """(sd float32 state dict, inp): inp has the packed cells' arrays, hints [P, H, 128], pn [16 P, 256] or None, gout [P, 2]"""
    from text2loc_amd import synth

    sd = weights(cfg.L, seed + 7)
    if cfg.n_feat > 1:
        sd["object_encoder.mlp_merge.0.0.weight"] = np.ascontiguousarray(sd["object_encoder.mlp_merge.0.0.weight"][:, :D * cfg.n_feat])
    cells = synth.make_cells(cfg.P, seed=seed + 3, min_obj=OBJ, max_obj=OBJ)
    rng = np.random.default_rng((seed + 11, cfg.P, cfg.H))
    inp = {k: v for k, v in cells.items() if k != "counts"}
    inp["class_idx"] = inp["class_idx"].copy()
    inp["class_idx"][::5] = 0  # padding rows: read, no gradient
    inp["hints"] = rng.standard_normal((cfg.P, cfg.H, D)).astype(F32)
    inp["pn"] = rng.standard_normal((cfg.P * OBJ, 256)).astype(F32) if cfg.needs_pn else None
    inp["gout"] = rng.standard_normal((cfg.P, 2)).astype(F32)
    return sd, inp


def _w(sd, name):
    return np.asarray(sd[name], np.float64)


def branch_plan(cfg, f):
    """(kind, state-dict prefix, input key, layer sizes) of feature branch f"""
    oe = "object_encoder."
    if f == "class":
        return ("embed", oe + "class_embedding.weight", "class_idx", ()) if cfg.embed else ("mlp", oe + "mlp_pointnet", "pn", ((256, D),))
    if f == "color":
        return ("embed", oe + "color_embedding.weight", "color_idx", ()) if cfg.embed else ("mlp", oe + "color_encoder", "rgb", ((3, 64), (64, D)))
    if f == "position":
        return ("mlp", oe + "pos_encoder", "center", ((3, 64), (64, D)))
    return ("mlp", oe + "num_encoder", "n_pts", ((1, 64), (64, D)))


def _layer(fn, args, dtype):
    """the tier's layer rule: [(value in ``dtype`` as float64, tol)] per output of fn(*args, dtype)"""
    out = TB.layer_tol(fn, *args)
    if dtype is np.float64:
        return out
    return [(v.astype(np.float64), tol) for v, (_, tol) in zip(fn(*args, dtype), out)]


def _prod(A, W, b, dtype, relu=False):
    """one lin_fwd launch: (value, tol) under the product bound"""
    ref, tol = TB.linear(A, W.T, EX, bias=b, relu=relu)
    return (ref if dtype is np.float64 else f32_lin(A, W.T, bias=b, relu=relu)), tol


def _bn_layer(x, W, b, g, beta, rm, rv, dtype):
    """Linear + BatchNorm + ReLU (two launches) -> (xhat, out, rstd, rm, rv)"""
    y = x.astype(dtype) @ W.astype(dtype).T + b.astype(dtype)
    r = bn_fwd(y, g, beta, rm, rv, dtype)
    return r["xhat"], r["out"], r["rstd"], r["rm"], r["rv"]


def _proj_ln(x, a, W, b, g, beta, factor, dtype):
    """out-projection / linear2 into the scratch rows, then residual + dropout + LayerNorm (two launches) -> (out, xhat, rstd)"""
    y = a.astype(dtype) @ W.astype(dtype).T + b.astype(dtype)
    return TB.ln_fwd(x, y, g, beta, factor, dtype)


def forward_chain(cfg, sd, inp, seed, p, saved=None, dtype=np.float64, running0=None, mut=None):
    """{key: (value, tol)} of every saved field of one forward, stage by stage. key: (layer, field) with layer -1 the encoder, plus
    (-1, 'offsets') and (-1, 'run:<buffer name>') for the BatchNorm running buffers after the step. ``saved`` {key: float64 array}: the
    kernel's own saved tensors — every stage is fed ITS predecessors from there; None: chained (each stage fed the reference before it).
    ``dtype`` float32: every stage's value from a float32 numpy run of the same reference (tolerances stay the float64 run's).
    ``running0``: the running buffers before the step (default: the state dict's)."""
    out = {}
    get = (lambda k: out[k][0]) if saved is None else (lambda k: np.asarray(saved[k], np.float64))
    M0 = cfg.P * OBJ
    zero = np.zeros(())
    run = (lambda n: _w(sd, n)) if running0 is None else (lambda n: np.asarray(running0[n], np.float64))

    def bn_stage(pre, key, x):
        W, b, g, beta = (_w(sd, pre + s) for s in (".0.weight", ".0.bias", ".1.weight", ".1.bias"))
        r = _layer(_bn_layer, (x, W, b, g, beta, run(pre + ".1.running_mean"), run(pre + ".1.running_var")), dtype)
        for name, v in zip(("xhat", "out", "rstd"), r):
            out[(-1, f"{key}.{name}")] = v
        out[(-1, f"run:{pre}.1.running_mean")], out[(-1, f"run:{pre}.1.running_var")] = r[3], r[4]

    cols = []
    for f in cfg.use:
        kind, pre, src, sizes = branch_plan(cfg, f)
        if kind == "embed":
            out[(-1, f + ".raw")] = (gather_ref(_w(sd, pre), np.asarray(inp[src])), zero)
            last = (-1, f + ".raw")
        else:
            x = np.asarray(inp[src], np.float64).reshape(M0, -1)
            if f == "num":
                out[(-1, "num.in")] = num_in_ref(x[:, 0])
                # chained: the float32 value the reference model itself feeds num_encoder (two float32 operations on the host)
                x = (get((-1, "num.in")) if saved is not None else
                     ((x[:, 0].astype(F32) - F32(NUM_MEAN)) / F32(NUM_STD)).astype(np.float64)).reshape(M0, 1)
            for li in range(len(sizes)):
                bn_stage(f"{pre}.{li}", f"{f}.{li}", x if li == 0 else get((-1, f"{f}.{li - 1}.out")))
            last = (-1, f"{f}.{len(sizes) - 1}.out")
        (y, ty), (n, tn) = _layer(TB.rownorm_fwd, (get(last),), dtype)
        out[(-1, f + ".nrm")] = (n, tn)
        cols.append((y, ty))
    if mut == "E_order":
        cols = cols[1:] + cols[:1]
    out[(-1, "E")] = (np.concatenate([c[0] for c in cols], axis=1), np.concatenate([np.broadcast_to(c[1], c[0].shape) for c in cols], axis=1))
    if cfg.pn_stats:
        bn_stage("object_encoder.mlp_pointnet.0", "pn_only", np.asarray(inp["pn"], np.float64))
    feat = (-1, "E")
    if cfg.n_feat > 1:
        bn_stage("object_encoder.mlp_merge.0", "merge", get((-1, "E")))
        feat = (-1, "merge.out")
    out[(-1, "D0")], out[(-1, "nrm0")] = _layer(TB.rownorm_fwd, (get(feat),), dtype)
    obj, hint = (-1, "D0"), None
    hints = np.asarray(inp["hints"], np.float64).reshape(cfg.P * cfg.H, D)
    for li, (pre, is_obj, site) in enumerate(cfg.layers):
        Tq, Tk = cfg.t(li)
        M = cfg.P * Tq
        x = get(obj) if is_obj else (hints if hint is None else get(hint))
        mem = (hints if hint is None else get(hint)) if is_obj else get(obj)
        w = lambda s: _w(sd, pre + "." + s)
        s4, s5 = (site + 5, site + 4) if mut == "site_45" else (site + 4, site + 5)
        out[(li, "qkv")] = _prod(x, w("self_attn.in_proj_weight"), w("self_attn.in_proj_bias"), dtype)
        qkv = get((li, "qkv"))
        f0 = attn_factor(seed, site, p, cfg.P, Tq, Tq)
        r, _ = xattn_fwd_ref(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], cfg.P, Tq, Tq, f0)
        if dtype is not np.float64:
            P32, O32, _ = xattn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], cfg.P, Tq, Tq, f0, dtype)
            r = {"P": (P32.astype(np.float64), r["P"][1]), "O": (O32.astype(np.float64), r["O"][1])}
        out[(li, "Ps")], out[(li, "os")] = r["P"], r["O"]
        out[(li, "x1")], out[(li, "xh1")], out[(li, "r1")] = _layer(_proj_ln, (
            x, get((li, "os")), w("self_attn.out_proj.weight"), w("self_attn.out_proj.bias"), w("norm1.weight"), w("norm1.bias"),
            TB.drop_factor(seed, site + 1, p, (M, D))), dtype)
        cw, cb = w("multihead_attn.in_proj_weight"), w("multihead_attn.in_proj_bias")
        out[(li, "q2")] = _prod(get((li, "x1")), cw[:D], cb[:D], dtype)
        out[(li, "kv2")] = _prod(mem, cw[:2 * D], cb[:2 * D], dtype) if mut == "kv_slice" else _prod(mem, cw[D:], cb[D:], dtype)
        q2, kv2 = get((li, "q2")), get((li, "kv2"))
        f2 = attn_factor(seed, site + 2, p, cfg.P, Tq, Tk)
        r, _ = xattn_fwd_ref(q2, kv2[:, :D], kv2[:, D:], cfg.P, Tq, Tk, f2)
        if dtype is not np.float64:
            P32, O32, _ = xattn_fwd(q2, kv2[:, :D], kv2[:, D:], cfg.P, Tq, Tk, f2, dtype)
            r = {"P": (P32.astype(np.float64), r["P"][1]), "O": (O32.astype(np.float64), r["O"][1])}
        out[(li, "Pc")], out[(li, "oc")] = r["P"], r["O"]
        out[(li, "x2")], out[(li, "xh2")], out[(li, "r2")] = _layer(_proj_ln, (
            get((li, "x1")), get((li, "oc")), w("multihead_attn.out_proj.weight"), w("multihead_attn.out_proj.bias"), w("norm2.weight"),
            w("norm2.bias"), TB.drop_factor(seed, site + 3, p, (M, D))), dtype)
        out[(li, "h1")] = _prod(get((li, "x2")), w("linear1.weight"), w("linear1.bias"), dtype, relu=True)
        h1 = get((li, "h1"))
        # within 1 ulp of h1 * factor, the factor's scale being the float32 quotient 1.f / (1.f - p) that make_drop documents (the real
        # 1 / (1 - p) is 0.77 u away from it for p = 0.1f: a correct float32 kernel would sit up to 1.27 ulp from THAT product). One
        # float32 product: 1/2 ulp. Exact for p = 0: h1d IS h1.
        # (Chained, for the comparison with the twin, the factor is the real one like everywhere else.)
        f4 = TB.drop_factor(seed, s4, p, (M, FF))
        if saved is not None and p > 0:
            f4 = (f4 > 0) * float(F32(1.0) / (F32(1.0) - F32(p)))
        hd = h1 * f4
        out[(li, "h1d")] = ((h1.astype(F32) * f4.astype(F32)).astype(np.float64) if (dtype is not np.float64 and p > 0) else hd,
                            np.spacing(np.abs(hd).astype(F32)).astype(np.float64) * (p > 0))
        out[(li, "out")], out[(li, "xh3")], out[(li, "r3")] = _layer(_proj_ln, (
            get((li, "x2")), get((li, "h1d")), w("linear2.weight"), w("linear2.bias"), w("norm3.weight"), w("norm3.bias"),
            TB.drop_factor(seed, s5, p, (M, D))), dtype)
        if is_obj:
            obj = (li, "out")
        else:
            hint = (li, "out")
    last = get(hint).reshape(cfg.P, cfg.H, D)
    out[(-1, "pool")] = (last.max(axis=1), zero)  # no arithmetic: the kernel's own rows, exactly
    out[(-1, "arg")] = (TB.first_argmax(last), zero)
    out[(-1, "a1")] = _prod(get((-1, "pool")), _w(sd, "mlp_offsets.0.weight"), _w(sd, "mlp_offsets.0.bias"), dtype, relu=True)
    out[(-1, "offsets")] = _prod(get((-1, "a1")), _w(sd, "mlp_offsets.2.weight"), _w(sd, "mlp_offsets.2.bias"), dtype)
    return out


def dec_bwd_ref(sv, W, dout, dmem0, g0, seed, site, p, pairs, Tq, Tk, dtype=np.float64):
    """One decoder layer's backward from the saved tensors exactly as dec_bwd uses them. sv: {field: array} with the layer's saved
    fields plus 'x' and 'mem'; W: {DEC_PARAMS name: array}; g0: {name: the .grad contents before the call} (a missing name: frozen, no
    gradient returned). -> (dx, dmem, {name: grad}, inter) all in ``dtype``; inter: the operands of the last launches that the
    per-element bounds need (dq of the self-attention block, dkv of the cross-attention block)."""
    t = dtype
    a = lambda k: np.asarray(sv[k], np.float64).astype(t)
    w = lambda k: np.asarray(W[k], np.float64).astype(t)
    M = pairs * Tq
    fac = lambda s, shape: TB.drop_factor(seed, site + s, p, shape)
    grads = {}

    def add(name, val, rows=None):
        if name not in g0:
            return
        if name not in grads:
            grads[name] = np.asarray(g0[name], np.float64).astype(t).copy()
        if rows is None:
            grads[name] += val
        else:
            grads[name][rows] += val

    def ln(dY, xh, r, n, s):
        add(f"{n}.weight", (dY * a(xh)).sum(axis=0, dtype=t))
        add(f"{n}.bias", dY.sum(axis=0, dtype=t))
        return TB.ln_bwd(dY, sv[xh], sv[r], W[f"{n}.weight"], fac(s, (M, D)), t)

    def lin(name, dY, X, rows=None):
        add(name + "weight", dY.T @ X, rows)
        add(name + "bias", dY.sum(axis=0, dtype=t), rows)

    dx2, ds = ln(np.asarray(dout, np.float64).astype(t), "xh3", "r3", "norm3", 5)
    lin("linear2.", ds, a("h1d"))
    dh = ds @ w("linear2.weight")
    dh = np.where(a("h1") > 0, dh * fac(4, (M, FF)).astype(t), t(0.0))
    lin("linear1.", dh, a("x2"))
    dx2 = dx2 + dh @ w("linear1.weight")
    dx1, ds = ln(dx2, "xh2", "r2", "norm2", 3)
    lin("multihead_attn.out_proj.", ds, a("oc"))
    dob = ds @ w("multihead_attn.out_proj.weight")
    kv2 = np.asarray(sv["kv2"], np.float64)
    dq, dk, dv = xattn_bwd(sv["q2"], kv2[:, :D], kv2[:, D:], sv["Pc"], dob, pairs, Tq, Tk, attn_factor(seed, site + 2, p, pairs, Tq, Tk), t)
    cw = w("multihead_attn.in_proj_weight")
    lin("multihead_attn.in_proj_", dq, a("x1"), slice(0, D))
    dx1 = dx1 + dq @ cw[:D]
    dkv = np.concatenate([dk, dv], axis=1)
    lin("multihead_attn.in_proj_", dkv, a("mem"), slice(D, 3 * D))
    dmem = np.asarray(dmem0, np.float64).astype(t) + dkv @ cw[D:]
    dx, ds = ln(dx1, "xh1", "r1", "norm1", 1)
    lin("self_attn.out_proj.", ds, a("os"))
    dob = ds @ w("self_attn.out_proj.weight")
    qkv = np.asarray(sv["qkv"], np.float64)
    d3 = xattn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["Ps"], dob, pairs, Tq, Tq, attn_factor(seed, site, p, pairs, Tq, Tq), t)
    dqkv = np.concatenate(d3, axis=1)
    lin("self_attn.in_proj_", dqkv, a("x"))
    dx = dx + dqkv @ w("self_attn.in_proj_weight")
    return dx, dmem, grads, {"dqkv": dqkv, "dkv": dkv, "dq2": dq}


def dec_bwd_bounds(sv, W, dout, dmem0, g0, seed, site, p, pairs, Tq, Tk):
    """{name: (ref, tol)} for 'dx', 'dmem' and every gradient of g0 under the layer rule per tensor; PLUS {name + '/el': (ref, tol)}
    per element for self_attn.in_proj_weight, self_attn.in_proj_bias and multihead_attn.in_proj_bias: the product bound of their LAST
    launch (lin_dw over the rows of dqkv / dq, dkv; K = the row count) on the reference's own operand, plus what the layer rule allows
    that operand (its scalar tolerance through |X|'s column sums, resp. the row count) — so an element that is small beside its
    tensor's maximum (the key part of an in-projection bias, whose true gradient is 0) is held at ITS size."""
    args = (sv, W, dout, dmem0, g0, seed, site, p, pairs, Tq, Tk)
    r64, r32 = dec_bwd_ref(*args, np.float64), dec_bwd_ref(*args, F32)

    def rule(a, b):
        e32 = float(np.abs(a - b.astype(np.float64)).max())
        return max(16.0 * e32, 8.0 * U * float(np.abs(a).max()))

    out = {"dx": (r64[0], rule(r64[0], r32[0])), "dmem": (r64[1], rule(r64[1], r32[1]))}
    for n, g in r64[2].items():
        out[n] = (g, rule(g, r32[2][n]))
    it = {k: rule(r64[3][k], r32[3][k]) for k in r64[3]}
    x, mem, x1 = (np.asarray(sv[k], np.float64) for k in ("x", "mem", "x1"))
    dqkv, dkv, dq2 = r64[3]["dqkv"], r64[3]["dkv"], r64[3]["dq2"]
    n = "self_attn.in_proj_weight"
    if n in g0:
        ref, tol = TB.linear(dqkv.T, x, EX, C0=np.asarray(g0[n], np.float64))
        out[n + "/el"] = (ref, tol + it["dqkv"] * np.abs(x).sum(axis=0)[None, :])
    n = "self_attn.in_proj_bias"
    if n in g0:
        ref, tol = TB.colsum(dqkv, np.asarray(g0[n], np.float64))
        out[n + "/el"] = (ref, tol + it["dqkv"] * dqkv.shape[0])
    n = "multihead_attn.in_proj_bias"
    if n in g0:
        b0 = np.asarray(g0[n], np.float64)
        rq, tq = TB.colsum(dq2, b0[:D])
        rk, tk = TB.colsum(dkv, b0[D:])
        out[n + "/el"] = (np.concatenate([rq, rk]), np.concatenate([tq + it["dq2"] * dq2.shape[0], tk + it["dkv"] * dkv.shape[0]]))
    return out


def layer_args(cfg, sd, inp, saved, li, p, seed, frozen=()):
    """the arguments of dec_bwd_ref / dec_bwd_bounds for cascade layer li from a dict of saved tensors: x and mem as the cascade wires
    them, non-zero dout, dmem and gradient contents (``frozen``: DEC_PARAMS names without a gradient)"""
    pre, is_obj, site = cfg.layers[li]
    Tq, Tk = cfg.t(li)
    hints = np.asarray(inp["hints"], np.float64).reshape(-1, D)
    prev = lambda obj: next((saved[(j, "out")] for j in reversed(range(li)) if cfg.layers[j][1] == obj), saved[(-1, "D0")] if obj else hints)
    sv = {f: saved[(li, f)] for f in DEC_FIELDS}
    sv["x"], sv["mem"] = prev(is_obj), prev(not is_obj)
    W = {n: _w(sd, f"{pre}.{n}") for n in DEC_PARAMS}
    g0 = {n: gauss((SEED, 9, li, i), *W[n].shape) for i, n in enumerate(DEC_PARAMS) if n not in frozen}
    return sv, W, gauss((SEED, 8, li), cfg.P * Tq, D), gauss((SEED, 7, li), cfg.P * Tk, D), g0, seed, site, p, cfg.P, Tq, Tk


def step_ref(cfg, sd, inp, seed, p):
    """The whole step in float64 from the stage references chained: (offsets, {parameter: gradient}, grad_hint, running buffers)."""
    fw = forward_chain(cfg, sd, inp, seed, p)
    v = lambda layer, f: fw[(layer, f)][0]
    P, H, M0 = cfg.P, cfg.H, cfg.P * OBJ
    g = {}

    def lin_b(pre, dY, X):
        g[pre + "weight"] = g.get(pre + "weight", 0.0) + dY.T @ X
        g[pre + "bias"] = g.get(pre + "bias", 0.0) + dY.sum(axis=0)

    gout = np.asarray(inp["gout"], np.float64)
    lin_b("mlp_offsets.2.", gout, v(-1, "a1"))
    da1 = np.where(v(-1, "a1") > 0, gout @ _w(sd, "mlp_offsets.2.weight"), 0.0)
    lin_b("mlp_offsets.0.", da1, v(-1, "pool"))
    dpool = da1 @ _w(sd, "mlp_offsets.0.weight")
    (g1,) = TB.seq_max_bwd(dpool, v(-1, "arg"), H, np.float64)
    g1 = g1.reshape(P * H, D)
    g0 = np.zeros((M0, D))
    hints = np.asarray(inp["hints"], np.float64).reshape(P * H, D)
    ins = []  # (x, mem) of every layer, as forward_chain wired them
    obj, hint = v(-1, "D0"), hints
    for li, (pre, is_obj, site) in enumerate(cfg.layers):
        ins.append((obj, hint) if is_obj else (hint, obj))
        if is_obj:
            obj = v(li, "out")
        else:
            hint = v(li, "out")
    for li in reversed(range(len(cfg.layers))):
        pre, is_obj, site = cfg.layers[li]
        Tq, Tk = cfg.t(li)
        sv = {f: v(li, f) for f in DEC_FIELDS}
        sv["x"], sv["mem"] = ins[li]
        W = {n: _w(sd, f"{pre}.{n}") for n in DEC_PARAMS}
        zeros = {n: np.zeros_like(W[n]) for n in DEC_PARAMS}
        dx, dmem, grads, _ = dec_bwd_ref(sv, W, g0 if is_obj else g1, g1 if is_obj else g0, zeros, seed, site, p, P, Tq, Tk)
        g0, g1 = (dx, dmem) if is_obj else (dmem, dx)
        for n, val in grads.items():
            g[f"{pre}.{n}"] = val
    # ObjectEncoder
    feat = v(-1, "merge.out") if cfg.n_feat > 1 else v(-1, "E")
    (dfeat,) = TB.rownorm_bwd(g0, v(-1, "D0"), v(-1, "nrm0"), np.float64)

    def bn_b(pre, key, dout, x):
        r = bn_bwd(dout, v(-1, key + ".out"), v(-1, key + ".xhat"), v(-1, key + ".rstd"), _w(sd, pre + ".1.weight"), np.zeros(dout.shape[1]),
                   np.zeros(dout.shape[1]))
        g[pre + ".1.weight"], g[pre + ".1.bias"] = r["dg"], r["db"]
        lin_b(pre + ".0.", r["dy"], x)
        return r["dy"] @ _w(sd, pre + ".0.weight")

    dE = bn_b("object_encoder.mlp_merge.0", "merge", dfeat, v(-1, "E")) if cfg.n_feat > 1 else dfeat
    del feat
    for col, f in enumerate(cfg.use):
        kind, pre, src, sizes = branch_plan(cfg, f)
        sl = slice(col * D, (col + 1) * D)
        if kind == "embed":
            (draw,) = TB.rownorm_bwd(dE[:, sl], v(-1, "E")[:, sl], v(-1, f + ".nrm"), np.float64)
            g[pre] = scatter_ref(draw, np.asarray(inp[src]), np.zeros_like(_w(sd, pre)))[0]
            continue
        (d,) = TB.rownorm_bwd(dE[:, sl], v(-1, "E")[:, sl], v(-1, f + ".nrm"), np.float64)
        for li in reversed(range(len(sizes))):
            if li > 0:
                x = v(-1, f"{f}.{li - 1}.out")
            else:
                x = np.asarray(inp[src], np.float64).reshape(M0, -1)
                if f == "num":
                    x = ((x[:, 0].astype(F32) - F32(NUM_MEAN)) / F32(NUM_STD)).astype(np.float64).reshape(M0, 1)
            d = bn_b(f"{pre}.{li}", f"{f}.{li}", d, x)
    run = {k[1][4:]: val[0] for k, val in fw.items() if k[0] == -1 and k[1].startswith("run:")}
    return v(-1, "offsets"), g, g1.reshape(P, H, D), run


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library (text2loc_amd/csrc/fine_train_blocks.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def load_blocks():
    """the blocks library with the whole C ABI declared (engine.load_library) and the wrappers of this tier"""
    import ctypes as Ct

    from tests.fine_blocks import blocks_path
    from text2loc_amd import engine

    lib = engine.load_library(blocks_path())  # T2LError if it was not built: there is no fallback
    p, i, l, u, f = Ct.c_void_p, Ct.c_int, Ct.c_int64, Ct.c_uint32, Ct.c_float
    sigs = {
        "t2l_blk_ft_lin_fwd": [p, l, i, i, p, l, p, i, p, l, i],
        "t2l_blk_ft_lin_dx": [p, l, i, i, p, l, i, p, l, i],
        "t2l_blk_ft_lin_dw": [p, l, p, l, i, i, i, p, l, p],
        "t2l_blk_ft_bn_fwd": [p, i, i, p, p, p, p, p, p],
        "t2l_blk_ft_bn_bwd": [p, p, p, p, p, i, i, p, p, p],
        "t2l_blk_ft_attn_fwd": [p, l, p, l, p, l, i, i, i, p, p, l, u, i, f],
        "t2l_blk_ft_attn_bwd": [p, l, p, l, p, l, p, p, l, p, l, p, l, p, l, i, i, i, u, i, f],
        "t2l_blk_ft_gather": [p, i, p, i, p],
        "t2l_blk_ft_scatter_add": [p, i, p, i, p],
        "t2l_blk_ft_num_in": [p, i, p],
        "t2l_blk_ft_saved": [p, i, Ct.c_char_p, p, l, Ct.POINTER(l)],
        "t2l_blk_ft_dec_bwd": [p, i, p, p, p],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i, args
    lib.t2l_blk_last_error.restype, lib.t2l_blk_last_error.argtypes = Ct.c_char_p, []
    return lib
