"""TEST INFRASTRUCTURE — float64 references, derived tolerances and the case lists of the training-block tier
(tests/test_train_blocks_cpu.py, tests/test_gpu_train_blocks.py).

Every block of the training steps — a product of gemm_f32.h with its epilogue, attention, LayerNorm, F.normalize of a row, element-wise
dropout, pool + normalise, seq-max — is a continuous function of its inputs or takes its mask / arg-max as an input, so it has an exact float64 reference and an element-wise
bound. numpy only; the arithmetic comes from ``oracle.arith`` and ``oracle.t2l_oracle_train.dropout_keep``, never from the product.

Products.  ``ref = arith.product(A, B, arithmetic) (+ bias) (+ C0)`` then the epilogue; per element

    tol = factor * (K + 8) * 2^-24 * (|A| @ |B| + |bias| + |C0|),   factor = 2

the first-order bound of ANY summation order with one float32 rounding per step over the full reduction length K (the 8: the four-way
partial sum, the bias add, the split-z atomics; the 2: second order). The same form bounds colsum / db and dgamma / dbeta with the
row count for K. ReLU and the 0/1 masks are 1-Lipschitz, the dropout scale multiplies value and bound alike.

Layer kernels.  Per output tensor ``tol = max(16 * e32, 8 * 2^-24 * max|ref|)`` with e32 the largest error of the SAME function run
in float32 numpy against its float64 run (every function below takes the dtype): measured on the reference side only. 16: the device
sums sequentially and through atomics where numpy sums pairwise.
"""
import functools
import itertools

import numpy as np

from oracle import arith
from oracle.t2l_oracle_train import dropout_keep

U = 2.0 ** -24
FACTOR = {arith.EXACT: 2.0, arith.BF16: 2.0, arith.SPLIT: 2.0}  # per arithmetic (profiles/train_blocks.md: measured worst err / tol)
ARITHS = (arith.EXACT, arith.BF16, arith.SPLIT)
P_DROP = float(np.float32(0.1))  # the float32 the wrappers receive
LN_EPS = float(np.float32(1e-5))
NORM_EPS = float(np.float32(1e-12))
# One seed for every tensor of the tier. A dropped reduction index is invisible to ANY bound where its operand happens to be ~0, and the
# one-row cases (M = 1) have a single operand value per index: the CPU tier's dropped-index control therefore holds for a seed whose
# edge operands are not that small (with 20240607, x[0, 0] of the M = 1, (768, 256) case is -1.6e-3 and its products stay inside the
# bound). Nothing else depends on the choice.
SEED = 7

# rows M (the reduction length of gemm_tn): 257 -> a split of 2 whose second chunk is 65 rows, 600 -> a split of 3
ROWS = (1, 31, 32, 33, 63, 64, 65, 140, 257, 600)
# (N, Kp): 32-blocks even with the block option on | 64-blocks | square | the QKV product
WIDTHS = ((32, 96), (64, 128), (256, 256), (768, 256))
# the multi-job kernels: the small branches' second Linear (64 -> 256), and the narrowest legal shape
MULTI_WIDTHS = ((256, 64), (32, 96))


def gauss(seed, *shape):
    """float64 array of exact float32 Gaussian values."""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32).astype(np.float64)


def drop_factor(seed, site, p, shape, transposed=False):
    """The factor the dropout site multiplies a [rows, ld] tensor with: keep / (1 - p) at element index row * ld + col
    (``transposed``: the WRONG index col * ld + row, a negative control)."""
    if p <= 0.0:
        return np.ones(shape)
    rows, ld = int(np.prod(shape[:-1])), shape[-1]
    keep = dropout_keep(seed, site, rows * ld, p)
    if transposed:
        r, c = np.meshgrid(np.arange(rows), np.arange(ld), indexing="ij")
        keep = dropout_keep(seed, site, ld * ld + rows, p)[(c * ld + r).ravel()]
    return (keep / (1.0 - p)).reshape(shape)


def tn_split(M, N, Kp, blk):
    """train.hip: tn_split — (ksplit, kchunk) of the dW product's reduction over M rows. Used by the negative controls only (which
    index opens the last z-chunk); no reference depends on it."""
    tiles = (N // blk) * (Kp // blk)
    ksplit = max(1, min((M + 255) // 256, (1024 + tiles - 1) // tiles))
    kchunk = (((M + ksplit - 1) // ksplit) + 63) & ~63
    return (M + kchunk - 1) // kchunk, kchunk


# ---------------------------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------------------------
def linear(A, B, ar, bias=None, C0=None, relu=False, base=None):
    """(ref, tol) of C = A @ B (+ bias) (+ C0) (relu) under arithmetic ``ar``; A [M, K], B [K, N]. ``base``: a cached
    (arith.product(A, B, ar), |A| @ |B|)."""
    prod, mag = base if base is not None else (arith.product(A, B, ar), np.abs(A) @ np.abs(B))
    ref, mag = prod.copy(), mag.copy()
    if bias is not None:
        ref += bias
        mag += np.abs(bias)
    if C0 is not None:
        ref += C0
        mag += np.abs(C0)
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, FACTOR[ar] * (A.shape[1] + 8) * U * mag


def colsum(X, c0):
    """(ref, tol) of c0 + the column sums of X [rows, n] (db, dbeta; always a float32 sum of the unrounded values)."""
    return c0 + X.sum(axis=0), FACTOR[arith.EXACT] * (X.shape[0] + 8) * U * (np.abs(X).sum(axis=0) + np.abs(c0))


def masked_dropped(ref, tol, factor, mask_src=None):
    """The epi == 2 epilogue (mask_src > 0, then the dropout factor) or, without mask_src, the C2 of epi == 1."""
    if mask_src is not None:
        keep = mask_src > 0
        ref, tol = np.where(keep, ref, 0.0), np.where(keep, tol, 0.0)
    return ref * factor, tol * factor


def f32_matmul(A, B, ar):
    """float32 numpy.matmul of the modelled operands (what a correct float32-accumulating kernel may return), as float64."""
    f = lambda x: x.astype(np.float32)
    if ar == arith.EXACT:
        out = f(A) @ f(B)
    elif ar == arith.BF16:
        out = f(arith.bf16_rne(A)) @ f(arith.bf16_rne(B))
    else:
        (ah, al), (bh, bl) = arith.split_bf16(A), arith.split_bf16(B)
        out = f(ah) @ f(bh) + f(ah) @ f(bl) + f(al) @ f(bh)
    return out.astype(np.float64)


class ProductCase:
    """The operands of one (launcher kind, M, N, Kp): float64 arrays of exact float32 values, from a fixed seed.
    kind nt: Y[M,N] = X[M,Kp] W[N,Kp]^T + b        nn: dX[M,Kp] (+)= dY[M,N] W[N,Kp]        tn: dW[N,Kp] += dY[M,N]^T X[M,Kp], db += colsum dY
    (tn_nn is tn and nn from one launch.) A, B, K: the product as ``linear`` takes it."""

    def __init__(self, kind, M, N, Kp, job=0):
        self.kind, self.M, self.N, self.Kp = kind, M, N, Kp
        seed = (SEED, {"nt": 1, "nn": 2, "tn": 3}[kind], M, N, Kp, job)
        dy_seed = (SEED, 0, M, N, Kp, job)  # nn and tn share their dY: gemm_tn_nn computes both from one
        if kind == "nt":
            self.X, self.W, self.b = gauss(seed + (0,), M, Kp), gauss(seed + (1,), N, Kp), gauss(seed + (2,), N)
            self.A, self.B = self.X, self.W.T
        elif kind == "nn":
            self.dY, self.W, self.C0 = gauss(dy_seed, M, N), gauss(seed + (1,), N, Kp), gauss(seed + (2,), M, Kp)
            self.mask_src = gauss(seed + (3,), M, Kp)
            self.A, self.B = self.dY, self.W
        else:
            self.dY, self.X = gauss(dy_seed, M, N), gauss(seed + (1,), M, Kp)
            self.C0, self.db0 = gauss(seed + (2,), N, Kp), gauss(seed + (3,), N)
            self.A, self.B = self.dY.T, self.X
        self.K = self.A.shape[1]
        self._base = {}

    def base(self, ar):
        if ar not in self._base:
            self._base[ar] = (arith.product(self.A, self.B, ar), np.abs(self.A) @ np.abs(self.B))
        return self._base[ar]


@functools.lru_cache(maxsize=8)
def product_case(kind, M, N, Kp, job=0):
    return ProductCase(kind, M, N, Kp, job)


def nt_variants():
    """(bias, relu, epi, p) of the gemm_nt cases."""
    plain = [(bias, relu, 0, 0.0) for bias, relu in itertools.product((False, True), (False, True))]
    return plain + [(True, True, 1, 0.0), (True, True, 1, P_DROP)]


def tn_nn_variants():
    """(mask, accumulate, p) of the gemm_tn_nn cases: the two ways the step calls it (linear1: accumulate, no mask; linear2: mask)."""
    return [(False, 1, 0.0), (False, 0, P_DROP), (True, 0, 0.0), (True, 0, P_DROP)]


def nt_reference(c, ar, bias, relu, epi, p, site=2):
    """{name: (ref, tol)} of a gemm_nt case."""
    ref, tol = linear(c.A, c.B, ar, bias=c.b if bias else None, relu=relu, base=c.base(ar))
    out = {"Y": (ref, tol)}
    if epi == 1:
        out["Y2"] = masked_dropped(ref, tol, drop_factor(SEED, site, p, ref.shape))
    return out


def nn_reference(c, ar, accumulate, mask=False, p=0.0, site=2):
    ref, tol = linear(c.A, c.B, ar, C0=c.C0 if accumulate else None, base=c.base(ar))
    if mask:
        ref, tol = masked_dropped(ref, tol, drop_factor(SEED, site, p, ref.shape), c.mask_src)
    return {"dX": (ref, tol)}


def tn_reference(c, ar):
    return {"dW": linear(c.A, c.B, ar, C0=c.C0, base=c.base(ar)), "db": colsum(c.dY, c.db0)}


# ---------------------------------------------------------------------------------------------------------------------------
# layer kernels: every function runs in the dtype it is given (float64 = the reference, float32 = the restatement behind e32)
# ---------------------------------------------------------------------------------------------------------------------------
def layer_tol(fn, *args):
    """[(ref, tol)] per output of ``fn(*args, dtype)``: tol = max(16 e32, 8 * 2^-24 * max|ref|), a scalar per tensor."""
    ref, r32 = fn(*args, np.float64), fn(*args, np.float32)
    out = []
    for a, b in zip(ref, r32):
        e32 = float(np.abs(a - b.astype(np.float64)).max()) if a.size else 0.0
        out.append((a, max(16.0 * e32, 8.0 * U * float(np.abs(a).max()))))
    return out


def attn_fwd(qkv, B, S, HD, factor, dtype):
    """qkv [B S, 12 HD], factor [B, 4, S, S] (dropout on the probabilities) -> (P [B, 4, S, S], O [B S, 4 HD])"""
    x = qkv.astype(dtype).reshape(B, S, 3, 4, HD)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))  # [B, 4, S, HD]
    s = (q @ k.transpose(0, 1, 3, 2)) * dtype(1.0 / np.sqrt(dtype(HD)))
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    P = e / e.sum(axis=-1, keepdims=True)
    O = (P * factor.astype(dtype)) @ v
    return P, O.transpose(0, 2, 1, 3).reshape(B * S, 4 * HD)


def attn_bwd(qkv, P, dO, B, S, HD, factor, dtype):
    """-> (dqkv [B S, 12 HD],)"""
    x = qkv.astype(dtype).reshape(B, S, 3, 4, HD)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    P, m = P.astype(dtype), factor.astype(dtype)
    go = dO.astype(dtype).reshape(B, S, 4, HD).transpose(0, 2, 1, 3)
    dV = (P * m).transpose(0, 1, 3, 2) @ go
    dP = m * (go @ v.transpose(0, 1, 3, 2))
    t = (dP * P).sum(axis=-1, keepdims=True)
    dS = P * (dP - t) * dtype(1.0 / np.sqrt(dtype(HD)))
    dQ, dK = dS @ k, dS.transpose(0, 1, 3, 2) @ q
    d = np.stack([dQ, dK, dV], axis=0).transpose(1, 3, 0, 2, 4)  # [B, S, 3, 4, HD]
    return (d.reshape(B * S, 12 * HD),)


def ln_fwd(x, y, gamma, beta, factor, dtype):
    """-> (out, xhat, rstd) of LayerNorm(x + y * factor)"""
    a = x.astype(dtype) + y.astype(dtype) * factor.astype(dtype)
    a = a - a.mean(axis=1, keepdims=True, dtype=dtype)
    rstd = 1.0 / np.sqrt((a * a).mean(axis=1, keepdims=True, dtype=dtype) + dtype(LN_EPS))
    xhat = a * rstd
    return xhat * gamma.astype(dtype) + beta.astype(dtype), xhat, rstd[:, 0]


def ln_bwd(dout, xhat, rstd, gamma, factor, dtype):
    """-> (d_res, d_y); dgamma / dbeta are sums over the rows and bounded by ``ln_param_grads``"""
    d, h = dout.astype(dtype), xhat.astype(dtype)
    dh = d * gamma.astype(dtype)
    m1, m2 = dh.mean(axis=1, keepdims=True, dtype=dtype), (dh * h).mean(axis=1, keepdims=True, dtype=dtype)
    dz = rstd.astype(dtype)[:, None] * (dh - m1 - h * m2)
    return dz, dz * factor.astype(dtype)


def ln_param_grads(dout, xhat, dg0, db0):
    """{name: (ref, tol)} of dgamma = dg0 + sum_t dout * xhat, dbeta = db0 + sum_t dout (the products' bound, rows for K)."""
    return {"dgamma": colsum(dout * xhat, dg0), "dbeta": colsum(dout, db0)}


def rownorm_fwd(x, dtype):
    """x [M, D] -> (y, n): F.normalize(x, dim=-1) and the norm it divides by (clamped at 1e-12)"""
    x = x.astype(dtype)
    n = np.maximum(np.sqrt((x * x).sum(axis=1, dtype=dtype)), dtype(NORM_EPS))
    return x / n[:, None], n


def rownorm_bwd(dy, y, n, dtype):
    """-> (dx [M, D],): (dy - y (dy . y)) / n, and dy / 1e-12 for a row whose norm sits at the clamp"""
    dy, y, n = dy.astype(dtype), y.astype(dtype), n.astype(dtype)[:, None]
    t = (dy * y).sum(axis=1, keepdims=True, dtype=dtype)
    return (np.where(n <= dtype(NORM_EPS), dy / dtype(NORM_EPS), (dy - y * t) / n),)


def drop_reference(h, factor, d=None):
    """(ref, tol) of drop_fwd — hd = h * factor — or, with d, of relu_drop_bwd — d * factor where h > 0, else 0. ``layer_tol``'s bound
    on the elements that are kept; 0 (the value must be the reference's exactly) on the dropped and the masked ones."""
    live = factor > 0 if d is None else (factor > 0) & (h > 0)

    def fn(v, dtype):
        return (np.where(live, v.astype(dtype) * factor.astype(dtype), dtype(0.0)),)

    ((ref, tol),) = layer_tol(fn, h if d is None else d)
    return ref, np.where(live, tol, 0.0)


def pool_norm_fwd(X, dtype):
    """X [B, 28, 256] -> (out [B, 256], save_n [B]); the arg-max is ``first_argmax(X)`` (exact: no arithmetic before the comparison)"""
    mx = X.astype(dtype).max(axis=1)
    n = np.maximum(np.sqrt((mx * mx).sum(axis=1, dtype=dtype)), dtype(NORM_EPS))
    return mx / n[:, None], n


def pool_norm_bwd(g, y, arg, n, S, dtype):
    """-> (dX [B, S, 256],)"""
    g, y, n = g.astype(dtype), y.astype(dtype), n.astype(dtype)[:, None]
    d = (g - y * (g * y).sum(axis=1, keepdims=True, dtype=dtype)) / n
    return (np.where(np.arange(S)[None, :, None] == arg[:, None, :], d[:, None, :], dtype(0.0)),)


def first_argmax(X):
    """[B, S, D] -> int32 [B, D], the first maximal row (numpy's argmax rule, torch.max's, the kernels')."""
    return X.argmax(axis=1).astype(np.int32)


def seq_values(X, R):
    """What seq_max compares: X, or float32(X + R) — ONE float32 addition per element, which is part of the operation's definition
    (so the arg-max of the reference is the kernel's, exactly)."""
    return X if R is None else (X.astype(np.float32) + R.astype(np.float32)).astype(np.float64)


def seq_max_fwd(V, dtype):
    return (V.astype(dtype).max(axis=1),)


def seq_max_bwd(g, arg, S, dtype):
    return (np.where(np.arange(S)[None, :, None] == arg[:, None, :], g.astype(dtype)[:, None, :], dtype(0.0)),)


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library (text2loc_amd/csrc/train_blocks.hip): loaded by path, beside libt2l.so; nothing of the Python package is imported
# ---------------------------------------------------------------------------------------------------------------------------
def load_blocks():
    import ctypes as C
    import os.path as osp

    path = osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "text2loc_amd", "libt2l_blocks.so")
    lib = C.CDLL(path)  # OSError if it was not built: there is no fallback
    p, i, u, f = C.c_void_p, C.c_int, C.c_uint32, C.c_float
    sigs = {
        "t2l_blk_gemm_nt": [p, p, p, p, p, i, i, i, i, i, i, i, u, i, f],
        "t2l_blk_gemm_nn": [p, p, p, i, i, i, i, i, i],
        "t2l_blk_gemm_tn": [p, p, p, p, i, i, i, i, i],
        "t2l_blk_gemm_tn_nn": [p, p, p, p, p, p, i, i, i, i, p, i, i, u, i, f],
        "t2l_blk_gemm_nt_multi": [i, p, p, p, p, i, i, i, i],
        "t2l_blk_gemm_tn_nn_multi": [i, p, p, p, p, p, p, i, i, i, i],
        "t2l_blk_attn_fwd": [p, p, p, i, i, i, u, i, f],
        "t2l_blk_attn_bwd": [p, p, p, p, i, i, i, u, i, f],
        "t2l_blk_ln_fwd": [p, p, i, i, p, p, p, p, p, u, i, f],
        "t2l_blk_ln_bwd": [p, p, p, i, i, i, p, p, p, p, p, u, i, f],
        "t2l_blk_rownorm_fwd": [p, i, i, p, i, p],
        "t2l_blk_rownorm_bwd": [p, p, i, p, i, i, p],
        "t2l_blk_drop_fwd": [p, C.c_int64, p, u, i, f],
        "t2l_blk_relu_drop_bwd": [p, p, C.c_int64, u, i, f],
        "t2l_blk_pool_norm_fwd": [p, p, p, p, p, i],
        "t2l_blk_pool_norm_bwd": [p, p, p, p, p, i],
        "t2l_blk_seq_max_fwd": [p, p, i, i, i, p, p],
        "t2l_blk_seq_max_bwd": [p, p, i, i, i, p],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    lib.t2l_blk_last_error.restype = C.c_char_p
    lib.t2l_blk_last_error.argtypes = []
    return lib
