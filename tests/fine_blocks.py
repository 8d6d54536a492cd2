"""TEST INFRASTRUCTURE — float64 references, derived tolerances and fixtures of the fine-match block tier
(tests/test_fine_blocks_cpu.py, tests/test_gpu_fine_blocks.py; profiles/fine_blocks.md).

``t2l_fine_match`` (csrc/fine.hip) is held one attention block and one decoder pass at a time through the dev library's wrappers
(csrc/fine_blocks.hip). Every stage reference below is fed the KERNEL'S OWN input of that stage (for the plane arms
float64(hi) + float64(lo)), so nothing compounds across calls. numpy only; of the product only ``synth`` (fixture weights) is used.

References (float64).  ``mha_core`` is multi-head attention, four heads of 32, scale 1/sqrt(32), with an optional visibility matrix;
``decoder_layer`` the post-norm ``nn.TransformerDecoderLayer`` (ReLU, width 512, LayerNorm eps 1e-5, two-pass variance);
``cross_match64`` the oracle's ``cross_match`` per pair without tiles. The TILED forms take 32-row tiles and the product's
``TileGroups``: the query of row i of tile x (group base + (i >> shift)) sees key j of tile mem when j's group is the same pair and
``(j & mask) < count``. Every sum of the value path runs as an explicit sequential loop, so a masked key (probability exactly 0) or a
row of another pair changes no bit: the tiled reference equals the per-pair one EXACTLY, which tests/test_fine_blocks_cpu.py asserts.

Tolerance (derived; nothing is fitted to a kernel's error).  u = 2^-24, c = 2 (second order). A product y = W a + b over K terms,
its input known within ea, with mag = |W||a| + |b|:

    e(y) = |W| ea + c [ (P (K + 8)) u mag + rel mag + floor (sum|a| + sum|W|) ]                (no BatchNorm is folded here: F = 0)

with (P, rel, floor) of the arm as in tests/pointnet_blocks.py (f32: 1, 0, 0; split: 3, 3 * 2^-22, 2^-25; f16: 1, 2^-10 + 2^-22,
2^-25). The "+ 8" covers the bias add, the residual adds and the MFMA's internal partial sums. A value stored to planes is split
once: + max(2^-22 |v|, 2^-25).

Attention.  q, k, v by the product bound (arm of the call). Logits s = (q . k) / sqrt(32) over K = 32: the errors of q and k
propagated, plus the product bound of the attention CORE's arm — the f32 MFMA for arm f32, the three-product split form for split
AND for plain f16 (fine.hip: "always the three-product form") —, one rounding for the scale and one for the subtraction of the
maximum. With delta the largest logit error among a query's visible keys, p' / p lies in [e^-2 delta, e^2 delta] whatever the shift:

    e(p) = p [ e^(2 delta) (1 + eta) - 1 ],   eta = 2 EPS_EXP + EPS_RCP + 20 u      (__expf on both sides of the quotient, the 17
                                                                                    additions of the sum, 1.f / sum, the product)

EPS_EXP is the relative error of ``__expf`` for arguments in [-LOGIT_RANGE, 0]; a key whose logit sits further below the maximum
adds the absolute EXP_TAIL instead. o = p v over the visible keys (K = 32 slots): e(p) |v| + p e(v) + the core arm's product bound.
A row that sees no key: exactly zero where the block writes it, exactly what the tile held where it does not (second-order terms of
all propagated errors are included as products of the bounds).

LayerNorm.  out = (y - mu) / sqrt(var + eps) * g + b. Its Jacobian has 2-norm <= max|g| / sigma, sigma = sqrt(var + eps), and sigma
is (1 / sqrt(D))-Lipschitz in y, so for an input within ey (float32 roundings of the mean — at most LN_DEPTH additions on any path —
and of y - mu counted as input error):

    e(out) = max|g| ||ey'||_2 / (sigma - ||ey'||_2 / sqrt(D))  +  c [ (LN_DEPTH / 2 + 4) u + EPS_RSQRT ] |out - b|  +  c u |out|

(never more than 2 sqrt(D - 1) |g|: a LayerNorm's output lies within sqrt(D - 1) |g| of b whatever its row holds — the propagated
part saturates there once the chained worst cases stop being small, which they do after a few passes).

EPS_EXP, EXP_TAIL, EPS_RCP and EPS_RSQRT cannot be derived from the code (``__expf``, ``1.f / sum``, ``1.0f / sqrtf``): they are
TWICE the worst error measured once on the MI355X through ``t2l_blk_fine_probe`` (profiles/fine_blocks.md has the measurement).

Max over the hints and ReLU are 1-Lipschitz: a pooled element's bound is the largest among its candidate rows. ``mlp_offsets`` is a
plain float32 product (arm f32, K = 128 and 64). The end-to-end bound of ``cross_match_bound`` chains all of the above through
3 n_layers decoder passes; it is loose by construction and is stated beside the 5e-5 bar in profiles/fine_blocks.md.
"""
import numpy as np

F32, F16 = np.float32, np.float16
U = 2.0 ** -24
C = 2.0
LN_EPS = 1e-5
LN_DEPTH = 16
D, HEADS, HD, FF = 128, 4, 32, 512
SCALE = 0.17677669529663687  # 1 / sqrt(32), the kernel's literal
ARMS = {  # (P, rel, floor)
    "f32": (1, 0.0, 0.0),
    "split": (3, 3 * 2.0 ** -22, 2.0 ** -25),
    "f16": (1, 2.0 ** -10 + 2.0 ** -22, 2.0 ** -25),
}
ARM_ID = {"f32": 0, "split": 1, "f16": 2}
GUARD = 64.0

# twice the worst error measured on the MI355X (t2l_blk_fine_probe, 2^20 samples each; profiles/fine_blocks.md)
LOGIT_RANGE = 16.0
EPS_EXP = 2 * 9.41e-7     # relative, __expf on [-16, 0]              (measured 9.401e-07)
EXP_TAIL = 2 * 1.01e-13   # absolute, __expf on [-2^17, -16]          (measured 1.002e-13)
EPS_RCP = 2 * 5.97e-8     # relative, 1.f / x on [1e-6, 1e6]          (measured 5.960e-08: correctly rounded)
EPS_RSQRT = 2 * 8.95e-8   # relative, 1.0f / sqrtf(x) on [1e-6, 1e6]  (measured 8.941e-08)
ETA = 2 * EPS_EXP + EPS_RCP + 20 * U

GA, GB = (4, 16, 32, 0), (4, 16, 32, 2)  # TileGroups {shift, count, rows, base} of the object tiles


def ghint(n_hints):
    return (3, int(n_hints), 32, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# planes: the split of mfma_h3.h in numpy (RNE f16 of v, then RNE f16 of the exact float32 remainder)
# ---------------------------------------------------------------------------------------------------------------------------
def split(v):
    v = np.asarray(v, dtype=F32)
    hi = v.astype(F16)
    lo = (v - hi.astype(F32)).astype(F16)
    return hi, lo


def join64(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64)


def store_err(v, e, planes):
    """a produced value is split once when it is stored to planes"""
    return np.maximum(2.0 ** -22 * (np.abs(v) + e), 2.0 ** -25) if planes else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# values: float64, every sum an explicit sequential loop (row- and mask-independent bits)
# ---------------------------------------------------------------------------------------------------------------------------
def mm(a, wt):
    """a [..., T, K] @ wt [K, N], added up in k order"""
    acc = np.zeros(a.shape[:-1] + (wt.shape[1],))
    for k in range(wt.shape[0]):
        acc = acc + a[..., k:k + 1] * wt[k]
    return acc


def linear(a, W, b):
    return mm(a, np.asarray(W, np.float64).T) + np.asarray(b, np.float64)


def visible(gx, gm, mut=None):
    """bool [32 queries of tile x, 32 keys of tile mem] — f_group_softmax's rule"""
    i, j = np.arange(32), np.arange(32)
    gi = gx[3] + (i >> gx[0]) - gm[3]
    own = (j >> gm[0])[None, :] == gi[:, None]
    if mut == "neighbour":
        own |= (j >> gm[0])[None, :] == (gi ^ 1)[:, None]
    within = (j & ((1 << gm[0]) - 1))
    ok = (within <= gm[1]) if mut == "mask_le" else (within < gm[1])
    return own & ok[None, :] & (j < gm[2])[None, :]


def head_scale(hd):
    """the kernels' literal of 1 / sqrt(head_dim) (fine.hip; encode.hip: planes_layer)"""
    return {32: SCALE, 64: 0.125}[hd]


def heads_core(q, k, v, vis=None, hd=HD):
    """(o [Tq, W], any [Tq], p [heads, Tq, Tk], z [heads, Tq, Tk]): softmax(q k^T / sqrt(hd)) v per head of ``hd`` features over the
    visible keys; W = q's width (128 and four heads of 32 in the fine match; tests/encode_blocks.py: 128 or 256, heads of 32 or 64)"""
    Tq, Tk = q.shape[0], k.shape[0]
    vis = np.ones((Tq, Tk), bool) if vis is None else vis
    anyk = vis.any(axis=1)
    o = np.zeros((Tq, q.shape[1]))
    ps, zs = [], []
    for h in range(q.shape[1] // hd):
        c = slice(h * hd, (h + 1) * hd)
        s = mm(q[:, c], k[:, c].T) * head_scale(hd)
        s = np.where(vis, s, -np.inf)
        m = np.where(anyk, s.max(axis=1, initial=-np.inf), 0.0)
        z = s - m[:, None]
        e = np.where(vis, np.exp(z), 0.0)
        tot = np.zeros(Tq)
        for j in range(Tk):
            tot = tot + e[:, j]
        p = e / np.where(anyk, tot, 1.0)[:, None]
        o[:, c] = mm(p, np.where(vis.any(axis=0)[:, None], v[:, c], 0.0))  # a key no query sees may hold anything finite
        ps.append(p)
        zs.append(z)
    return o, anyk, np.stack(ps), np.stack(zs)


def mha_core(xq, xk, W, b, vis=None, mut=None, hd=HD):
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    width = W.shape[1]  # (the module's D unless tests/encode_blocks.py calls)
    # the lo plane dropped from the activation operand of ONE product: the value projection's (drop_lo), the query projection's
    # (drop_lo_q), the key projection's (drop_lo_k)
    xq_q = split(xq)[0].astype(np.float64) if mut == "drop_lo_q" else xq
    xk_k = split(xk)[0].astype(np.float64) if mut == "drop_lo_k" else xk
    xk_v = split(xk)[0].astype(np.float64) if mut == "drop_lo" else xk
    q, k, v = (linear(xq_q, W[:width], b[:width]), linear(xk_k, W[width:2 * width], b[width:2 * width]),
               linear(xk_v, W[2 * width:], b[2 * width:]))
    o, anyk, p, z = heads_core(q, k, v, vis, hd)
    if mut == "head_cols":  # heads 1 and 2 change places
        assert width >= 3 * hd, "the mutant swaps the second and the third head"
        o = o.copy()
        o[:, hd:2 * hd], o[:, 2 * hd:3 * hd] = o[:, 2 * hd:3 * hd].copy(), o[:, hd:2 * hd].copy()
    return o, anyk, (q, k, v, p, z)


def layer_norm(y, g, b, mut=None):
    mu = y.mean(axis=-1, keepdims=True)
    d = y - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    if mut == "ln_onepass":  # E[x^2] - mu^2 in float32
        y32 = y.astype(F32)
        mu32 = y32.mean(axis=-1, keepdims=True, dtype=F32)
        var = ((y32 * y32).mean(axis=-1, keepdims=True, dtype=F32) - mu32 * mu32).astype(np.float64)
    return d / np.sqrt(var + LN_EPS) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def _get(sd, prefix):
    g = lambda k: np.asarray(sd[prefix + k], np.float64)
    return g


def decoder_layer(x, mem, sd, prefix):
    """per pair, no tiles: x [Tq, 128], mem [Tk, 128]"""
    g = _get(sd, prefix)
    a = mha_core(x, x, g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias"))[0]
    x = layer_norm(x + linear(a, g(".self_attn.out_proj.weight"), g(".self_attn.out_proj.bias")), g(".norm1.weight"), g(".norm1.bias"))
    a = mha_core(x, mem, g(".multihead_attn.in_proj_weight"), g(".multihead_attn.in_proj_bias"))[0]
    x = layer_norm(x + linear(a, g(".multihead_attn.out_proj.weight"), g(".multihead_attn.out_proj.bias")), g(".norm2.weight"), g(".norm2.bias"))
    h = np.maximum(linear(x, g(".linear1.weight"), g(".linear1.bias")), 0.0)
    return layer_norm(x + linear(h, g(".linear2.weight"), g(".linear2.bias")), g(".norm3.weight"), g(".norm3.bias"))


def mlp_offsets(pooled, sd):
    g = _get(sd, "mlp_offsets")
    return linear(np.maximum(linear(pooled, g(".0.weight"), g(".0.bias")), 0.0), g(".2.weight"), g(".2.bias"))


def cross_match64(obj_enc, hint_enc, sd, n_layers):
    """obj_enc [P, 16, 128], hint_enc [P, n_hints, 128] -> offsets float64 [P, 2]: the oracle's cross_match, pair by pair"""
    out = []
    for d0, d1 in zip(np.asarray(obj_enc, np.float64), np.asarray(hint_enc, np.float64)):
        if n_layers == 0:
            d1 = decoder_layer(d1, d0, sd, "cross_hints")
        for i in range(n_layers):
            d0 = decoder_layer(d0, d1, sd, f"cross_objects.{i}")
            d1 = decoder_layer(d1, d0, sd, f"cross_hints.{i}")
        out.append(mlp_offsets(d1.max(axis=0)[None, :], sd)[0])
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds: (value, error) pairs on 32-row tiles
# ---------------------------------------------------------------------------------------------------------------------------
def lin_b(a, ea, W, b, arm):
    """(y, ey) of y = W a + b on the rows of a, a known within ea"""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    P, rel, floor = ARMS[arm]
    K = W.shape[1]
    aW = np.abs(W)
    mag = np.abs(a) @ aW.T + np.abs(b)
    ey = ea @ aW.T + C * ((P * (K + 8) * U + rel) * mag + floor * (np.abs(a).sum(axis=1, keepdims=True) + aW.sum(axis=1)))
    return linear(a, W, b), ey


def attention_b(x, ex, mem, em, gx, gm, W, b, arm, mut=None, vis=None, hd=HD):
    """One attention block on tiles -> (o, eo, any): o, eo [32, W] BEFORE the store, any [32] = the query sees a key in mem.
    vis: the visibility matrix itself instead of the one the tile groups give (tests/encode_blocks.py; gx, gm are then unused);
    hd: the head size (the width is W's)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    width, heads, scale = W.shape[1], W.shape[1] // hd, head_scale(hd)
    core = "f32" if arm == "f32" else "split"
    Pc, relc, floorc = ARMS[core]
    vis = visible(gx, gm, mut) if vis is None else vis
    o, anyk, (q, k, v, p, z) = mha_core(x, mem, W, b, vis, mut, hd)
    _, eq = lin_b(x, ex, W[:width], b[:width], arm)
    _, ek = lin_b(mem, em, W[width:2 * width], b[width:2 * width], arm)
    _, ev = lin_b(mem, em, W[2 * width:], b[2 * width:], arm)
    eo = np.zeros((32, width))
    seen = vis.any(axis=0)
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        aq, ak, av = np.abs(q[:, c]), np.abs(k[:, c]), np.where(seen[:, None], np.abs(v[:, c]), 0.0)
        evh = np.where(seen[:, None], ev[:, c], 0.0)
        s_abs = scale * (aq @ ak.T)
        es = scale * (eq[:, c] @ ak.T + aq @ ek[:, c].T + eq[:, c] @ ek[:, c].T)
        es = es + C * ((Pc * (hd + 8) * U + relc) * s_abs + floorc * scale * (aq.sum(axis=1)[:, None] + ak.sum(axis=1)[None, :]))
        zh = np.where(vis, z[h], 0.0)
        es = es + C * U * (s_abs + np.abs(zh))  # the scale, the subtraction of the maximum
        delta = np.where(vis, es, 0.0).max(axis=1)
        rho = np.exp(np.minimum(2 * delta, 50.0)) * (1 + ETA) - 1
        ep = np.minimum(p[h] * rho[:, None] + np.where(vis & (zh < -LOGIT_RANGE), EXP_TAIL * (1 + ETA), 0.0), 1.0)  # (a probability)
        pv = p[h] @ av
        eo[:, c] = ep @ av + p[h] @ evh + ep @ evh
        eo[:, c] += C * ((Pc * (hd + 8) * U + relc) * pv + floorc * (p[h].sum(axis=1)[:, None] + (vis.astype(np.float64) @ av)))
    eo[~anyk] = 0.0
    return o, eo, anyk


def attention_tiles_b(x, ex, mems, gx, gms, W, b, arm, shared, init=None, mut=None):
    """The obuf tile after the product's attention call(s) over the mem tiles ``mems`` = [(mem, em), ...] with groups ``gms``:
    (o, eo) with the store's split included for the plane arms. Rows no pass writes: zero (one tile, or the f32 form, whose first
    call writes every row) or ``init`` (the shared plane form, which writes only rows that saw a key)."""
    planes = arm != "f32"
    o = np.zeros((32, D)) if (init is None or not (shared and planes)) else np.array(init, np.float64)
    eo = np.zeros((32, D))
    written = np.zeros(32, bool)
    for n, ((mem, em), gm) in enumerate(zip(mems, gms)):
        oi, ei, anyk = attention_b(x, ex, mem, em, gx, gm, W, b, arm, mut)
        if mut == "shared_zero" and n == 1:
            o[:], eo[:] = 0.0, 0.0
        if mut == "shared_resplit" and n == 1:  # the first pass's rows read back as hi + lo, zero added, split again
            o[written] = join64(*split(join64(*split(o[written]))))
        o[anyk], eo[anyk] = oi[anyk], ei[anyk]
        written |= anyk
    return o, eo + np.where(written[:, None], store_err(o, eo, planes), 0.0)


def layer_norm_b(y, ey, g, b, mut=None):
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    width = y.shape[-1]
    out = layer_norm(y, g, b, mut)
    mu = y.mean(axis=-1, keepdims=True)
    sig = np.sqrt(((y - mu) ** 2).mean(axis=-1, keepdims=True) + LN_EPS)
    e_in = ey + LN_DEPTH * U * np.abs(y).mean(axis=-1, keepdims=True) + U * np.abs(y - mu)
    nrm = np.sqrt((e_in * e_in).sum(axis=-1, keepdims=True))
    sig_eff = sig - nrm / np.sqrt(width)
    ref = layer_norm(y, g, b)
    cap = 2 * np.sqrt(width - 1.0) * np.abs(g)  # |out - b| <= sqrt(D - 1) |g| whatever the row holds
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(sig_eff > 0, np.abs(g).max() * nrm / sig_eff, np.inf)
    e = np.minimum(e, cap) + C * ((LN_DEPTH / 2 + 4) * U + EPS_RSQRT) * np.abs(ref - b) + C * U * np.abs(ref)
    return out, e + np.zeros_like(y)


def decoder_stages_b(x, ex, mems, gx, gms, sd, prefix, arm, taps=None, mut=None):
    """One decoder pass on tiles -> [(x1, e1), (x2, e2), (x3, e3)]: the x tile after each residual + LayerNorm ([32, 128] each).
    mems = [(mem, em)] or [(memA, emA), (memB, emB)]. taps = (t1, t2), the KERNEL'S OWN x tile after the first and second LayerNorm:
    stage 2 is then fed t1 and stage 3 t2, both exact, so each stage answers for itself; None: the three stages chained."""
    g = _get(sd, prefix)
    planes = arm != "f32"
    shared = len(mems) == 2

    def resid_ln(x, ex, a, ea, lin_name, norm, m=None):
        W, b = g(lin_name + ".weight"), g(lin_name + ".bias")
        y, ey = lin_b(a, ea, W, b, arm)
        yr = x + y
        eyr = ex + ey + C * 3 * U * (np.abs(x) + np.abs(y))
        out, e = layer_norm_b(yr, eyr, g(f".{norm}.weight"), g(f".{norm}.bias"), m)
        return out, e + store_err(out, e, planes)

    a, ea = attention_tiles_b(x, ex, [(x, ex)], gx, [gx], g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias"), arm, False,
                              mut=mut if mut in ("head_cols",) else None)
    x1, e1 = resid_ln(x, ex, a, ea, ".self_attn.out_proj", "norm1", mut if mut == "ln_onepass" else None)
    i1 = (x1, e1) if taps is None else (np.asarray(taps[0], np.float64), np.zeros((32, D)))
    ca = ".self_attn" if mut == "sa_for_ca" else ".multihead_attn"
    c, ec = attention_tiles_b(*i1, mems, gx, gms, g(ca + ".in_proj_weight"), g(ca + ".in_proj_bias"), arm, shared,
                              init=a, mut=mut if mut in ("mask_le", "neighbour", "shared_zero", "shared_resplit", "drop_lo", "drop_lo_q") else None)
    x2, e2 = resid_ln(*i1, c, ec, ".multihead_attn.out_proj", "norm2")
    i2 = (x2, e2) if taps is None else (np.asarray(taps[1], np.float64), np.zeros((32, D)))
    b1 = g(".linear1.bias")
    if mut == "ffn_bias":  # quarter q takes the bias slice of quarter q ^ 1: hidden tile t <-> t ^ 2, unit n <-> n ^ 64
        b1 = b1[np.arange(FF) ^ 64]
    h, eh = lin_b(i2[0], i2[1], g(".linear1.weight"), b1, arm)
    h = np.maximum(h, 0.0)
    eh = eh + store_err(h, eh, planes)
    x3, e3 = resid_ln(*i2, h, eh, ".linear2", "norm3")
    return [(x1, e1), (x2, e2), (x3, e3)]


def decoder_b(x, ex, mems, gx, gms, sd, prefix, arm, mut=None):
    return decoder_stages_b(x, ex, mems, gx, gms, sd, prefix, arm, None, mut)[2]


def pool(tile, n_hints, all8=False):
    """max over the first n_hints rows of each pair's 8-row slot: [32, 128] -> [4, 128]"""
    t = np.asarray(tile, np.float64).reshape(4, 8, D)
    return t[:, :(8 if all8 else n_hints)].max(axis=1)


def mlp_b(pooled, epooled, sd):
    g = _get(sd, "mlp_offsets")
    h, eh = lin_b(pooled, epooled, g(".0.weight"), g(".0.bias"), "f32")
    return lin_b(np.maximum(h, 0.0), eh, g(".2.weight"), g(".2.bias"), "f32")


def tiles_of(obj_enc, hint_enc, n_hints):
    """the product's arrangement of <= 4 pairs (tail pairs duplicate the last): tile A = pairs 0-1, tile B = pairs 2-3 (16 rows each),
    the hint tile = pair p at rows 8 p .. 8 p + n_hints - 1, zeros elsewhere. float32 in, float32 out."""
    n = len(obj_enc)
    idx = np.minimum(np.arange(4), n - 1)
    o = np.asarray(obj_enc, F32)[idx].reshape(64, D)
    h = np.zeros((4, 8, D), F32)
    h[:, :n_hints] = np.asarray(hint_enc, F32)[idx]
    return o[:32].copy(), o[32:].copy(), h.reshape(32, D)


def passes(n_layers):
    """the product's order of decoder passes: (x tile, which, layer) with x in 'A', 'B', 'H'"""
    if n_layers == 0:
        return [("H", 1, 0)]
    out = []
    for l in range(n_layers):
        out += [("A", 0, l), ("B", 0, l), ("H", 1, l)]
    return out


def prefix_of(which, layer, n_layers):
    return "cross_hints" if n_layers == 0 else f"{'cross_hints' if which else 'cross_objects'}.{layer}"


def workgroup_b(obj_enc, hint_enc, sd, n_layers, arm, mut=None, mut_at=None):
    """<= 4 pairs through the tiled reference with the bound chained through every pass -> (offsets [4, 2], bound [4, 2], final hint
    tile, its bound). ``mut`` is applied in decoder pass number ``mut_at`` (or, for 'max_all8', at the pooling)."""
    n_hints = np.asarray(hint_enc).shape[1]
    planes = arm != "f32"
    t = {}
    for name, v in zip("ABH", tiles_of(obj_enc, hint_enc, n_hints)):
        v64 = v.astype(np.float64)  # the raw rows are split on load: hi + lo is the state of the plane arms
        t[name] = (v64, store_err(v64, 0.0, planes) * (v64 != 0))
    gr = {"A": GA, "B": GB, "H": ghint(n_hints)}
    for n, (xn, which, layer) in enumerate(passes(n_layers)):
        mems = [t["A"], t["B"]] if xn == "H" else [t["H"]]
        gms = [GA, GB] if xn == "H" else [gr["H"]]
        t[xn] = decoder_b(*t[xn], mems, gr[xn], gms, sd, prefix_of(which, layer, n_layers), arm, mut if n == mut_at else None)
    hv, he = t["H"]
    pooled = pool(hv, n_hints, all8=(mut == "max_all8"))
    epooled = (he + np.zeros_like(hv)).reshape(4, 8, D)[:, :n_hints].max(axis=1)
    off, eoff = mlp_b(pooled, epooled, sd)
    return off, eoff, hv, he


def cross_match_bound(obj_enc, hint_enc, sd, n_layers, arm):
    """(offsets float64 [P, 2], bound [P, 2]) pair by pair in groups of four — the compounded end-to-end bound"""
    P = len(obj_enc)
    off, tol = np.zeros((P, 2)), np.zeros((P, 2))
    for p0 in range(0, P, 4):
        n = min(4, P - p0)
        o, e, _, _ = workgroup_b(obj_enc[p0:p0 + n], hint_enc[p0:p0 + n], sd, n_layers, arm)
        off[p0:p0 + n], tol[p0:p0 + n] = o[:n], e[:n]
    return off, tol


def ratio(got, ref, tol):
    """worst err / tol (inf where a zero bound is missed; NaN propagates and fails every comparison)"""
    ref = np.asarray(ref, np.float64)
    tol = np.asarray(tol, np.float64) + np.zeros_like(ref)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    if np.isnan(err).any():
        return float("nan")
    return float(r.max()) if r.size else 0.0


def logit_spread(x, mem, gx, gm, W, b):
    """the largest distance of a visible logit below its row's maximum (the argument range ``__expf`` sees)"""
    _, _, (_, _, _, _, z) = mha_core(x, mem, W, b, visible(gx, gm))
    z = np.where(np.isfinite(z), z, 0.0)
    return float(-z.min())


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------------
def weights(n_layers, seed=7):
    """seeded synth.make_fine_weights with the LayerNorm gains and biases moved away from 1 / 0 and apart from each other, so that a
    swapped g1 / g2 / g3 (or b) shows"""
    from text2loc_amd import synth

    sd = dict(synth.make_fine_weights(seed, num_layers=n_layers))
    scale = {"norm1": (1.5, 0.20), "norm2": (0.7, -0.15), "norm3": (0.4, 0.10)}
    for k in list(sd):
        for n, (gs, bo) in scale.items():
            if k.endswith(n + ".weight") and k.startswith("cross_"):
                sd[k] = (np.asarray(sd[k], F32) * F32(gs)).astype(F32)
            if k.endswith(n + ".bias") and k.startswith("cross_"):
                sd[k] = (np.asarray(sd[k], F32) + F32(bo)).astype(F32)
    return sd


def pairs(n_pairs, n_hints, seed, big_mean=False):
    """(obj_enc f32 [n, 16, 128] unit rows, hint_enc f32 [n, n_hints, 128]): hint rows of both signs (a zero padding row could win a
    max). big_mean: the last hint row of the LAST pair has a large mean (mean 5, deviation 1/4: a one-pass variance would show; the
    worst-case bounds of everything that row touches grow with it, so only the fixture of that mutant carries one)"""
    rng = np.random.default_rng([seed, 0xF1B])
    o = rng.standard_normal((n_pairs, 16, D))
    o /= np.linalg.norm(o, axis=-1, keepdims=True)
    h = rng.standard_normal((n_pairs, n_hints, D))
    if big_mean:
        h[-1, -1] = 5.0 + 0.25 * h[-1, -1]
    return o.astype(F32), h.astype(F32)


def lo_aligned(rows, w_row, frac=0.45):
    """rows (float32 [..., 128]) moved so that every element sits ``frac`` of an f16 ulp beside its f16 neighbour, on the side of the
    sign of ``w_row`` [128]: hi = f16(row) is unchanged, every lo residue is as large as a split leaves it and all of them pull one
    product (the output whose weight row is ``w_row``) the same way — the input on which a dropped lo plane shows most"""
    hi = np.asarray(rows, F32).astype(F16)
    step = np.sign(np.asarray(w_row, np.float64)) + np.zeros(hi.shape)
    away = step * np.sign(hi.astype(np.float64)) >= 0  # f16 spacing on the side the element moves to (it halves below a power of two)
    ulp = np.where(away, np.spacing(np.abs(hi)), np.abs(hi) - np.nextafter(np.abs(hi), F16(0))).astype(np.float64)
    out = (hi.astype(np.float64) + frac * ulp * step).astype(F32)
    assert np.array_equal(out.astype(F16), hi)
    return out


LO_COLUMN = 40  # the output column of the value projection the lo fixture is aligned to


def lo_fixture(sd):
    """(A, B, H) float32 tiles, n_hints = 1: every pair's one hint row lo-aligned to row LO_COLUMN of cross_objects.0's cross-attention
    value projection. An object row attending one key has p = 1 and o = v: a lo plane dropped from that projection's activation
    operand leaves the split arm's bound there (tests/test_fine_blocks_cpu.py); the GPU tier runs the same tiles."""
    o, h = pairs(4, 1, 1)
    h = lo_aligned(h, np.asarray(sd["cross_objects.0.multihead_attn.in_proj_weight"])[2 * D + LO_COLUMN])
    return tiles_of(o, h, 1)


def junk(rng, shape):
    """large finite junk for rows nobody may read as a key: +-4 per element (row norm 45, inside what the split arm may hold)"""
    return (4.0 * np.sign(rng.standard_normal(shape))).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library (text2loc_amd/csrc/fine_blocks.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def blocks_path():
    import os.path as osp

    return osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "text2loc_amd", "libt2l_blocks.so")


def load_blocks():
    """the blocks library with the whole C ABI declared (engine.load_library) and the wrappers of this tier"""
    import ctypes as Ct

    from text2loc_amd import engine

    lib = engine.load_library(blocks_path())  # T2LError if it was not built: there is no fallback
    p, i = Ct.c_void_p, Ct.c_int
    lib.t2l_blk_fine_attention.restype, lib.t2l_blk_fine_attention.argtypes = i, [p, i, i, i, i, i, i, p, p, p, p, p, p, p, p, p, p, p]
    lib.t2l_blk_fine_decoder.restype, lib.t2l_blk_fine_decoder.argtypes = i, [p, i, i, i, i] + [p] * 15
    lib.t2l_blk_fine_probe.restype, lib.t2l_blk_fine_probe.argtypes = i, [p, p, p, p, i]
    lib.t2l_blk_last_error.restype, lib.t2l_blk_last_error.argtypes = Ct.c_char_p, []
    return lib
