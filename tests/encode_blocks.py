"""TEST INFRASTRUCTURE — float64 references, derived tolerances and fixtures of the encoder-layer block tier
(tests/test_encode_blocks_cpu.py, tests/test_gpu_encode_blocks.py; profiles/encode_blocks.md).

``planes_layer`` (csrc/encode.hip) — the post-norm transformer layer that the two-cell cell encoder and the one-launch
``t2l_text_inter`` share — is held ONE call at a time through the dev library's door (csrc/encode_blocks.hip), which copies out every
stage of the layer: the attention output (B planes), the X planes behind the first residual + LayerNorm, the hidden planes of every
feed-forward pass and the result (X planes, or the f32 tile of ``last_to_f32``). Every stage reference is fed the KERNEL'S OWN
predecessor (float64(hi) + float64(lo) of the tap before it, or of the planes the test packed), so nothing compounds across stages.

Two kinds of checks.

*Derived bounds on any weights* (``layer_stages``): the forms of tests/fine_blocks.py, imported from there (``lin_b``,
``attention_b``, ``layer_norm_b``, ``store_err``) with the width and the head size of the instance: a product as
(P (K + 8)) u mag + rel mag + floor per arm, a plane store as max(2^-22 |v|, 2^-25), the softmax and LayerNorm forms. The LayerNorm's
depth constant LN_DEPTH = 16 of fine_blocks covers ``resid_ln``'s association: 2 additions inside a register quad, 4 over the quads,
1 across the lane halves and D / 32 <= 8 over the waves, 15 on the longest path. This is the run that sees masks, rows, heads, tiles
and bias slices.

*Exact models on selection weights* (``selection_stages``): every row of out_proj, linear1, linear2 and of the v block of in_proj has
ONE entry +-1, so a split product leaves exactly +-(hi + lo) of one operand element in the accumulator (hi + lo of a split float32 is
a float32: both parts are multiples of the value's last place; every other term is an exact zero), the plain-f16 product exactly
+-hi. What the epilogue computes behind it is float32 arithmetic in a known order — the bias add, the residual
``plane_get4(x) + (acc + b)``, the ReLU — and ``plane_put4``'s split is RNE f16 twice (``split``). So
  * the hidden planes of every feed-forward pass are demanded BIT FOR BIT;
  * with S = 1 in the text mask every row is its own only key, p = 1 exactly (``__expf(0)``, 1.f / 1.f), and the attention tap is v
    to the 2^-22 of the P V split: exactly hi(v) + lo(v) of the float32 v = acc + bv (within max(2^-22 |v|, 2^-25) of v, a bound a
    split attains with equality, so the test demands the value itself);
  * the two LayerNorm taps are held to the LayerNorm's OWN roundings around a float64 LayerNorm of the exactly known float32 row
    (``layer_norm_b`` with a zero input error), no product bound in front: about 2.5e-5 of the value. That is some 25 times what
    a LayerNorm's roundings can do to a row: ``layer_norm_b`` charges the mean's LN_DEPTH u |mean| to every element and takes the
    2-norm over the D columns, a worst case a uniform shift of the row cannot reach. The form is kept as fine_blocks derives it
    (one derivation, imported); it is 100 to 1000 times below the same stage behind a Gaussian product and the one-pass and eps
    mutants sit 19 to 440 times above it.
  * the attention tap of every other selection case (Gaussian q and k blocks: nothing is exact there) is held to the derived
    attention bound of ``attention_stage`` on the same weights, so no tap of any case goes uncompared.
The *tilted* selection has entries +-(1 + 2^-12): hi = 1, lo = 2^-12. The split product is x_hi + x_hi 2^-12 + x_lo with at most three
float32 roundings of partial sums no larger than 2 |x| (and lo lo is not computed: 2^-12 |x_lo| <= 2^-23 |x|): within 4 u |x| of
x_hi (1 + 2^-12) + x_lo. A dropped weight lo plane is 2^-12 |x| = 4096 u |x| away. The plain-f16 arm reads hi alone: exactly +-x_hi.
The *small* selection scales the first LayerNorm's gain and bias by 0.02: the rows entering the second LayerNorm then have a variance
near 1e-3 and an eps of 1e-6 shows there too. The *high-mean* selection moves the rows that enter both LayerNorms to |mean| >= 100 standard deviations through the biases of
out_proj and linear2 (a one-pass variance then leaves the LayerNorm's own bound; tests/test_encode_blocks_cpu.py asserts the factor).

The only measured numbers are the four probe constants below (``__expf``, ``1.f / x``, ``1.0f / sqrtf(x)`` as encode_blocks.hip
compiles them): twice the worst value ``t2l_blk_enc_probe`` measured against float64 on the MI355X; the GPU half repeats the probe
on every run.

Around the layer, the free device functions of both encoder kernels have one-call doors of their own, with references and bounds
below: the row stages ``normalize_rows`` / ``normalize_rows_d`` / ``layer_norm_rows_d`` (``normalize_rows_b``,
``layer_norm_rows_b``), the two-cell kernel's feature branch ``small_mlp`` with ``gemm32`` (``small_mlp_b``), and every product of
the one-cell kernel through ``mm_tiles`` in its three arms on the loader's packing (``product_b``: Gaussian weights inside the
product bound, selection weights EQUAL to +-x / +-(hi + lo) / +-f16(x), tilted within 4 u |x|; mlp_merge's slots among them, with a
BatchNorm that is the identity in the loader's float32).

Not covered: what exists only inside the ``__global__`` bodies of ``encode_cells2_kernel`` and ``encode_cells_shaped_kernel`` —
taps there changed the shipped listing. That is the merge loop and its epilogue, the max-pool and the final normalise, the one-cell
kernel's attention core and epilogues, the table look-ups with their clamps, and with them the cell-shape cases (profiles/
encode_blocks.md, "what stays unseen")."""
import numpy as np

from tests import fine_blocks as FB

F32, F16, F64 = np.float32, np.float16, np.float64
U, C = FB.U, FB.C
ARMS = ("split", "f16")
ARM_ID = {"split": 1, "f16": 2}
KS = 28  # live key rows of the cell instance (kS)

# twice the worst error t2l_blk_enc_probe measured on the MI355X (2^20 samples each; profiles/encode_blocks.md)
PROBE = {
    "EPS_EXP": 2 * 9.401e-7,    # relative, __expf on [-16, 0]              (measured 9.401e-07)
    "EXP_TAIL": 2 * 1.002e-13,  # absolute, __expf on [-2^17, -16]          (measured 1.002e-13)
    "EPS_RCP": 2 * 5.960e-8,    # relative, 1.f / x on [1e-6, 1e6]          (measured 5.960e-08: correctly rounded)
    "EPS_RSQRT": 2 * 8.941e-8,  # relative, 1.0f / sqrtf(x) on [1e-6, 1e6]  (measured 8.941e-08)
}
# the bounds imported from fine_blocks carry that module's constants; this tier's may not be larger (asserted on the CPU and, against
# the probe, on the GPU), so the imported forms hold here as they stand
assert all(PROBE[k] <= getattr(FB, k) for k in PROBE)


class Geo:
    """one compiled instance of planes_layer"""

    def __init__(self, D, hd, ffp, text):
        self.D, self.hd, self.ffp, self.text = D, hd, ffp, text
        self.heads, self.FF, self.NW = D // hd, ffp * D, D // 32
        self.inst = 1 if text else 0

    def __repr__(self):
        return f"{'text' if self.text else 'cell'}_d{self.D}_hd{self.hd}"

    def units(self, c):
        """hidden units of feed-forward pass c in the order of the B planes' columns (planes_layer: cbase / tf)"""
        h = self.D // 2
        return np.concatenate([c * h + np.arange(h), self.FF // 2 + c * h + np.arange(h)])


CELL = Geo(256, 64, 2, False)
TEXT = {(D, heads): Geo(D, D // heads, 4, True) for D, heads in ((256, 4), (128, 4), (128, 2), (256, 8))}
TEXT_S = (1, 2, 5, 6, 16, 32)


def split(v):
    return FB.split(v)


def join64(hi, lo):
    return FB.join64(hi, lo)


def join32(hi, lo):
    """plane_get4: hi + lo in float32 (one rounding; exact for the two parts of a split float32)"""
    return hi.astype(F32) + lo.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------------
def vis_cell(mut=None):
    """may query row i see key row j: the 28 slots, zero pads included; the 4 dead rows of the tile are no keys"""
    j = np.arange(32)
    return np.broadcast_to((j <= KS) if mut == "mask_le" else (j < KS), (32, 32)).copy()


def vis_text(S, mut=None):
    """grp[i] == grp[j], grp = row / S: whole descriptions, then one partial group of the rows past the tile's last description"""
    grp = np.arange(32) // S
    own = grp[:, None] == grp[None, :]
    if mut == "neighbour":
        own |= (grp[:, None] ^ 1) == grp[None, :]
    return own


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 stages on any weights, with the derived bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _g(sd, prefix):
    return lambda k: np.asarray(sd[prefix + k], F64)


def ln_value(y, g, b, mut=None):
    """LayerNorm in float64; mutants: a one-pass variance in float32, eps 1e-6"""
    if mut == "ln_onepass":
        return FB.layer_norm(y, g, b, "ln_onepass")
    mu = y.mean(axis=-1, keepdims=True)
    d = y - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + (1e-6 if mut == "ln_eps" else FB.LN_EPS)) * g + b


def last_kstep(K):
    """the k-values of the last k-step of a product packed for K (mfma_h3.h: lane half kh of step s holds kh K/2 + 8 s ..)"""
    return np.concatenate([np.arange(K // 2 - 8, K // 2), np.arange(K - 8, K)])


def _operands(a, W, which, mut):
    """the operands of product ``which`` under a product mutant 'act_lo:<which>' / 'w_lo:<which>' / 'kstep:<which>'"""
    if mut == "act_lo:" + which:
        a = split(a)[0].astype(F64)
    if mut == "w_lo:" + which:
        W = W.astype(F32).astype(F16).astype(F64)
    if mut == "kstep:" + which:
        W = W.copy()
        W[:, last_kstep(W.shape[1])] = 0.0
    return a, W


def resid_ln_b(x, ex, a, ea, W, b, g, be, arm, planes, which, mut=None):
    """LayerNorm(x + a W^T + b) g + be -> (value, bound); ``planes``: the result is stored to planes (split once)"""
    am, Wm = _operands(a, W, which, mut)
    y, ey = FB.lin_b(a, ea, W, b, arm)
    ym = FB.linear(am, Wm, b) if (am is not a or Wm is not W) else y
    yr, eyr = x + y, ex + ey + C * 3 * U * (np.abs(x) + np.abs(y))
    _, e = FB.layer_norm_b(yr, eyr, g, be)
    out = ln_value(x + ym, g, be, mut if mut in ("ln_onepass", "ln_eps") else None)
    return out, e + FB.store_err(out, e, planes)


def attention_stage(geo, x, sd, prefix, vis, arm, mut=None):
    """the B planes behind the attention: (o, bound), the store's split included"""
    g = _g(sd, prefix)
    z = np.zeros_like(x)
    W, b = g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias")
    fb_mut = {"act_lo:v": "drop_lo", "act_lo:q": "drop_lo_q", "act_lo:k": "drop_lo_k"}.get(mut)
    o, eo, _ = FB.attention_b(x, z, x, z, None, None, W, b, arm, vis=vis, hd=geo.hd)
    if mut in ("act_lo:v", "act_lo:q", "act_lo:k", "w_lo:v", "kstep:v", "head_cols"):
        Wm = W
        if mut == "w_lo:v":
            Wm = W.copy()
            Wm[2 * geo.D:] = W[2 * geo.D:].astype(F32).astype(F16).astype(F64)
        if mut == "kstep:v":
            Wm = W.copy()
            Wm[2 * geo.D:, last_kstep(geo.D)] = 0.0
        o = FB.mha_core(x, x, Wm, b, vis, fb_mut, geo.hd)[0]
        if mut == "head_cols":  # head 0's output in head 1's columns and the other way round
            o = o.copy()
            o[:, :geo.hd], o[:, geo.hd:2 * geo.hd] = o[:, geo.hd:2 * geo.hd].copy(), o[:, :geo.hd].copy()
    return o, eo + FB.store_err(o, eo, True)


def layer_stages(geo, sd, prefix, xh, xl, vis, arm, last_to_f32, taps=None, mut=None, vis_mut=None):
    """One tile through one planes_layer call -> {stage: (value float64 [32, D], bound)} for 'att', 'x1', 'hid0' .. and 'out'.
    xh, xl: the tile's X planes (f16 [32, D]). taps: {'att': (hi, lo), 'x1': (hi, lo), 'hid': [(hi, lo)] * ffp} — the kernel's own
    planes of THIS tile; every stage is then fed its predecessor's tap (exact); None: the reference's own values, chained with
    their bounds. mut: a change of the reference (tests/test_encode_blocks_cpu.py); the bounds are those of the unchanged one."""
    g = _g(sd, prefix)
    D = geo.D
    x = join64(xh, xl)
    z = np.zeros((32, D))
    out = {}
    out["att"] = attention_stage(geo, x, sd, prefix, vis if vis_mut is None else vis_mut, arm, mut)
    if vis_mut is not None:
        out["att"] = (out["att"][0], attention_stage(geo, x, sd, prefix, vis, arm)[1])
    a, ea = out["att"] if taps is None else (join64(*taps["att"]), z)
    out["x1"] = resid_ln_b(x, z, a, ea, g(".self_attn.out_proj.weight"), g(".self_attn.out_proj.bias"), g(".norm1.weight"),
                           g(".norm1.bias"), arm, True, "out_proj", mut)
    x1, e1 = out["x1"] if taps is None else (join64(*taps["x1"]), z)
    W1, b1 = g(".linear1.weight"), g(".linear1.bias")
    hid = []
    for c in range(geo.ffp):
        u = geo.units(c)
        h, eh = FB.lin_b(x1, e1, W1[u], b1[u], arm)
        if mut in ("act_lo:linear1", "w_lo:linear1", "kstep:linear1"):
            h = FB.linear(*_operands(x1, W1[u], "linear1", mut), b1[u])
        if mut == "bias_tile":  # every 32-unit tile takes the bias slice of its neighbour
            h = h - b1[u] + b1[u ^ 32]
        h = np.maximum(h, 0.0)
        eh = eh + FB.store_err(h, eh, True)
        out[f"hid{c}"] = (h, eh)
        hid.append((h, eh) if taps is None else (join64(*taps["hid"][c]), z))
    hfull, efull = np.zeros((32, geo.FF)), np.zeros((32, geo.FF))
    for c in range(geo.ffp):
        src = hid[c ^ 1] if mut == "pass_swap" else hid[c]  # pass c reads the other pass's hidden units
        hfull[:, geo.units(c)], efull[:, geo.units(c)] = src
    out["out"] = resid_ln_b(x1, e1, hfull, efull, g(".linear2.weight"), g(".linear2.bias"), g(".norm2.weight"), g(".norm2.bias"),
                            arm, not last_to_f32, "linear2", mut)
    return out


def stage_names(geo):
    return ["att", "x1"] + [f"hid{c}" for c in range(geo.ffp)] + ["out"]


def logit_spread(geo, x, sd, prefix, vis):
    """the largest distance of a visible logit below its row's maximum: the softmax bound wants it inside FB.LOGIT_RANGE"""
    g = _g(sd, prefix)
    z = FB.mha_core(x, x, g(".self_attn.in_proj_weight"), g(".self_attn.in_proj_bias"), vis, None, geo.hd)[2][4]
    return float(-np.where(np.isfinite(z), z, 0.0).min())


# ---------------------------------------------------------------------------------------------------------------------------
# selection weights and their exact models
# ---------------------------------------------------------------------------------------------------------------------------
def selection(N, K, passes=1):
    """(pi [N], sign [N]): output row n picks input k = pi(n) with sign +-1. In the packing of mfma_h3.h a k-step s covers
    k in [8 s, 8 s + 8) of the lower and of the upper half of K; a 32-row output tile (one wave's) has K / 16 steps. Up to 32 steps
    (K <= 512) every tile draws from EVERY step, from both lane halves among them; beyond (the text layer's linear2, K = 4 D at
    D = 256) a tile's first 2 * passes rows take the first and the last step of every feed-forward pass (``passes`` of them, K / 16 /
    passes steps each) and the rest walk on through the steps from tile to tile, so that the tiles together cover every step. The
    element within the step moves with the row and the tile. (tests/text_head_blocks.py: selection visits 16-wide contiguous steps
    of a 256-row tile — another packing; the rule, round-robin over the steps, is the same.)"""
    n = np.arange(N)
    j, t = n % 32, n // 32
    steps = K // 16
    if steps <= 32:
        step = (j + t) % steps
        half = ((j // steps) if steps < 32 else j) & 1
    else:
        per = steps // passes
        special = np.array([s for c in range(passes) for s in (c * per, (c + 1) * per - 1)])
        ns = len(special)
        step = np.where(j < ns, special[np.minimum(j, ns - 1)], (t * (32 - ns) + (j - ns)) % steps)
        half = (j + t) & 1
    pi = half * (K // 2) + 8 * step + (3 * j + 5 * t) % 8
    sign = np.where(((n * 2654435761) >> 7) & 1, -1.0, 1.0)
    return pi.astype(np.int64), sign


SEL_KEYS = ("v", "out_proj", "linear1", "linear2")


def selection_of(geo):
    D = geo.D
    return {"v": selection(D, D), "out_proj": selection(D, D), "linear1": selection(geo.FF, D), "linear2": selection(D, geo.FF, geo.ffp)}


def selection_layer(sd, prefix, geo, tilt=False, high_mean=False, small=False, seed=5):
    """the layer ``prefix`` of state dict ``sd`` with the four chosen matrices replaced by selection matrices (entries +-1, or
    +-(1 + 2^-12) when tilted); q and k blocks, biases and LayerNorm vectors stay (high_mean: the biases of out_proj and linear2 are
    moved to +400 / -1200 so that the rows entering both LayerNorms have a mean hundreds of standard deviations large; small: the
    first LayerNorm's gain and bias and linear2's bias are scaled by 0.02, so that the rows entering the SECOND LayerNorm have a
    variance near 1e-3, where an eps of 1e-6 instead of 1e-5 shows)"""
    sd = dict(sd)
    D = geo.D
    e = F32(1.0 + 2.0 ** -12) if tilt else F32(1.0)
    sel = selection_of(geo)

    def mat(key, N, K):
        pi, sign = sel[key]
        W = np.zeros((N, K), F32)
        W[np.arange(N), pi] = sign.astype(F32) * e
        return W

    Win = np.array(sd[prefix + ".self_attn.in_proj_weight"], F32)
    Win[2 * D:] = mat("v", D, D)
    sd[prefix + ".self_attn.in_proj_weight"] = Win
    sd[prefix + ".self_attn.out_proj.weight"] = mat("out_proj", D, D)
    sd[prefix + ".linear1.weight"] = mat("linear1", geo.FF, D)
    sd[prefix + ".linear2.weight"] = mat("linear2", D, geo.FF)
    if high_mean:
        rng = np.random.default_rng([seed, 0x4D])
        sd[prefix + ".self_attn.out_proj.bias"] = (400.0 + 0.1 * rng.standard_normal(D)).astype(F32)
        sd[prefix + ".linear2.bias"] = (-1200.0 + 0.1 * rng.standard_normal(D)).astype(F32)
    if small:
        for k in (".norm1.weight", ".norm1.bias", ".linear2.bias"):
            sd[prefix + k] = (np.asarray(sd[prefix + k], F32) * F32(0.02)).astype(F32)
    return sd


def sel_acc32(hi, lo, pi, sign, arm, mut=None):
    """what the MFMAs leave in the accumulator for a +-1 selection: +-(hi + lo) of the picked element (plain f16: +-hi), float32"""
    a = hi.astype(F32)[:, pi]
    if arm == "split" and mut != "act_lo":
        a = a + lo.astype(F32)[:, pi]
    if mut == "kstep":
        a = np.where(np.isin(pi, last_kstep(hi.shape[1]))[None, :], F32(0), a)
    return (sign.astype(F32)[None, :] * a).astype(F32)


def sel_acc64(hi, lo, pi, sign, arm, tilt, mut=None):
    """(value float64, bound) of the accumulator: exact for +-1; for the tilted selection in the split arm
    +-(x_hi (1 + 2^-12) + x_lo) within 4 u |x|"""
    if not (tilt and arm == "split"):
        return sel_acc32(hi, lo, pi, sign, arm, mut).astype(F64), 0.0
    h, l = hi.astype(F64)[:, pi], lo.astype(F64)[:, pi]
    if mut == "act_lo":
        l = 0.0 * l
    v = h * ((1.0 + 2.0 ** -12) if mut != "w_lo" else 1.0) + l
    if mut == "kstep":
        v = np.where(np.isin(pi, last_kstep(hi.shape[1]))[None, :], 0.0, v)
    return sign[None, :] * v, 4 * U * (np.abs(h) + np.abs(l))


def selection_stages(geo, sd, prefix, xh, xl, taps, arm, last_to_f32, tilt=False, S=None, mut=None):
    """The stages of one tile that selection weights make known without a product bound -> {stage: (kind, ref, tol)}.
    kind 'bits': ref = (hi, lo) planes demanded bit for bit; 'tol': ref float64 with its bound. ``taps`` as in layer_stages (required:
    every stage is fed the kernel's own predecessor). S = 1: the attention tap too. mut = (stage, what) changes that stage's model."""
    g = _g(sd, prefix)
    D = geo.D
    sel = selection_of(geo)
    exact = not (tilt and arm == "split")
    m = lambda stage: mut[1] if mut is not None and mut[0] == stage else None
    out = {}
    if S == 1:
        acc, ea = sel_acc64(xh, xl, *sel["v"], arm, tilt, m("att"))
        bv = g(".self_attn.in_proj_bias")[2 * D:]
        if exact:
            # p = 1: o = v_hi 1 + v_lo 1 exactly, a float32; its re-split at the store keeps the VALUE (the bits of hi and lo may
            # move when v_hi + v_lo lands on an f16 tie). Demanded exactly — inside the max(2^-22 |v|, 2^-25) of the P V split, which
            # a split can attain with equality
            v = join64(*split(acc.astype(F32) + bv.astype(F32)))
            out["att"] = ("tol", v, np.zeros_like(v))
        else:
            v = acc + bv
            e = ea + 2 * U * np.abs(v)  # the bias add, p v
            out["att"] = ("tol", v, e + FB.store_err(v, e, True))

    def ln_stage(stage, res_hi, res_lo, a_hi, a_lo, key, bias, gn, bn, planes):
        acc, ea = sel_acc64(a_hi, a_lo, *sel[key], arm, tilt, m(stage) if m(stage) in ("act_lo", "w_lo", "kstep") else None)
        b = g(bias)
        if exact:  # the row that enters the LayerNorm is a known float32
            y = (join32(res_hi, res_lo) + (acc.astype(F32) + b.astype(F32))).astype(F64)
            ey = np.zeros_like(y)
        else:
            x = join64(res_hi, res_lo)
            y = x + (acc + b)
            ey = ea + 2 * U * (np.abs(acc + b) + np.abs(y))
        _, e = FB.layer_norm_b(y, ey, g(gn + ".weight"), g(gn + ".bias"))
        val = ln_value(y, g(gn + ".weight"), g(gn + ".bias"), m(stage) if m(stage) in ("ln_onepass", "ln_eps") else None)
        return ("tol", val, e + FB.store_err(val, e, planes))

    out["x1"] = ln_stage("x1", xh, xl, *taps["att"], "out_proj", ".self_attn.out_proj.bias", ".norm1", ".norm1", True)
    x1h, x1l = taps["x1"]
    b1 = g(".linear1.bias")
    pi1, s1 = sel["linear1"]
    for c in range(geo.ffp):
        u = geo.units(c)
        mc = m(f"hid{c}")
        bu = b1[u ^ 32] if mc == "bias_tile" else b1[u]
        acc, ea = sel_acc64(x1h, x1l, pi1[u], s1[u], arm, tilt, mc if mc in ("act_lo", "w_lo", "kstep") else None)
        if exact:
            out[f"hid{c}"] = ("bits", split(np.maximum(acc.astype(F32) + bu.astype(F32), F32(0))), None)
        else:
            h = np.maximum(acc + bu, 0.0)
            e = ea + U * np.abs(acc + bu)
            out[f"hid{c}"] = ("tol", h, e + FB.store_err(h, e, True))
    hh, hl = np.zeros((32, geo.FF), F16), np.zeros((32, geo.FF), F16)
    for c in range(geo.ffp):
        src = taps["hid"][c ^ 1] if m("out") == "pass_swap" else taps["hid"][c]
        hh[:, geo.units(c)], hl[:, geo.units(c)] = src
    out["out"] = ln_stage("out", x1h, x1l, hh, hl, "linear2", ".linear2.bias", ".norm2", ".norm2", not last_to_f32)
    return out


def reference_taps(geo, sd, prefix, xh, xl, vis, arm):
    """the taps an exact kernel would leave: the float64 stages of the tile, each rounded to float32 and split (CPU half)"""
    st = layer_stages(geo, sd, prefix, xh, xl, vis, arm, False)
    return {"att": split(st["att"][0]), "x1": split(st["x1"][0]), "hid": [split(st[f"hid{c}"][0]) for c in range(geo.ffp)]}


def ratio(got, ref, tol):
    return FB.ratio(got, ref, tol)


# ---------------------------------------------------------------------------------------------------------------------------
# the row stages outside planes_layer: normalize_rows (encode.hip), normalize_rows_d / layer_norm_rows_d (encode_shaped.hip)
# ---------------------------------------------------------------------------------------------------------------------------
# A normalise is out = v * (1.f / fmaxf(sqrtf(ss), 1e-12f)), ss = sum v^2 in float32: D / 64 (at most 4) squares and additions in a
# lane, six levels of wave_sum — every term positive, so ss is within 11 u of the sum RELATIVELY and its square root within 6 u;
# sqrtf and the quotient together are the probe's 1.0f / sqrtf (EPS_RSQRT; EPS_RCP on top for the fmaxf in between, which keeps the two
# from being one instruction), and the product with v is one more rounding. The error is relative in every element (the factor is the
# row's): NORM_REL |out|; a zero row stays zero and rows >= nvalid are zeroed: bound 0 there.
NORM_REL = C * (6 * U + PROBE["EPS_RSQRT"] + PROBE["EPS_RCP"] + U)
ROW_NVALID = (0, 1, 27, 28, 32)


def normalize_rows_b(x32, nvalid, mut=None):
    """(value, bound) of F.normalize over the columns of rows < nvalid of x32 (float32 [32, D]), rows >= nvalid zero. Mutants: the row
    behind the last valid one normalised too ('nvalid_plus'), the norm over the first half of the columns ('half')"""
    x = np.asarray(x32, F64)
    D = x.shape[1]
    nrm = np.sqrt((x[:, :D // 2 if mut == "half" else D] ** 2).sum(axis=1, keepdims=True))
    out = x / np.maximum(nrm, 1e-12)
    out[nvalid + (1 if mut == "nvalid_plus" else 0):] = 0.0
    return out, NORM_REL * np.abs(out)


def layer_norm_rows_b(x32, g, b, mut=None):
    """(value, bound) of LayerNorm(D, eps 1e-5) over the rows of x32: layer_norm_b with a zero input error (the rows are exact
    float32). LN_DEPTH = 16 covers layer_norm_rows_d's sums: D / 64 - 1 <= 3 additions in a lane and six levels of wave_sum.
    Mutants: 'ln_onepass', 'ln_eps', and the gain read one column on ('gain_shift')"""
    x = np.asarray(x32, F64)
    g, b = np.asarray(g, F64), np.asarray(b, F64)
    _, e = FB.layer_norm_b(x, np.zeros_like(x), g, b)
    return ln_value(x, np.roll(g, 1) if mut == "gain_shift" else g, b, mut if mut in ("ln_onepass", "ln_eps") else None), e


def row_tiles(D, seed, n_wg=2):
    """float32 [n_wg, 32, D]: Gaussian rows over six decades of scale, a zero row, rows 1000 standard deviations off zero (a one-pass
    variance), rows of variance 4e-4 (eps)"""
    rng = np.random.default_rng([seed, D, 0x90])
    x = rng.standard_normal((n_wg, 32, D)) * np.exp(rng.uniform(-7, 7, (n_wg, 32, 1)))
    x[:, 5] = 0.0
    x[:, 9] = 1000.0 + rng.standard_normal((n_wg, D))
    x[:, 10] = -1000.0 + rng.standard_normal((n_wg, D))
    x[:, 20] = 0.02 * rng.standard_normal((n_wg, D))
    x[:, 21] = 0.5 + 0.02 * rng.standard_normal((n_wg, D))
    return x.astype(F32)


def row_gain(D, seed):
    rng = np.random.default_rng([seed, D, 0x91])
    return rng.uniform(0.5, 1.5, D).astype(F32), (0.2 * rng.standard_normal(D)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the products of the one-cell kernel: mm_tiles on the loader's packing, one product per call (t2l_blk_encs_product)
# ---------------------------------------------------------------------------------------------------------------------------
# which: 0 q, 1 k, 2 v, 3 out_proj, 4 linear1, 5 linear2 pass sub, 6 mlp_merge slot sub, 7 second layer of the pos / color / num encoder
PRODUCTS = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0), (6, 1), (6, 2), (6, 3), (7, 0), (7, 2))
PRODUCT_ARMS = {0: "f32", 1: "split", 2: "f16"}
SHAPED = {128: 4, 256: 4}  # width -> heads of the models the product door is run on
FOLD_REL = 4 * U  # the loader folds an eval-mode BatchNorm in float32: g / sqrtf(var + eps), W * s — three roundings per weight


def _fold(sd, lin, bn):
    """(W, b) of Linear `lin` with BatchNorm `bn` folded, float64 from the float32 tensors"""
    g = lambda k: np.asarray(sd[k], F64)
    s = g(bn + ".weight") / np.sqrt(g(bn + ".running_var") + 1e-5)
    # where the loader's float32 scale g / sqrtf(var + 1e-5f) is exactly 1 (the identity BatchNorm of the selection fixtures), W * s
    # is W itself in the loaded model, and so it is here
    s32 = np.asarray(sd[bn + ".weight"], F32) / np.sqrt(np.asarray(sd[bn + ".running_var"], F32) + F32(1e-5), dtype=F32)
    s = np.where(s32 == F32(1.0), 1.0, s)
    return g(lin + ".weight") * s[:, None], (g(lin + ".bias") - g(bn + ".running_mean")) * s + g(bn + ".bias")


def pass_units(D, sub):
    """hidden units of linear2's pass `sub` in the order of the one-cell kernel's buf columns (2 D hidden units)"""
    h = D // 2
    return np.concatenate([sub * h + np.arange(h), D + sub * h + np.arange(h)])


def product_matrix(sd, D, which, layer, sub):
    """(W float64 [N, kin], folded): the matrix with out = x W^T for product (which, layer, sub) of state dict sd"""
    p = CELL_PREFIX.format(layer)
    g = lambda k: np.asarray(sd[p + k], F64)
    if which <= 2:
        return g(".self_attn.in_proj_weight")[which * D:(which + 1) * D], False
    if which == 3:
        return g(".self_attn.out_proj.weight"), False
    if which == 4:
        return g(".linear1.weight"), False
    if which == 5:
        return g(".linear2.weight")[:, pass_units(D, sub)], False
    if which == 6:
        return _fold(sd, "object_encoder.mlp_merge.0.0", "object_encoder.mlp_merge.0.1")[0][:, sub * D:(sub + 1) * D], True
    name = ("pos_encoder", "color_encoder", "num_encoder")[sub]
    return _fold(sd, f"object_encoder.{name}.1.0", f"object_encoder.{name}.1.1")[0], True


def product_b(x32, W, folded, arm, mut=None):
    """(value, bound) of out = x W^T as mm_tiles computes it in `arm`. W with one entry +-1 per row: the value is exact (bound 0:
    +-x on the f32 MFMA, +-(hi + lo) of the split x, +-f16(x)); one entry +-(1 + 2^-12) per row: within 4 u |x| (plain f16 reads
    hi = 1: exact); anything else: the product bound of lin_b, plus FOLD_REL mag where the loader folded a BatchNorm into W.
    Mutants: 'act_lo' / 'w_lo' (the lo plane of an operand dropped), 'kstep' (the last k-step dropped), 'tile_swap' (every 32-wide
    output tile written where its neighbour belongs)"""
    x = np.asarray(x32, F32)
    W = np.asarray(W, F64)
    a = x.astype(F64) if arm == "f32" else join64(*split(x)) if arm == "split" else split(x)[0].astype(F64)
    Wa = W if arm != "f16" else W.astype(F32).astype(F16).astype(F64)
    nz = np.abs(Wa[Wa != 0])
    one_per_row = (np.count_nonzero(Wa, axis=1) <= 1).all()
    if one_per_row and (nz == 1.0).all():
        tol = np.zeros((x.shape[0], W.shape[0]))
    elif one_per_row and np.isin(nz, (1.0, 1.0 + 2.0 ** -12)).all():
        tol = 4 * U * (np.abs(a) @ np.abs(Wa).T)
    else:
        _, tol = FB.lin_b(x.astype(F64), np.zeros(x.shape), W, np.zeros(W.shape[0]), arm)
        if folded:
            tol = tol + FOLD_REL * (np.abs(x.astype(F64)) @ np.abs(W).T)
        a, Wa = x.astype(F64), W  # (the arm's roundings are inside the bound)
    if mut == "act_lo":
        a = split(x)[0].astype(F64)
    if mut == "w_lo":
        Wa = Wa.astype(F32).astype(F16).astype(F64)
    if mut == "kstep":
        Wa = Wa.copy()
        Wa[:, last_kstep(W.shape[1])] = 0.0
    val = a @ Wa.T
    if mut == "tile_swap":
        val = val[:, np.arange(val.shape[1]) ^ 32]
    return val, tol


NUM_MEAN, NUM_STD = float(F32(1826.6844940968194)), float(F32(2516.8905096993817))  # the kernels' float32 constants
SMALL_NAMES = ("pos_encoder", "color_encoder", "num_encoder")


def small_mlp_input(sub, seed, n_wg=2):
    """float32 [n_wg, 32, IN]: centres / colours in [0, 1]^3, point counts between 50 and 10,000"""
    rng = np.random.default_rng([seed, sub, 0x5A])
    return (rng.uniform(50, 10000, (n_wg, 32, 1)) if sub == 2 else rng.uniform(0, 1, (n_wg, 32, 3))).astype(F32)


def small_mlp_b(sd, sub, x32, nobj, mut=None):
    """(value, bound) [32, 256] of one feature branch as small_mlp computes it: (num: (n - mean) / std,) hidden = relu(W1 v + b1),
    y = relu(W2 hidden + b2) on the f32 MFMA, both with the loader's float32 BatchNorm folding (FOLD_REL mag on top of the product
    bound), F.normalize over the rows < nobj, zero rows behind. A normalise of y known within ey, eps = ||ey||_2, n = ||y||_2:
    |y' / n' - y / n| <= ey / (n - eps) + |y| eps / (n (n - eps)), plus NORM_REL |out| for its own roundings.
    Mutants: 'no_num_norm' (the point count enters raw), 'nobj_plus', 'kstep' (gemm32's last k-step dropped)"""
    name = "object_encoder." + SMALL_NAMES[sub]
    W1, b1 = _fold(sd, name + ".0.0", name + ".0.1")
    W2, b2 = _fold(sd, name + ".1.0", name + ".1.1")
    v = np.asarray(x32, F64)
    ev = np.zeros_like(v)
    if sub == 2:
        ev = 2 * U * (np.abs(v) + NUM_MEAN) / NUM_STD
        if mut != "no_num_norm":
            v = (v - NUM_MEAN) / NUM_STD
    h, eh = FB.lin_b(v, ev, W1, b1, "f32")
    eh = eh + FOLD_REL * (np.abs(v) @ np.abs(W1).T + np.abs(b1))
    h = np.maximum(h, 0.0)
    y, ey = FB.lin_b(h, eh, W2, b2, "f32")
    ey = ey + FOLD_REL * (h @ np.abs(W2).T + np.abs(b2))
    if mut == "kstep":
        W2m = W2.copy()
        W2m[:, [28, 29, 30, 31, 60, 61, 62, 63]] = 0.0  # (pack_half_split: the last float4 of each k half)
        y = FB.linear(h, W2m, b2)
    y = np.maximum(y, 0.0)
    n = np.sqrt((y * y).sum(axis=1, keepdims=True))
    eps = np.sqrt((ey * ey).sum(axis=1, keepdims=True))
    out = y / np.maximum(n, 1e-12)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(n > eps, ey / (n - eps) + np.abs(y) * eps / (n * (n - eps)), np.inf) + NORM_REL * np.abs(out)
    keep = nobj + (1 if mut == "nobj_plus" else 0)
    out[keep:], e[nobj:] = 0.0, 0.0
    return out, e


def shaped_weights(D, kind="gauss"):
    """state dict of the object branch at width D (two layers, embedding mode, four features). kind 'sel' / 'tilt': EVERY matrix of
    both layers (q and k blocks included) and every slot of mlp_merge is a selection matrix, and mlp_merge's BatchNorm is the
    identity in the loader's float32 (gain 1, bias 0, mean 0, var 1 - 1e-5: sqrtf(var + eps) == 1)"""
    from text2loc_amd import synth

    sd = dict(synth.make_object_branch_weights(W_SEED, embed_dim=D))
    if kind == "gauss":
        return sd
    e = F32(1.0 + 2.0 ** -12) if kind == "tilt" else F32(1.0)

    def mat(N, K, passes=1, shift=0):
        pi, sign = selection(N, K, passes)
        W = np.zeros((N, K), F32)
        W[np.arange(N), (pi + shift) % K] = sign.astype(F32) * e
        return W

    for l in range(2):
        p = CELL_PREFIX.format(l)
        sd[p + ".self_attn.in_proj_weight"] = mat(3 * D, D)
        sd[p + ".self_attn.out_proj.weight"] = mat(D, D, shift=8 * l)
        sd[p + ".linear1.weight"] = mat(2 * D, D)
        sd[p + ".linear2.weight"] = mat(D, 2 * D, 2)
    m = "object_encoder.mlp_merge.0."
    sd[m + "0.weight"] = np.concatenate([mat(D, D, shift=16 * s) for s in range(4)], axis=1)
    sd[m + "1.weight"], sd[m + "1.bias"] = np.ones(D, F32), np.zeros(D, F32)
    sd[m + "1.running_mean"], sd[m + "1.running_var"] = np.zeros(D, F32), np.full(D, 1.0 - 1e-5, F32)
    assert np.all(np.sqrt(sd[m + "1.running_var"] + F32(1e-5), dtype=F32) == F32(1.0))
    return sd


def product_input(D, which, seed, n_wg=2):
    """float32 [n_wg, 32, kin]: rows over four decades, a zero row; ReLU outputs (non-negative) for the hidden-layer products"""
    kin = 64 if which == 7 else D
    rng = np.random.default_rng([seed, D, which, 0x9D])
    x = rng.standard_normal((n_wg, 32, kin)) * np.exp(rng.uniform(-4, 4, (n_wg, 32, 1)))
    x[:, 11] = 0.0
    return (np.abs(x) if which in (5, 7) else x).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------------
LN_SCALE = {"norm1": (1.5, 0.20), "norm2": (0.7, -0.15)}


def _move_norms(sd, prefix):
    """LayerNorm gains away from 1 and apart from each other, biases apart (tests/fine_blocks.py: weights): a swapped g1 / g2 shows"""
    for n, (gs, bo) in LN_SCALE.items():
        sd[f"{prefix}.{n}.weight"] = (np.asarray(sd[f"{prefix}.{n}.weight"], F32) * F32(gs)).astype(F32)
        sd[f"{prefix}.{n}.bias"] = (np.asarray(sd[f"{prefix}.{n}.bias"], F32) + F32(bo)).astype(F32)


CELL_PREFIX = "obj_inter_module.{}"
TEXT_PREFIX = "language_encoder.inter_module.0"
W_SEED = 7


def cell_weights(kind="gauss"):
    """state dict of the object branch (two layers, embedding mode) for t2l_load_weights; kind: 'gauss', 'sel', 'tilt', 'mean', 'small'"""
    from text2loc_amd import synth

    sd = dict(synth.make_object_branch_weights(W_SEED))
    for l in range(2):
        _move_norms(sd, CELL_PREFIX.format(l))
        if kind != "gauss":
            sd = selection_layer(sd, CELL_PREFIX.format(l), CELL, tilt=kind == "tilt", high_mean=kind == "mean", small=kind == "small", seed=l)
    return sd


def text_weights(D, heads, kind="gauss"):
    """state dict of the language head at width D for t2l_text_head_load_weights (inter_num_heads = heads)"""
    from text2loc_amd import synth

    sd = dict(synth.make_language_head_weights(W_SEED, embed_dim=D))
    _move_norms(sd, TEXT_PREFIX)
    if kind != "gauss":
        sd = selection_layer(sd, TEXT_PREFIX, TEXT[(D, heads)], tilt=kind == "tilt", high_mean=kind == "mean", small=kind == "small")
    return sd


def cell_tiles(seed, second_zero=False, scale=1.0):
    """float32 [1, 2, 32, 256]: one workgroup's two cells as the merge leaves them — unit rows for the first nobj slots (27 and 13 objects),
    zero pad slots up to 28, and Gaussian junk in the 4 dead rows (after a first layer they hold a LayerNorm's output; no key, no
    pooled row, but a query all the same). second_zero: the second tile all zero."""
    rng = np.random.default_rng([seed, 0xCE11])
    x = np.zeros((1, 2, 32, 256))
    for t, nobj in enumerate((27, 13)):
        r = rng.standard_normal((nobj, 256))
        x[0, t, :nobj] = scale * r / np.linalg.norm(r, axis=-1, keepdims=True)
        x[0, t, KS:] = 0.1 * scale * rng.standard_normal((4, 256))
    if second_zero:
        x[0, 1] = 0.0
    return x.astype(F32)


def cell_tiles_wide(seed, scale=1.0):
    """as cell_tiles with rows of a second layer's size (a LayerNorm's output: |x| ~ 1 per element), all 32 rows live"""
    rng = np.random.default_rng([seed, 0xCE12])
    return (scale * rng.standard_normal((1, 2, 32, 256))).astype(F32)


def text_pack(sent, n_desc, S):
    """sent float32 [n_desc * S, D] -> float32 [n_wg, 2, 32, D] as text_inter_fused2_kernel packs it: floor(32 / S) whole descriptions
    per tile, two tiles per workgroup, zero rows behind"""
    D = sent.shape[1]
    dpt = 32 // S
    n_wg = (n_desc + 2 * dpt - 1) // (2 * dpt)
    x = np.zeros((n_wg, 2, 32, D), F32)
    for d in range(n_desc):
        w, r = divmod(d, 2 * dpt)
        t, p = divmod(r, dpt)
        x[w, t, p * S:(p + 1) * S] = sent[d * S:(d + 1) * S]
    return x


def text_sentences(D, S, seed, n_wg=2, scale=1.0):
    """(sent, n_desc) filling n_wg workgroups but for the last tile's last description: a tail workgroup whose second tile is short — or,
    with one description per tile (S > 16), has no description at all"""
    dpt = 32 // S
    n_desc = max(1, n_wg * 2 * dpt - 1)
    rng = np.random.default_rng([seed, S, D])
    return (scale * rng.standard_normal((n_desc * S, D))).astype(F32), n_desc


def text_unpack_max(y, sent, n_desc, S):
    """the kernel's epilogue in float32: out[d] = max over the description's sentences of y + sent"""
    D = sent.shape[1]
    dpt = 32 // S
    out = np.zeros((n_desc, D), F32)
    for d in range(n_desc):
        w, r = divmod(d, 2 * dpt)
        t, p = divmod(r, dpt)
        out[d] = (y[w, t, p * S:(p + 1) * S].astype(F32) + sent[d * S:(d + 1) * S]).max(axis=0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library (text2loc_amd/csrc/encode_blocks.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def load_blocks():
    import ctypes as Ct

    lib = FB.load_blocks()
    p, i = Ct.c_void_p, Ct.c_int
    lib.t2l_blk_enc_layer.restype, lib.t2l_blk_enc_layer.argtypes = i, [p, i, i, i, i, i, i] + [p] * 12
    lib.t2l_blk_enc_probe.restype, lib.t2l_blk_enc_probe.argtypes = i, [p, p, p, p, i]
    lib.t2l_blk_enc_normalize.restype, lib.t2l_blk_enc_normalize.argtypes = i, [i, p, i]
    lib.t2l_blk_encs_rows.restype, lib.t2l_blk_encs_rows.argtypes = i, [i, i, i, p, p, p, i]
    lib.t2l_blk_enc_small_mlp.restype, lib.t2l_blk_enc_small_mlp.argtypes = i, [p, i, i, p, i, p]
    lib.t2l_blk_encs_product.restype, lib.t2l_blk_encs_product.argtypes = i, [p, i, i, i, i, i, p, p]
    return lib
