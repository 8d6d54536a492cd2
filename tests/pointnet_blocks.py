"""TEST INFRASTRUCTURE — float64 stage references, derived tolerances and the fixtures of the PointNet++ block tier
(tests/test_pointnet_blocks_cpu.py, tests/test_gpu_pointnet_blocks.py; profiles/pointnet_blocks.md).

The eval-mode backbone (csrc/pointnet.hip) is held stage by stage: every function below takes the KERNEL'S OWN output of the previous
stage, so no error compounds and every launch group answers for itself. numpy only; nothing of the product is imported.

Centres.  ``fps`` is the restatement's sampling (start at point 0, float32 ``((dx*dx + dy*dy) + dz*dz)``, lowest index on ties). Both
sides evaluate the same float32 expression without FMA, so there is no near-tie a reference could resolve differently: the
expectation is BIT EQUALITY of dst_pos with src_pos[sel]. Neighbour lists use the same float32 rule (``d2 < f32(r*r)``, first 32 in
index order) and relative positions are subtracted in float32, then widened: the inputs of every product are exact on both sides.

Values.  A stage is rows -> Linear + BatchNorm(eval) + ReLU -> Linear + BatchNorm(eval) -> max over the rows of a group -> ReLU,
computed here in float64 with the UNFOLDED BatchNorm of the state dict (s = gamma / sqrt(var + eps)):

    y1 = s1 (W1 x + b1 - m1) + be1,  h = relu(y1);    y2 = s2 (W2 h + b2 - m2) + be2;    out = relu(max_rows y2)

Tolerance (derived, not measured; nothing here is fitted to a kernel's error).  With u = 2^-24 and the magnitudes

    mag1 = |s1| (|W1| |x| + |b1| + |m1|) + |be1|          mag2 = |s2| (|W2| h + |b2| + |m2|) + |be2|

a kernel that folds the BatchNorm in float32 at load time (mfma32.h: fold_batchnorm — s: add, sqrt, divide; W' = W s; b' = (b - m) s +
be: at most F = 6 roundings on any term), accumulates in float32 in ANY order (one rounding per product and pass, K products, 8 more
for the bias column, the bias add behind the max and the MFMA's internal partial sums) and rounds its operands as its arm does, stays
within

    e1 = c [ (P (K1 + 8) + F) u mag1 + rel mag1 + floor (sum|x| + 1 + sum|W1'| + |b1'|) ]
    e2 = |s2| |W2| e1  +  c [ (P (K2 + 8) + F) u mag2 + rel mag2 + floor (sum h + sum|W2'|) ],        c = 2 (second order)

per row, where the arm sets (P, rel, floor) from the packing the kernels really use (mfma_h3.h):

    f32     one v_mfma_f32_32x32x2_f32 pass over exact operands                                   P = 1, rel = 0,               floor = 0
    split   a = hi + lo, hi = f16(a), lo = f16(a - hi): |a - hi - lo| <= max(2^-22 |a|, 2^-25) (f16 subnormals are honoured, the
            2^-25 is half the smallest one); hi*hi + hi*lo + lo*hi, the lo*lo term (<= 2^-22 |a||b|) dropped; f16 x f16 products are
            exact in the float32 accumulator                                                      P = 3, rel = 3 * 2^-22,       floor = 2^-25
    f16     option encoder_f16: one product per operand pair, each operand within max(2^-11 |a|, 2^-25)
                                                                                                  P = 1, rel = 2^-10 + 2^-22,   floor = 2^-25

max and ReLU are 1-Lipschitz, so an element's tolerance is the LARGEST e2 among its candidate rows: a kernel whose arg-max differs
from the reference's because of rounding is still inside it. Only values are held, never selections downstream of rounded arithmetic.
lin1 / lin2 are plain float32 products on the raw weights: tol = c (K + 8) u (|W| |x| + |b|).

Magnitude watch.  The split kernels flag an object when anything that ENTERS a split product (a row value — features, relative
positions — or a hidden activation) reaches 3e4. ``Stage.opmax`` is the float64 reference's largest such operand per object; the
fixtures keep it >= 2 x 3e4 or <= 3e4 / 2 at every level so that the expected flag does not depend on rounding.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
C = 2.0
FOLD = 6
BN_EPS = float(np.float32(1e-5))
WATCH = 3.0e4
ARMS = {  # (P, rel, floor)
    "f32": (1, 0.0, 0.0),
    "split": (3, 3 * 2.0 ** -22, 2.0 ** -25),
    "f16": (1, 2.0 ** -10 + 2.0 ** -22, 2.0 ** -25),
}
PREFIX = "object_encoder.pointnet."
LEVELS = ((0.2, "sa1"), (0.3, "sa2"), (0.4, "sa3"))  # source points 256, 128, 64
MAX_NB = 32
MUTANTS = ("k31", "last32", "drop_last", "radius_1pct", "swap_fps", "le", "self_k1")


# ---------------------------------------------------------------------------------------------------------------------------
# geometry: float32, exactly the kernels' expressions
# ---------------------------------------------------------------------------------------------------------------------------
def d2(p, q):
    """float32 ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own"""
    d = (p.astype(F32) - q.astype(F32)).astype(F32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32)


def fps(pos, mutant=None):
    """pos f32 [n, ns, 3] -> selection order int64 [n, ns // 2] of every object (all objects advance together)"""
    n, ns, _ = pos.shape
    nd = ns // 2
    sel = np.zeros((n, nd), dtype=np.int64)
    mind = d2(pos, pos[:, :1])
    rows = np.arange(n)
    for t in range(1, nd):
        sel[:, t] = np.argmax(mind, axis=1)  # the first maximum
        mind = np.minimum(mind, d2(pos, pos[rows, sel[:, t]][:, None]))
    if mutant == "swap_fps":
        sel[:, [nd - 2, nd - 1]] = sel[:, [nd - 1, nd - 2]]
    return sel


def centres(src_pos, mutant=None):
    """the centres of a level: src_pos[sel], bit for bit"""
    sel = fps(src_pos, mutant)
    return np.take_along_axis(src_pos, sel[:, :, None], axis=1)


def in_radius(src_pos, dst_pos, radius, mutant=None):
    """bool [n, nd, ns]: d2 < f32(r * r)"""
    r = F32(radius) * (F32(1.01) if mutant == "radius_1pct" else F32(1.0))
    r2 = F32(r * r)
    dd = d2(src_pos[:, None, :, :], dst_pos[:, :, None, :])
    return dd <= r2 if mutant == "le" else dd < r2


def neighbours(src_pos, dst_pos, radius, mutant=None):
    """(idx int64 [n, nd, 32], valid bool [n, nd, 32]): the first 32 in-radius source points of every centre in index order"""
    inr = in_radius(src_pos, dst_pos, radius, mutant)
    keep = MAX_NB - 1 if mutant == "k31" else MAX_NB
    if mutant == "last32":
        rank = np.cumsum(inr[..., ::-1], axis=-1)[..., ::-1] - 1  # rank from the end
    else:
        rank = np.cumsum(inr, axis=-1) - 1
    take = inr & (rank < keep)
    if mutant == "drop_last":  # every centre loses its last neighbour (a lone neighbour stays)
        cnt = take.sum(axis=-1, keepdims=True)
        pos_rank = np.cumsum(take, axis=-1) - 1
        take &= ~((pos_rank == cnt - 1) & (cnt > 1))
    order = np.argsort(~take, axis=-1, kind="stable")[..., :MAX_NB]  # the taken indices first, ascending
    return order, np.take_along_axis(take, order, axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# values: float64 with the unfolded BatchNorm, and the per-row bound
# ---------------------------------------------------------------------------------------------------------------------------
def _block(sd, prefix, i):
    g = lambda k: np.asarray(sd[f"{prefix}.{i}{k}"], dtype=np.float64)
    W, b = g(".0.weight"), g(".0.bias")
    s = g(".1.weight") / np.sqrt(g(".1.running_var") + BN_EPS)
    return W, b, s, g(".1.running_mean"), g(".1.bias")


class Stage:
    """ref [G, H2], tol {arm: [G, H2]}, opmax [G] (largest operand entering a product, over the valid rows)"""

    def __init__(self, ref, tol, opmax):
        self.ref, self.tol, self.opmax = ref, tol, opmax


def mlp2_max(rows, valid, sd, prefix, arms=("split",)):
    """rows float64 [G, M, K] (exact float32 values), valid bool [G, M] -> Stage: the two get_mlp blocks of ``prefix`` per row, the max
    over a group's valid rows, ReLU."""
    G, M, K1 = rows.shape
    x = rows.reshape(G * M, K1)
    W1, b1, s1, m1, be1 = _block(sd, prefix, 0)
    W2, b2, s2, m2, be2 = _block(sd, prefix, 1)
    K2 = W2.shape[1]
    ax, aW1, aW2 = np.abs(x), np.abs(W1), np.abs(W2)
    y1 = (x @ W1.T + b1 - m1) * s1 + be1
    h = np.maximum(y1, 0.0)
    mag1 = (ax @ aW1.T + np.abs(b1) + np.abs(m1)) * np.abs(s1) + np.abs(be1)
    y2 = (h @ W2.T + b2 - m2) * s2 + be2
    mag2 = (h @ aW2.T + np.abs(b2) + np.abs(m2)) * np.abs(s2) + np.abs(be2)
    sW1 = (aW1 * np.abs(s1)[:, None]).sum(axis=1) + (np.abs(b1) + np.abs(m1)) * np.abs(s1) + np.abs(be1)  # sum|W1'| + |b1'| per output
    sW2 = (aW2 * np.abs(s2)[:, None]).sum(axis=1)
    sx, sh = ax.sum(axis=1, keepdims=True) + 1.0, h.sum(axis=1, keepdims=True)
    v = valid.reshape(G, M, 1)
    ref = np.maximum(np.where(v, y2.reshape(G, M, -1), -np.inf).max(axis=1), 0.0)
    tol = {}
    for arm in arms:
        P, rel, floor = ARMS[arm]
        e1 = C * (((P * (K1 + 8) + FOLD) * U + rel) * mag1 + floor * (sx + sW1))
        e2 = (e1 @ aW2.T) * np.abs(s2) + C * (((P * (K2 + 8) + FOLD) * U + rel) * mag2 + floor * (sh + sW2))
        tol[arm] = np.where(v, e2.reshape(G, M, -1), 0.0).max(axis=1)
    op = np.maximum(ax.max(axis=1), h.max(axis=1)).reshape(G, M)
    return Stage(ref, tol, np.where(valid, op, 0.0).max(axis=1))


def sa_rows(src_pos, src_x, dst_pos, cell_offsets, radius, self_loops, mutant=None):
    """(rows float64 [n * nd, 33, cin + 3], valid [n * nd, 33]) of a SetAbstraction level: [x_j | pos_j - pos_i] of the <= 32
    neighbours and, with ``self_loops``, of node k = (o - first object of the cell) * nd + t of the cell's batch (row 32)."""
    n, ns, _ = src_pos.shape
    nd = dst_pos.shape[1]
    idx, valid = neighbours(src_pos, dst_pos, radius, mutant)
    o = np.arange(n)[:, None, None]
    rel = (src_pos[o, idx].astype(F32) - dst_pos[:, :, None, :].astype(F32)).astype(F32)
    rows = np.concatenate([src_x[o, idx].astype(np.float64), rel.astype(np.float64)], axis=-1)  # [n, nd, 32, cin + 3]
    extra = np.zeros((n, nd, 1, rows.shape[-1]))
    if self_loops:
        base = np.zeros(n, dtype=np.int64)
        for c in range(len(cell_offsets) - 1):
            base[int(cell_offsets[c]):int(cell_offsets[c + 1])] = int(cell_offsets[c])
        k = (np.arange(n) - base)[:, None] * nd + np.arange(nd)[None, :] + (1 if mutant == "self_k1" else 0)
        node = base[:, None] * ns + k  # into the object-major flat batch
        flat_pos, flat_x = src_pos.reshape(-1, 3), src_x.reshape(n * ns, -1)
        erel = (flat_pos[node].astype(F32) - dst_pos.astype(F32)).astype(F32)
        extra = np.concatenate([flat_x[node].astype(np.float64), erel.astype(np.float64)], axis=-1)[:, :, None, :]
    rows = np.concatenate([rows, extra], axis=2)
    valid = np.concatenate([valid, np.full((n, nd, 1), bool(self_loops))], axis=2)
    return rows.reshape(n * nd, MAX_NB + 1, -1), valid.reshape(n * nd, MAX_NB + 1)


def sa_level(level, src_pos, src_x, dst_pos, cell_offsets, sd, self_loops=True, arms=("split",), mutant=None):
    """Stage of level 0..2 from ITS source points / features and ITS centres: ref, tol [n, nd, H2]; opmax [n]"""
    radius, name = LEVELS[level]
    n, nd = dst_pos.shape[:2]
    rows, valid = sa_rows(src_pos, src_x, dst_pos, cell_offsets, radius, self_loops, mutant)
    st = mlp2_max(rows, valid, sd, f"{PREFIX}{name}.point_conv.local_nn", arms)
    h2 = st.ref.shape[-1]
    return Stage(st.ref.reshape(n, nd, h2), {a: t.reshape(n, nd, h2) for a, t in st.tol.items()}, st.opmax.reshape(n, nd).max(axis=1))


def ga(x3, p3, sd, arms=("split",)):
    """GlobalAbstraction: get_mlp([259, 512, 1024]) on [x3 | p3] of the 32 remaining points, max -> Stage [n, 1024]"""
    rows = np.concatenate([x3.astype(np.float64), p3.astype(np.float64)], axis=-1)
    return mlp2_max(rows, np.ones(rows.shape[:2], dtype=bool), sd, PREFIX + "ga.mlp", arms)


def lin(x, sd, name):
    """(ref, tol) of relu(x W^T + b) with the raw float32 weights of ``name`` (lin1, lin2): a plain float32 product"""
    W, b = np.asarray(sd[PREFIX + name + ".weight"], np.float64), np.asarray(sd[PREFIX + name + ".bias"], np.float64)
    x = x.astype(np.float64)
    return np.maximum(x @ W.T + b, 0.0), C * (W.shape[1] + 8) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))


def ratio(got, ref, tol):
    """worst err / tol (inf where a zero bound is missed; NaN propagates and fails every comparison)"""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def hold_all(levels, pos, rgb, cell_offsets, sd, self_loops, arm_of):
    """Every stage of one call against its reference. levels: dict of the kernel's p1, x1, p2, x2, p3, x3, f0, f1, f2 (numpy float32).
    arm_of: one arm name, or the arm of every object at each of the four MLP stages ([4][n]: levels 1-3, the global MLP). Returns
    {stage: worst err / tol}; ``centres L`` is 0.0 for bit equality, inf otherwise. Also returns the per-stage opmax [4, n]."""
    n = pos.shape[0]
    arm_of = np.array([[arm_of] * n] * 4) if isinstance(arm_of, str) else np.asarray(arm_of)
    arms = tuple(sorted(set(arm_of.ravel())))
    pick = lambda tol, stage: np.stack([tol[a][o] for o, a in enumerate(arm_of[stage])])
    out, opmax = {}, []
    src_p, src_x = pos, rgb
    for L in range(3):
        gp, gx = levels[f"p{L + 1}"], levels[f"x{L + 1}"]
        out[f"centres{L + 1}"] = 0.0 if np.array_equal(gp.view(np.uint32), centres(src_p).view(np.uint32)) else float("inf")
        st = sa_level(L, src_p, src_x, gp, cell_offsets, sd, self_loops, arms)
        out[f"x{L + 1}"] = ratio(gx, st.ref, pick(st.tol, L))
        opmax.append(st.opmax)
        src_p, src_x = gp, gx
    st = ga(src_x, src_p, sd, arms)
    out["f0"] = ratio(levels["f0"], st.ref, pick(st.tol, 3))
    opmax.append(st.opmax)
    out["f1"] = ratio(levels["f1"], *lin(levels["f0"], sd, "lin1"))
    out["f2"] = ratio(levels["f2"], *lin(levels["f1"], sd, "lin2"))
    return out, np.stack(opmax)


# ---------------------------------------------------------------------------------------------------------------------------
# numpy models of the arms' operand rounding (the CPU tier's consistency check): float32 fold as the loader's, operands rounded as
# the packing does, products and sums in float64
# ---------------------------------------------------------------------------------------------------------------------------
def _f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=F32).astype(np.float16).astype(np.float64)


def _product(a, b, arm):
    """a [.., K] @ b [K, ..] with both operands (exact float32 values) rounded as ``arm`` does"""
    if arm == "f32":
        return a @ b
    ah, bh = _f16(a), _f16(b)
    if arm == "f16":
        return ah @ bh
    al = _f16((np.asarray(a, F32) - ah.astype(F32)).astype(F32))
    bl = _f16((np.asarray(b, F32) - bh.astype(F32)).astype(F32))
    return ah @ bh + ah @ bl + al @ bh


def _fold32(sd, prefix, i):
    g = lambda k: np.asarray(sd[f"{prefix}.{i}{k}"], dtype=F32)
    s = (g(".1.weight") / np.sqrt((g(".1.running_var") + F32(1e-5)).astype(F32)).astype(F32)).astype(F32)
    W = (g(".0.weight") * s[:, None]).astype(F32)
    b = (((g(".0.bias") - g(".1.running_mean")).astype(F32) * s).astype(F32) + g(".1.bias")).astype(F32)
    return W.astype(np.float64), b.astype(np.float64)


def model_mlp2_max(rows, valid, sd, prefix, arm):
    """what a kernel of ``arm`` computes up to summation order: [G, H2] float64"""
    G, M, K = rows.shape
    W1, b1 = _fold32(sd, prefix, 0)
    W2, b2 = _fold32(sd, prefix, 1)
    x1 = np.concatenate([rows.reshape(G * M, K), np.ones((G * M, 1))], axis=1)  # the bias rides on a constant-1 column
    h = np.maximum(_product(x1, np.concatenate([W1, b1[:, None]], axis=1).T, arm), 0.0).astype(F32).astype(np.float64)
    y2 = _product(h, W2.T, arm).reshape(G, M, -1)
    m = np.where(valid[:, :, None], y2, -np.inf).max(axis=1)
    return np.maximum(m + b2, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------------
def weights(seed=0):
    from text2loc_amd import synth

    sd = synth.make_object_branch_weights(seed)
    sd.update(synth.make_pointnet_weights(seed))
    return sd


def table_fixture():
    """the issue's fixture: 5 objects in cells of 2 and 3, level-1 in-radius counts from 1 to 61"""
    from text2loc_amd import synth

    cells = synth.make_cells(2, seed=1, min_obj=2, max_obj=3)
    pos, rgb = synth.make_sampled_points(cells, 1)
    return pos, rgb, cells["offsets"].astype(np.int32)


def count_fixture(n_obj, seed, offsets=None):
    """n_obj synthetic objects; ``offsets`` None: one cell per 3 objects"""
    from text2loc_amd import synth

    if offsets is None:
        offsets = np.minimum(np.arange(0, n_obj + 3, 3), n_obj)
        offsets = np.unique(offsets)
    offsets = np.asarray(offsets, dtype=np.int32)
    pos, rgb = synth.make_sampled_points({"offsets": np.array([0, n_obj])}, seed)
    return pos, rgb, offsets


RADII = (0.2, 0.3, 0.4)


def _clusters(rng, sizes, spread=0.004):
    """points of tight clusters (sizes in index order) whose centres sit >= 1 apart on a line"""
    out = []
    for i, s in enumerate(sizes):
        c = np.array([1.1 * i - 1.1 * (len(sizes) - 1) / 2, 0.1 * (i % 2), 0.0])
        out.append(c + spread * rng.uniform(-1, 1, size=(s, 3)))
    return out


def geometry_fixture():
    """(pos, rgb, offsets, info): objects built for the conditions tests/test_pointnet_blocks_cpu.py asserts.
      0 radius boundary: point 0 at the origin; (f32(r), 0, 0) and nextafter(f32(r), 0) on another axis for r = .2, .3, .4 at indices
        1..6; the rest within 0.04 of the origin (every ball of centre 0 saturates, the probes sit inside its first 32)
      1 saturation: clusters of exactly 1, 31, 32, 33 and 159 points, far apart
      2 chunk placement: cluster P = 31 points in indices 0..63 + 20 in 64..127; cluster Q all inside 192..255
      3 all 256 points identical      4 two distinct points repeated      5 a line (sparse balls)
    cells: [0, 1, 2], [], [3, 4], [5]"""
    rng = np.random.default_rng(20240611)
    pos = np.zeros((6, 256, 3))
    probes = []
    for i, r in enumerate(RADII):
        on = np.zeros(3)
        on[0] = F32(r)
        under = np.zeros(3)
        under[1 + i % 2] = float(np.nextafter(F32(r), F32(0))) * (1 if i < 2 else -1)
        probes += [on, under]
    pos[0, 1:7] = probes
    pos[0, 7:] = 0.04 * rng.uniform(-1, 1, size=(249, 3)) / np.sqrt(3)
    pos[1] = np.concatenate(_clusters(rng, (1, 31, 32, 33, 159)))
    P, R, Q, S, T = _clusters(rng, (51, 33, 40, 108, 24))
    pos[2] = np.concatenate([P[:31], R, P[31:], S, Q, T])  # 0..30 P | 31..63 R | 64..83 P | 84..191 S | 192..231 Q | 232..255 T
    pos[3] = 0.25
    two = np.array([[0.1, -0.2, 0.3], [0.15, 0.1, 0.25]])
    pos[4] = two[np.arange(256) % 2]
    pos[5] = np.linspace(-1, 1, 256)[:, None] * np.array([1.0, 0.0, 0.0])
    rgb = rng.uniform(0, 1, size=(6, 256, 3))
    info = {"boundary": 0, "saturation": 1, "chunks": 2, "identical": 3, "two": 4, "line": 5,
            "chunk_P": np.r_[0:31, 64:84], "chunk_Q": np.r_[192:232]}
    return pos.astype(F32), rgb.astype(F32), np.array([0, 3, 3, 5, 6], dtype=np.int32), info


def cell_frame_fixture():
    """raw cell-frame coordinates (`--no_pc_augment`): objects a few percent of the cell wide anywhere in [0, 1]^3 — most balls hold
    more than 32 points, relative positions are small against the absolute ones — and a facade across the cell"""
    rs = np.random.default_rng(21)
    n = 4
    centre, extent = rs.uniform(0.05, 0.95, size=(n, 1, 3)), rs.uniform(0.01, 0.12, size=(n, 1, 3))
    pos = (centre + rs.standard_normal((n, 256, 3)) * extent).astype(F32)
    pos[0] = rs.uniform(0, 1, size=(256, 3)).astype(F32) * np.array([1, 0.05, 0.6], F32)
    rgb = np.clip(rs.uniform(0, 1, size=(n, 1, 3)) + 0.1 * rs.standard_normal((n, 256, 3)), 0, 1).astype(F32)
    return pos, rgb, np.array([0, 1, 4], dtype=np.int32)


def reference_levels(pos, rgb, cell_offsets, sd, self_loops=True):
    """the float64 references chained on THEMSELVES (rounded to float32 between the stages): stands in for a kernel where the CPU tier
    needs level buffers — the magnitude fixture's search, the mutant tests"""
    lv, src_p, src_x = {}, pos, rgb
    for L in range(3):
        p = centres(src_p)
        x = sa_level(L, src_p, src_x, p, cell_offsets, sd, self_loops, ("f32",)).ref.astype(F32)
        lv[f"p{L + 1}"], lv[f"x{L + 1}"] = p, x
        src_p, src_x = p, x
    lv["f0"] = ga(src_x, src_p, sd, ("f32",)).ref.astype(F32)
    lv["f1"] = lin(lv["f0"], sd, "lin1")[0].astype(F32)
    lv["f2"] = lin(lv["f1"], sd, "lin2")[0].astype(F32)
    return lv


def magnitude_fixture():
    """(pos, rgb, offsets, sd, expect flags int32 [n], first flagged stage per object (0 = never)): object 1's colours are scaled so
    that its level-1 operands reach 2 x 3e4; object 3's so that nothing reaches 3e4 / 2 at level 1 and something exceeds 2 x 3e4 at
    level 2. With the synthetic weights a level's output is SMALLER than its hidden layer, so no colour scale alone can do the latter:
    this fixture's state dict has the affine of sa1's LAST BatchNorm (gamma, beta) multiplied by 32 — level 1's operands are unchanged,
    its output (level 2's operand) is 32 times larger. One object per cell: no self-loop row carries one object's magnitudes into
    another. The scale of object 3 is found from the reference's own magnitudes (they grow linearly with the colours), and every
    object's margin is asserted by the CPU tier."""
    sd = dict(weights(0))
    for k in (".1.1.weight", ".1.1.bias"):
        name = PREFIX + "sa1.point_conv.local_nn" + k
        sd[name] = (np.asarray(sd[name], dtype=F32) * F32(32.0)).astype(F32)
    pos, rgb, _ = count_fixture(5, 9)
    offsets = np.arange(6, dtype=np.int32)
    rgb = rgb.copy()
    rgb[1] *= F32(2.0e5)
    probe = rgb.copy()
    probe[3] *= F32(1.0e3)
    _, op = hold_all(reference_levels(pos, probe, offsets, sd), pos, probe, offsets, sd, True, "f32")
    m1, m2 = float(op[0, 3]), float(op[1, 3])
    scale = 1.0e3 * np.sqrt((WATCH / 2) * (2 * WATCH)) / np.sqrt(m1 * m2)  # the geometric middle of the admissible interval
    rgb[3] *= F32(scale)
    return pos, rgb, offsets, sd, np.array([0, 1, 0, 1, 0], dtype=np.int32), np.array([0, 1, 0, 2, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library (text2loc_amd/csrc/pointnet_blocks.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def blocks_path():
    import os.path as osp

    return osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "text2loc_amd", "libt2l_blocks.so")


def load_blocks():
    """the blocks library with the whole C ABI declared (engine.load_library) and the block wrappers of this tier"""
    import ctypes as C

    from text2loc_amd import engine

    lib = engine.load_library(blocks_path())  # T2LError if it was not built: there is no fallback
    p, i = C.c_void_p, C.c_int
    lib.t2l_blk_pointnet_levels.restype, lib.t2l_blk_pointnet_levels.argtypes = i, [p, i, i, i] + [p] * 9
    lib.t2l_blk_pn_fps.restype, lib.t2l_blk_pn_fps.argtypes = i, [p, p, p, i, i]
    lib.t2l_blk_last_error.restype, lib.t2l_blk_last_error.argtypes = C.c_char_p, []
    return lib
