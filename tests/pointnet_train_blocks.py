"""TEST INFRASTRUCTURE — float64 references, derived bounds and case lists of the PointNet++ TRAINING block tier
(tests/test_pointnet_train_blocks_cpu.py, tests/test_gpu_pointnet_train_blocks.py; profiles/pointnet_train_blocks.md).

The chain tests (tests/test_gpu_pointnet_train.py, tests/test_gpu_train_arith.py) cannot be tight: one arg-max, ReLU or 32nd-neighbour
decision that falls the other way inside float32 rounding moves everything upstream by a percent. Here every kernel of
csrc/pointnet_train.h and csrc/gemm_rows2.h runs as ONE launch (csrc/train_blocks.hip: t2l_blk_pn_*) on synthetic operands with planted
index tables. At that level a block is a continuous function of its inputs, or takes its discrete decisions as inputs, or makes them on
inputs CONDITIONED so that the decision is unambiguous (``condition_*`` below; the CPU tier asserts it). Every element of every output
is compared. numpy only; arithmetic from ``oracle.arith``; nothing of the product is imported.

Bounds (u = 2^-24, factor = tests/train_blocks.py's 2; nothing is fitted to a run)

  products        train_blocks.linear:  factor (K + 8) u (|A| @ |B| + |bias|)
  fused operand   the kernels compute relu(fma(A - mean, rg, beta)) in float32 — two roundings, each below u (|A - mean| |rg| + |beta|) —
                  so + 2 u (|A - mean| |rg| + |beta|) @ |W|. ReLU is 1-Lipschitz. With bf16 / split-bf16 operands the float32 value is then
                  ROUNDED (a step function): the inputs are conditioned (``condition_fused``) so that every float32 within 4 u (...) of
                  the float64 value rounds to the same bf16 operand; the split-bf16 operand hi + lo has steps below that band where lo
                  is small, so there the inputs are conditioned to keep it within 16 u (...) across the band and the term is 16 u (...) @ |W|
  bf16 stores     (arith 1) the stored value is the RNE rounding of something within tol of the reference:
                  |got - ref| <= tol + 2^-8 (|ref| + tol).  bf16 keeps 8 significand bits, so the unit roundoff of its RNE rounding is
                  2^-8 (1 + 2^-8 rounds to 1); with 2^-9 the float32 restatement of the CPU tier, which is correct by construction,
                  stands at 1.97 of the bound
  BatchNorm sums  from the float64 product (not from the stored rows): colsum's form over the n rows of the cell plus the propagated
                  product bound —  S1: factor (n + 8) u sum|C| + sum tol;   S2: factor (n + 8) u sum C^2 + sum (2 |C| tol + tol^2)
  tables          mean, rstd, rg, running statistics, k1, k2, dgamma, dbeta, the element-wise backward: first-order propagation of the
                  bounds above through the closed forms of pointnet_train.h, doubled, plus R u (sum of the magnitudes of the terms)
                  for the R float32 roundings the kernel itself performs on the way (R is counted per output below, 4 at the least)
  scatter         np.add.at in float64; per address the sum of the row bounds that meet there + (multiplicity + 8) u sum|v|
  exact           index tables, arg, ysel (= y at arg), pos_out, nbr33, cnt_g, the gather and the layout kernels: bit equality
"""
import numpy as np

from oracle import arith
from tests import train_blocks as TB

U = TB.U
FACTOR = 2.0
F32 = np.float32
BN_EPS = float(F32(1e-5))
MOM = float(F32(0.1))
ONE_MINUS_MOM = float(F32(1.0) - F32(0.1))  # (1.f - momentum) as the kernel forms it
SEED = 11
ARITHS = TB.ARITHS
gauss = TB.gauss

# (K, N, fused) of the layers whose product forms the BatchNorm sums; (K, N) of the input-gradient products; (K, N, cols) scattered
ROWS2_STAT = ((32, 32, False), (32, 64, True), (96, 128, False), (128, 128, True), (160, 256, False), (256, 256, True),
              (288, 512, False), (512, 1024, False))
ROWS2_PLAIN = ((64, 32), (128, 128), (256, 256), (1024, 512), (512, 288))
ROWS2_SCAT = ((128, 64, 64), (256, 128, 128))
ROWS2_NARROW = ((32, 32, False), (32, 64, True), (128, 128, True))  # the shapes that also run the rows above 8 * 32 * CUs
ROWS2_SMALL_M = (1, 31, 32, 33, 257, 600)
# (N, K, k_real, fused)
TN2_SHAPES = ((64, 32, 32, True), (128, 128, 128, True), (256, 256, 256, True), (1024, 512, 512, False), (32, 32, 6, False),
              (128, 96, 67, False), (256, 160, 131, False), (512, 288, 259, False))


def store(x, ar):
    """an edge-row tensor as it lives in memory: bf16 with arith 1, float32 otherwise"""
    return arith.store(x, ar)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers' own formulas (pointnet_train.h: gemm_rows2, gemm_tn2) — the case lists are derived from them
# ---------------------------------------------------------------------------------------------------------------------------
def rows2_plan(M, N, K, ar, fused, n_cu):
    """(tp, grid, rpw): column tiles per pass, workgroups, rows per wave"""
    bpe = 2 if ar == arith.BF16 else 4
    maxt = (6 if fused else 8) if ar == arith.BF16 else 4
    tp = max(1, min(maxt, N // 32, (128 * 1024) // (32 * K * bpe)))
    passes = (N // 32 + tp - 1) // tp
    tp = (N // 32 + passes - 1) // passes
    grid = min(n_cu, (M + 255) // 256)
    rpw = ((M + grid * 8 - 1) // (grid * 8) + 31) // 32 * 32
    return tp, grid, rpw


def tn2_plan(M, N, K, n_cu):
    """[(gx, gy, gz, kt, rpw, SR)] of the one or two launches (part 0: the blocks of kb_tiles k tiles; part 1: a narrower last block)"""
    KT = K // 32
    kblocks = (KT + 3) // 4
    kb_tiles = (KT + kblocks - 1) // kblocks
    gy, nt = (N + 255) // 256, min(256, N) // 32
    SR = 8 // nt * 32
    last_tiles = KT - kb_tiles * (kblocks - 1)
    out = []
    for part in range(2):
        nfull = kblocks if last_tiles == kb_tiles else kblocks - 1
        gz = nfull if part == 0 else (0 if last_tiles == kb_tiles else 1)
        if gz == 0:
            continue
        gx = max(1, n_cu // (gy * gz))
        gx = min(gx, (M + SR - 1) // SR)
        rpw = ((M + gx - 1) // gx + SR - 1) // SR * SR
        out.append((gx, gy, gz, kb_tiles if part == 0 else last_tiles, rpw, SR))
    return out


def sizes_to_row_cell(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


def cell_layout(M, layout, rpw=32):
    """cell sizes of M rows. one: a single cell | two: 2 rows, then the rest | inside: a boundary inside a 32-row tile | tile: a
    boundary exactly on a tile boundary | small: cells of 2, 31, 32 and 33 rows, then the rest | wave: boundaries between two tiles of
    ONE wave (row rpw * w + 32 of waves 1 and 3), inside the last tile of wave 2 and on the boundary between waves 4 and 5"""
    if isinstance(layout, (list, tuple)):
        assert sum(layout) == M
        return list(layout)
    if layout == "one" or M < 4:
        return [M]
    if layout == "two":
        return [2, M - 2]
    if layout == "inside":
        b = max(2, (M // 2) // 32 * 32 + 13)
        return [b, M - b] if M - b >= 2 else [M]
    if layout == "tile":
        b = max(32, (M // 2) // 32 * 32)
        return [b, M - b]
    if layout == "small":
        head = [2, 31, 32, 33]
        assert M - sum(head) >= 2
        return head + [M - sum(head)]
    if layout == "wave":
        assert rpw >= 64 and M > 6 * rpw
        cuts = [rpw + 32, 3 * rpw - 7, 3 * rpw + 32, 5 * rpw]
        edges = [0] + cuts + [M]
        return [b - a for a, b in zip(edges[:-1], edges[1:])]
    raise ValueError(layout)


def rows2_big_rows(n_cu):
    """(M2, M3): the smallest row counts (ragged ends) at which a wave walks two tiles — the running BatchNorm sums and their flush
    across tiles execute from here on — and three"""
    return 8 * 32 * n_cu + 77, 2 * 8 * 32 * n_cu + 4 * 32 * n_cu + 45


def rows2_cases(n_cu):
    """[(kind, K, N, fused, cols, M, layout)], kind in stat / plain / scat"""
    out = []
    small = {1: ("one",), 31: ("two",), 32: ("one",), 33: ("inside",), 257: ("tile",), 600: ("small", "one")}
    for K, N, fused in ROWS2_STAT:
        for M in ROWS2_SMALL_M:
            out += [("stat", K, N, fused, 0, M, lay) for lay in small[M]]
        if (K, N, fused) in ROWS2_NARROW:
            M2, M3 = rows2_big_rows(n_cu)
            out += [("stat", K, N, fused, 0, M2, "wave"), ("stat", K, N, fused, 0, M3, "wave")]
    for K, N in ROWS2_PLAIN:
        out += [("plain", K, N, False, 0, M, "one") for M in ROWS2_SMALL_M]
    for K, N, cols in ROWS2_SCAT:
        out += [("scat", K, N, False, cols, M, "one") for M in (33, 600)]
    return out


def tn2_rows(N, K, n_cu):
    """the row counts of a tn2 shape: 1, SR - 1, SR, SR + 1; below gx0 * SR (a partial last workgroup); above it by one step (rows per
    workgroup double and the trailing workgroups have no rows); two steps for every workgroup with a partial last one"""
    gx0 = min(p[0] for p in tn2_plan(1 << 30, N, K, n_cu))
    SR = 8 // (min(256, N) // 32) * 32
    return (1, SR - 1, SR, SR + 1, gx0 * SR - SR // 2 - 3, (gx0 + 1) * SR + 5, 2 * gx0 * SR - 5)


def paths_reached(n_cu):
    """the launcher paths the case lists reach, by name (the CPU tier asserts the full set at 256 CUs)"""
    got = set()
    for kind, K, N, fused, cols, M, lay in rows2_cases(n_cu):
        for ar in ARITHS:
            tp, grid, rpw = rows2_plan(M, N, K, ar, fused, n_cu)
            tiles = rpw // 32
            got.add(f"rows2 tp={tp} arith={ar}")
            got.add("rows2 tiles/wave " + ("1" if tiles == 1 else "2" if tiles == 2 else ">=3"))
            got.add("rows2 passes " + ("1" if N // 32 <= tp else ">1"))
            if N // 32 % tp:
                got.add("rows2 last pass partly past N")
            if M % 32:
                got.add("rows2 ragged last tile")
            if grid * 8 * rpw - M >= rpw:
                got.add("rows2 waves without rows")
            if kind == "stat":
                sizes = cell_layout(M, lay, rpw)
                cuts = np.cumsum(sizes)[:-1]
                for b in cuts:
                    if b % 32:
                        got.add("rows2 boundary inside a tile")
                        continue
                    got.add("rows2 boundary on a tile boundary")
                    got.add("rows2 boundary between two tiles of one wave" if b % rpw else "rows2 boundary between two waves")
                if len(sizes) == 1:
                    got.add("rows2 one cell")
                for s in (2, 31, 32, 33):
                    if s in sizes[:-1]:
                        got.add(f"rows2 cell of {s} rows")
            if fused:
                got.add("rows2 fused")
            if kind == "scat":
                got.add("rows2 scattered")
    for N, K, k_real, fused in TN2_SHAPES:
        for M in tn2_rows(N, K, n_cu):
            plan = tn2_plan(M, N, K, n_cu)
            if len(plan) == 2:
                got.add("tn2 narrower last block as its own launch")
            for gx, gy, gz, kt, rpw, SR in plan:
                got.add(f"tn2 nt={min(256, N) // 32} kt={kt} fused={fused}")
                if gz > 1:
                    got.add("tn2 several k blocks (db from the first only)")
                if gy > 1:
                    got.add("tn2 several n blocks")
                if (gx - 1) * rpw >= M:
                    got.add("tn2 trailing workgroups without rows")
                if rpw >= 2 * SR and M > (gx - 1) * rpw and (M - (gx - 1) * rpw) % SR and M >= gx * rpw - SR:
                    got.add("tn2 two or more steps, partial last")
                if M < SR:
                    got.add("tn2 one partial step")
                if k_real < K:
                    got.add("tn2 k_real < K")
    return got


PATHS_AT_256 = {
    "rows2 tiles/wave 1", "rows2 tiles/wave 2", "rows2 tiles/wave >=3", "rows2 passes 1", "rows2 passes >1", "rows2 last pass partly past N",
    "rows2 ragged last tile", "rows2 waves without rows", "rows2 boundary inside a tile", "rows2 boundary between two tiles of one wave",
    "rows2 boundary between two waves", "rows2 boundary on a tile boundary", "rows2 one cell", "rows2 cell of 2 rows", "rows2 cell of 31 rows",
    "rows2 cell of 32 rows", "rows2 cell of 33 rows", "rows2 fused", "rows2 scattered",
    "tn2 narrower last block as its own launch", "tn2 several k blocks (db from the first only)", "tn2 several n blocks",
    "tn2 trailing workgroups without rows", "tn2 two or more steps, partial last", "tn2 one partial step", "tn2 k_real < K",
    "tn2 nt=2 kt=1 fused=True", "tn2 nt=4 kt=4 fused=True", "tn2 nt=8 kt=4 fused=True", "tn2 nt=1 kt=1 fused=False",
    "tn2 nt=4 kt=3 fused=False", "tn2 nt=8 kt=3 fused=False", "tn2 nt=8 kt=2 fused=False", "tn2 nt=8 kt=4 fused=False",
} | {f"rows2 tp={tp} arith={ar}" for ar, tps in ((0, (1, 2, 3, 4)), (1, (1, 2, 3, 4, 6, 8)), (2, (1, 2, 3, 4))) for tp in tps}


# ---------------------------------------------------------------------------------------------------------------------------
# conditioning: discrete decisions made unambiguous
# ---------------------------------------------------------------------------------------------------------------------------
def scale_table(seed, n_cells, K):
    """an rg = rstd * gamma table [n_cells][K]: both signs, 0.5 <= |rg| (the inputs can only be conditioned through a scale that is
    not ~0: a BatchNorm weight of 1e-3 leaves the operand at beta whatever the input)"""
    g = gauss(seed, n_cells, K)
    return f32(np.where(gauss(seed + (1,), n_cells, K) < -1.0, -1.0, 1.0) * (0.5 + np.abs(g)))


def fused_pre(A, mean, rg, beta, row_cell):
    """(pre, mag): (A - mean) rg + beta per element and |A - mean| |rg| + |beta|, tables [cell][K]"""
    d = A - mean[row_cell]
    return d * rg[row_cell] + beta, np.abs(d) * np.abs(rg[row_cell]) + np.abs(beta)


def operand_ambiguous(pre, mag, ar):
    """True where the ReLU of two float32 values within 4 u mag of pre could reach the product as operands further apart than FUSED_COEF u mag:
    never with exact operands; with bf16 where a rounding tie lies inside that band (the operand is then THE SAME for both); with
    split-bf16 where hi could round either way, or hi + lo — a step function of v, with steps up to 2^-17 |v| — moves by more than 16 u mag
    across the band (a step of lo below the band's own width cannot be conditioned away and is inside the 16)"""
    if ar == arith.EXACT:
        return np.zeros(pre.shape, dtype=bool)
    lo, hi = np.maximum(pre - 4 * U * mag, 0.0), np.maximum(pre + 4 * U * mag, 0.0)
    if ar == arith.BF16:
        return arith.bf16_rne(lo) != arith.bf16_rne(hi)
    (h1, l1), (h2, l2) = arith.split_bf16(lo), arith.split_bf16(hi)
    # (hi must not flip either: lo would change sign with it, and with lo the dropped lo * lo term — 2^-17 |a| |b| in one step)
    return (h1 != h2) | (np.abs((h2 + l2) - (h1 + l1)) > 16 * U * mag)


FUSED_COEF = {arith.EXACT: 2.0, arith.BF16: 2.0, arith.SPLIT: 16.0}


def step_away(x, direction, ar, steps=1):
    """x moved ``steps`` times by about one bf16 step (arith 1: the tensor is stored as bf16) or 64 float32 ulps, in ``direction`` (+-1)"""
    x32 = np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)
    size = np.maximum(np.abs(x32), 2.0 ** -6)  # (the inputs are O(1): an element near zero still moves)
    if ar == arith.BF16:
        return arith.bf16_rne(x32 + direction * steps * (2.0 ** -7) * size)
    return (x32 + direction * steps * 64 * (2.0 ** -23) * size).astype(F32).astype(np.float64)


def _steps(r, n, ar):
    """how far round r of a conditioning loop moves its n elements: 1 .. 3 bf16 steps, or a random 1 .. 255 times 64 float32 ulps (a
    fixed stride can fall in step with the grid it is meant to leave)"""
    return np.random.default_rng((SEED, 99, r)).integers(1, 4 if ar == arith.BF16 else 256, size=n).astype(np.float64)


def fused_band(mag):
    return 8 * U * mag


def fused_ambiguous(A, mean, rg, beta, row_cell, ar):
    """elements whose fused value relu(pre) could reach the product as two different operands, or whose ReLU sign is in doubt"""
    pre, mag = fused_pre(A, mean, rg, beta, row_cell)
    band = fused_band(mag)
    near_zero = np.abs(pre) <= band  # the ReLU sign (needed where the sign is recomputed from y; harmless elsewhere)
    return near_zero | operand_ambiguous(pre, mag, ar)


def condition_fused(A, mean, rg, beta, row_cell, ar, rounds=60, sign_only=False):
    """A with every element whose fused value sits within 8 u (|A - mean| |rg| + |beta|) of zero or (unless sign_only) on an
    operand-rounding step moved off it, a few grid steps of A's storage type at a time (one direction only: no way back onto the
    step it left). Returns the new A (exact values of the storage type). One full pass, then only the elements still in doubt."""
    A = store(A, ar).copy()
    pre, mag = fused_pre(A, mean, rg, beta, row_cell)
    bad = np.abs(pre) <= fused_band(mag)
    if not sign_only:
        bad |= operand_ambiguous(pre, mag, ar)
    rows, cols = np.nonzero(bad)
    for r in range(rounds):
        if len(rows) == 0:
            return A
        A[rows, cols] = step_away(A[rows, cols], 1.0, ar, steps=_steps(r, len(rows), ar))
        cell = row_cell[rows]
        d = A[rows, cols] - mean[cell, cols]
        pre, mag = d * rg[cell, cols] + beta[cols], np.abs(d) * np.abs(rg[cell, cols]) + np.abs(beta[cols])
        bad = np.abs(pre) <= fused_band(mag)
        if not sign_only:
            bad |= operand_ambiguous(pre, mag, ar)
        rows, cols = rows[bad], cols[bad]
    raise AssertionError("condition_fused did not converge")


# ---------------------------------------------------------------------------------------------------------------------------
# rows2: C = f(A) W^T + bias, BatchNorm sums, scattered output
# ---------------------------------------------------------------------------------------------------------------------------
class Rows2Case:
    def __init__(self, kind, K, N, fused, cols, M, layout, ar, n_cu):
        self.kind, self.K, self.N, self.fused, self.cols, self.M, self.layout, self.ar = kind, K, N, fused, cols, M, layout, ar
        seed = (SEED, 1, K, N, M, int(fused))
        self.tp, self.grid, self.rpw = rows2_plan(M, N, K, ar, fused, n_cu)
        self.A = store(gauss(seed + (0,), M, K), ar)
        self.W = gauss(seed + (1,), N, K)
        self.bias = None if kind == "scat" else gauss(seed + (2,), N)
        self.row_cell = self.sizes = None
        self.n_cells = 0
        if kind == "stat":
            self.sizes = cell_layout(M, layout, self.rpw)
            self.row_cell = sizes_to_row_cell(self.sizes)
            self.n_cells = len(self.sizes)
            self.acc0 = gauss(seed + (3,), self.n_cells, 2, 1024)
        if fused:
            self.mean = 0.5 * gauss(seed + (4,), self.n_cells, K)
            self.rg = scale_table(seed + (5,), self.n_cells, K)
            self.beta = f32(0.5 * gauss(seed + (6,), K))
            self.mean = f32(self.mean)
            self.A = condition_fused(self.A, self.mean, self.rg, self.beta, self.row_cell, ar)
        if kind == "scat":
            # multiplicities 1 .. 33 per source row, in a shuffled order
            mult = []
            while sum(mult) < M:
                mult.append(min(len(mult) % 33 + 1, M - sum(mult)))
            self.scat_rows = len(mult) + 3  # (three source rows nobody points at)
            src = np.repeat(np.arange(len(mult)), mult)
            self.scat_src = np.random.default_rng(seed).permutation(src).astype(np.int32)
            self.dst0 = gauss(seed + (7,), self.scat_rows, cols)

    def operand(self):
        """(f(A) float64, magnitude of the fused expression or None)"""
        if not self.fused:
            return self.A, None
        pre, mag = fused_pre(self.A, self.mean, self.rg, self.beta, self.row_cell)
        return np.maximum(pre, 0.0), mag


def rows2_reference(c, product=None):
    """{name: (ref, tol)}: C (as stored), acc [n_cells][2][N] — or dst for the scattered kind. ``product``: the arithmetic of the
    product (default: the case's own; the CPU tier's wrong arithmetics)"""
    ar = c.ar
    Aop, mag = c.operand()
    prod = arith.product(Aop, c.W.T, ar if product is None else product)
    absw = np.abs(c.W).T
    ref = prod if c.bias is None else prod + c.bias
    tol = FACTOR * (c.K + 8) * U * (np.abs(Aop) @ absw + (0.0 if c.bias is None else np.abs(c.bias)))
    if c.fused:
        tol = tol + FUSED_COEF[ar] * U * (mag @ absw)
    out = {}
    if c.kind == "scat":
        v, t = ref[:, :c.cols], tol[:, :c.cols]
        dst, dtol, mult, mag_s = c.dst0.copy(), np.zeros_like(c.dst0), np.zeros(c.scat_rows), np.abs(c.dst0)
        np.add.at(dst, c.scat_src, v)
        np.add.at(dtol, c.scat_src, t)
        np.add.at(mag_s, c.scat_src, np.abs(v))
        np.add.at(mult, c.scat_src, 1.0)
        out["dst"] = (dst, dtol + (mult[:, None] + 8) * U * mag_s)
        return out
    out["C"] = stored(ref, tol, ar)
    if c.kind == "stat":
        out["acc"] = stat_sums(ref, tol, c.row_cell, c.n_cells, c.acc0[:, :, :c.N])
    return out


def stored(ref, tol, ar):
    """(ref, tol) of a value written to an edge-row tensor"""
    if ar == arith.BF16:
        return ref, tol + 2.0 ** -8 * (np.abs(ref) + tol)
    return ref, tol


def stat_sums(C, tol, row_cell, n_cells, acc0=None):
    """(ref, tol) [n_cells][2][N] of S1 = sum C and S2 = sum C^2 over the rows of every cell (+ acc0)"""
    N = C.shape[1]
    ref, t = np.zeros((n_cells, 2, N)), np.zeros((n_cells, 2, N))
    for cell in range(n_cells):
        rows = row_cell == cell
        n = int(rows.sum())
        c, e = C[rows], tol[rows]
        ref[cell, 0], ref[cell, 1] = c.sum(axis=0), (c * c).sum(axis=0)
        t[cell, 0] = FACTOR * (n + 8) * U * np.abs(c).sum(axis=0) + e.sum(axis=0)
        t[cell, 1] = FACTOR * (n + 8) * U * (c * c).sum(axis=0) + (2 * np.abs(c) * e + e * e).sum(axis=0)
    if acc0 is not None:
        ref, t = ref + acc0, t + 2.0 ** -50 * np.abs(acc0)
    return ref, t


def rows2_restatement(c, n_cu_waves=None, mutant=None):
    """float32 numpy restatement of rows2_kernel with its wave / tile structure: the product per 32-row tile, the per-wave running sums
    flushed when the cell changes, straddling and ragged tiles element-wise. mutant: straddle_first (a straddling tile's sums credited to
    its first cell) | no_flush (a wave's running sums not flushed when the cell changes between two of its tiles) | scat_keep_one"""
    ar = c.ar
    Aop, _ = c.operand()
    if c.fused:  # the float32 fused expression
        d = (c.A.astype(F32) - c.mean.astype(F32)[c.row_cell]).astype(F32)
        Aop = np.maximum((d.astype(np.float64) * c.rg[c.row_cell] + c.beta).astype(F32), F32(0)).astype(np.float64)
    C = TB.f32_matmul(Aop, c.W.T, ar).astype(F32)
    if c.bias is not None:
        C = (C + c.bias.astype(F32)).astype(F32)
    out = {}
    if c.kind == "scat":
        dst = c.dst0.astype(F32).copy()
        if mutant == "scat_keep_one":
            dst[c.scat_src] += C[:, :c.cols]  # (numpy's fancy-index +=: one of the rows sharing a source survives)
        else:
            np.add.at(dst, c.scat_src, C[:, :c.cols])
        out["dst"] = dst.astype(np.float64)
        return out
    out["C"] = store(C.astype(np.float64), ar)
    if c.kind == "stat":
        acc = c.acc0[:, :, :c.N].copy()
        M, rpw = c.M, c.rpw
        for w0 in range(0, M, rpw):
            cur, run1, run2 = -1, np.zeros(c.N, F32), np.zeros(c.N, F32)

            def flush():
                nonlocal run1, run2
                if cur >= 0:
                    acc[cur, 0] += run1.astype(np.float64)
                    acc[cur, 1] += run2.astype(np.float64)
                    run1, run2 = np.zeros(c.N, F32), np.zeros(c.N, F32)

            for m0 in range(w0, min(M, w0 + rpw), 32):
                rows = slice(m0, min(M, m0 + 32))
                cells = c.row_cell[rows]
                uniform, full = cells[0] == cells[-1], m0 + 32 <= M
                if uniform and cells[0] != cur:
                    if mutant != "no_flush":
                        flush()
                    cur = int(cells[0])
                v = C[rows]
                if uniform and full:
                    run1 = (run1 + v.sum(axis=0, dtype=F32)).astype(F32)
                    run2 = (run2 + (v * v).sum(axis=0, dtype=F32)).astype(F32)
                else:
                    tgt = np.full(len(cells), cells[0]) if mutant == "straddle_first" else cells
                    np.add.at(acc[:, 0], tgt, v.astype(np.float64))
                    np.add.at(acc[:, 1], tgt, v.astype(np.float64) ** 2)
            flush()
        out["acc"] = acc
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# tn2: dW += dY^T f(X), db += colsum dY
# ---------------------------------------------------------------------------------------------------------------------------
class Tn2Case:
    def __init__(self, N, K, k_real, fused, M, ar):
        self.N, self.K, self.k_real, self.fused, self.M, self.ar = N, K, k_real, fused, M, ar
        seed = (SEED, 2, N, K, M)
        self.dY = store(gauss(seed + (0,), M, N), ar)
        # The bound of a sum over M rows grows like M^2 u: at tens of thousands of rows it is wider than what a handful of rows
        # contribute, and a dropped partial last step (the M mod SR trailing rows: rows_per_wg is a multiple of SR) would pass.
        # Those rows carry 2^10 times the gradient (an exact scaling), so that they weigh as much as all the others together.
        SR = 8 // (min(256, N) // 32) * 32
        if M > 4 * SR and M % SR:
            self.dY[M - M % SR:] *= 1024.0
        self.X = store(gauss(seed + (1,), M, K), ar)
        self.dW0, self.db0 = gauss(seed + (2,), N, k_real), gauss(seed + (3,), N)
        self.row_cell, self.n_cells = None, 0
        if fused:
            sizes = [M] if M < 6 else [M // 3, M // 3, M - 2 * (M // 3)]
            self.row_cell, self.n_cells = sizes_to_row_cell(sizes), len(sizes)
            self.mean = f32(0.5 * gauss(seed + (4,), self.n_cells, K))
            self.rg = scale_table(seed + (5,), self.n_cells, K)
            self.beta = f32(0.5 * gauss(seed + (6,), K))
            self.X = condition_fused(self.X, self.mean, self.rg, self.beta, self.row_cell, ar)

    def operand(self):
        if not self.fused:
            return self.X, None
        pre, mag = fused_pre(self.X, self.mean, self.rg, self.beta, self.row_cell)
        return np.maximum(pre, 0.0), mag


def tn2_reference(c, product=None):
    """{dW: (ref, tol) [N][k_real], db: (ref, tol)}"""
    Xop, mag = c.operand()
    kr = c.k_real
    prod = arith.product(c.dY.T, Xop[:, :kr], c.ar if product is None else product)
    absy = np.abs(c.dY).T
    tol = FACTOR * (c.M + 8) * U * (absy @ np.abs(Xop[:, :kr]) + np.abs(c.dW0))
    if c.fused:
        tol = tol + FUSED_COEF[c.ar] * U * (absy @ mag[:, :kr])
    return {"dW": (c.dW0 + prod, tol), "db": TB.colsum(c.dY, c.db0)}


def tn2_restatement(c, n_cu, mutant=None):
    """float32 restatement per workgroup chunk. mutant: drop_partial (the partial last step of a row chunk is dropped) | db_every_block
    (db added by every k block) | write_pad (the padding columns k >= k_real are written: they land in the next row of dW)"""
    Xop, _ = c.operand()
    if c.fused:
        d = (c.X.astype(F32) - c.mean.astype(F32)[c.row_cell]).astype(F32)
        Xop = np.maximum((d.astype(np.float64) * c.rg[c.row_cell] + c.beta).astype(F32), F32(0)).astype(np.float64)
    dW = np.zeros((c.N, c.K), F32)
    db = np.zeros(c.N, F32)
    plans = tn2_plan(c.M, c.N, c.K, n_cu)
    k0 = 0
    for part, (gx, gy, gz, kt, rpw, SR) in enumerate(plans):
        kcols = slice(k0, k0 + 32 * kt * gz)
        for m_lo in range(0, c.M, rpw):
            m_hi = min(c.M, m_lo + rpw)
            if mutant == "drop_partial" and (m_hi - m_lo) % SR:
                m_hi = m_lo + (m_hi - m_lo) // SR * SR
            if m_hi <= m_lo:
                continue
            dW[:, kcols] += TB.f32_matmul(c.dY[m_lo:m_hi].T, Xop[m_lo:m_hi, kcols], c.ar).astype(F32)
            if part == 0:
                reps = gz if mutant == "db_every_block" else 1
                db += reps * c.dY[m_lo:m_hi].astype(F32).sum(axis=0, dtype=F32)
        k0 += 32 * kt * gz
    flat = np.concatenate([c.dW0.astype(F32).ravel(), np.zeros(c.K, F32)])  # dW is [N][k_real] in memory
    for n in range(c.N):
        cols = c.K if mutant == "write_pad" else c.k_real
        flat[n * c.k_real:n * c.k_real + cols] += dW[n, :cols]
    out = flat[:c.N * c.k_real].reshape(c.N, c.k_real)
    return {"dW": out.astype(np.float64), "db": (c.db0.astype(F32) + db).astype(np.float64)}


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm tables: the forward's statistics, the backward's coefficients
# ---------------------------------------------------------------------------------------------------------------------------
def bn_forward_tables(S, S_tol, cnt, gamma, rm0, rv0, mutant=None):
    """From the sums S [n_cells][2][C] (and their bounds): {mean, rstd, rg, run_mean, run_var: (ref, tol)} as pt_bn_finalize_kernel
    computes them — biased variance for the normalisation, unbiased for running_var, one momentum update per cell in cell order.
    Own float32 roundings: mean 1 (the cast); rstd 4 (cast, + eps, sqrt, divide); rg 5; a momentum update 3 per cell.
    mutant: biased_running_var | one_update_per_batch"""
    n = np.asarray(cnt, dtype=np.float64)[:, None]
    mean = S[:, 0] / n
    var = np.maximum(S[:, 1] / n - mean * mean, 0.0)
    d_mean = S_tol[:, 0] / n
    d_var = S_tol[:, 1] / n + 2 * np.abs(mean) * d_mean + d_mean * d_mean
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    d_rstd = 0.5 * rstd ** 3 * d_var
    out = {"mean": (mean, 2 * d_mean + 4 * U * np.abs(mean)),
           "rstd": (rstd, 2 * d_rstd + 4 * U * rstd),
           "rg": (rstd * gamma, 2 * d_rstd * np.abs(gamma) + 5 * U * np.abs(rstd * gamma))}
    unb = n / np.maximum(n - 1.0, 1.0)
    vu, d_vu = (var if mutant == "biased_running_var" else var * unb), d_var * unb
    rm, rv = rm0.copy(), rv0.copy()
    e_m, e_v = np.zeros_like(rm0), np.zeros_like(rv0)
    if mutant == "one_update_per_batch":
        w = n / n.sum()
        rm, rv = ONE_MINUS_MOM * rm + MOM * (mean * w).sum(axis=0), ONE_MINUS_MOM * rv + MOM * (vu * w).sum(axis=0)
    else:
        for cell in range(S.shape[0]):
            e_m = ONE_MINUS_MOM * e_m + MOM * d_mean[cell] + 3 * U * (np.abs(ONE_MINUS_MOM * rm) + np.abs(MOM * mean[cell]))
            e_v = ONE_MINUS_MOM * e_v + MOM * d_vu[cell] + 3 * U * (np.abs(ONE_MINUS_MOM * rv) + np.abs(MOM * vu[cell]))
            rm = ONE_MINUS_MOM * rm + MOM * mean[cell]
            rv = ONE_MINUS_MOM * rv + MOM * vu[cell]
    out["run_mean"] = (rm, 2 * e_m + 4 * U * np.abs(rm))
    out["run_var"] = (rv, 2 * e_v + 4 * U * np.abs(rv))
    return out


class BlockFwdCase:
    """one get_mlp layer through pn_block_fwd: the product of a Rows2Case (statistics from zero), its per-cell tables and the running
    statistics from non-trivial prior values"""

    def __init__(self, K, C, fused, sizes, ar, n_cu):
        self.prod = p = Rows2Case("stat", K, C, fused, 0, int(sum(sizes)), list(sizes), ar, n_cu)
        p.acc0 = np.zeros_like(p.acc0)
        self.K, self.C, self.fused, self.ar, self.E, self.n_cells = K, C, fused, ar, p.M, p.n_cells
        self.cnt = np.asarray(sizes, dtype=np.int32)
        seed = (SEED, 6, K, C, p.M, p.n_cells)
        self.gamma, self.beta = f32(1.0 + 0.3 * gauss(seed + (0,), C)), f32(0.3 * gauss(seed + (1,), C))
        self.rm0, self.rv0 = gauss(seed + (2,), C), f32(0.5 + np.abs(gauss(seed + (3,), C)))


def block_fwd_reference(c, mutant=None):
    """{y, mean, rstd, rg, run_mean, run_var: (ref, tol)}"""
    r = rows2_reference(c.prod)
    out = bn_forward_tables(r["acc"][0], r["acc"][1], c.cnt, c.gamma, c.rm0, c.rv0, mutant)
    out["y"] = r["C"]
    return out


def bn_apply_reference(y, mean, rstd, gamma, beta, row_cell, ar):
    """(ref, tol) of a = relu((y - mean) rstd gamma + beta) from the tensors the apply kernel READS (the test hands it the kernel's own
    y, mean and rstd: no error compounds). Four float32 roundings."""
    d = y - mean[row_cell]
    s = rstd[row_cell] * gamma
    pre = d * s + beta
    return stored(np.maximum(pre, 0.0), 4 * U * (np.abs(d * s) + np.abs(beta)), ar)


def bn_backward_tables(S, S_tol, cnt, gamma, rstd, dgamma0, dbeta0, mutant=None):
    """{k1, k2 [n_cells][C], dgamma, dbeta [C]: (ref, tol)} from S1 = sum dv, S2 = sum dv xhat (pt_bn_bwd_finalize_kernel):
    k1 = gamma rstd S1 / n, k2 = gamma rstd^2 S2 / n (biased: n, not n - 1). Own roundings: k1 4, k2 5; dbeta / dgamma 2.
    mutant: n_minus_1"""
    n = np.asarray(cnt, dtype=np.float64)[:, None]
    if mutant == "n_minus_1":
        n = n - 1.0
    g = gamma * rstd / n
    k1, k2 = g * S[:, 0], g * rstd * S[:, 1]
    return {"k1": (k1, 2 * np.abs(g) * S_tol[:, 0] + 4 * U * np.abs(k1)),
            "k2": (k2, 2 * np.abs(g * rstd) * S_tol[:, 1] + 5 * U * np.abs(k2)),
            "dbeta": (dbeta0 + S[:, 0].sum(axis=0), 2 * S_tol[:, 0].sum(axis=0) + 4 * U * (np.abs(S[:, 0]).sum(axis=0) + np.abs(dbeta0))),
            "dgamma": (dgamma0 + S[:, 1].sum(axis=0), 2 * S_tol[:, 1].sum(axis=0) + 4 * U * (np.abs(S[:, 1]).sum(axis=0) + np.abs(dgamma0)))}


def bn_backward_sums(dv, y, mean, rstd, cell_of_term, n_cells):
    """(S, S_tol) [n_cells][2][C]: S1 = sum dv, S2 = sum dv (y - mean) rstd over the terms of every cell; a term of S2 takes three
    float32 roundings before it is summed (n + 8 covers n - 1 + 3)"""
    C = dv.shape[1]
    t2 = dv * (y - mean[cell_of_term]) * rstd[cell_of_term]
    S, T = np.zeros((n_cells, 2, C)), np.zeros((n_cells, 2, C))
    for cell in range(n_cells):
        sel = cell_of_term == cell
        n = int(sel.sum())
        S[cell, 0], S[cell, 1] = dv[sel].sum(axis=0), t2[sel].sum(axis=0)
        T[cell, 0] = FACTOR * (n + 8) * U * np.abs(dv[sel]).sum(axis=0)
        T[cell, 1] = FACTOR * (n + 8) * U * np.abs(t2[sel]).sum(axis=0)
    return S, T


def bn_backward_elementwise(dv, y, mean, rstd, gamma, tabs, row_cell, ar):
    """(ref, tol) of dx = k0 dv - k1 - (y - mean) k2, k0 = gamma rstd, as stored. Own roundings: at most 4 on any term."""
    (k1, t1), (k2, t2) = tabs["k1"], tabs["k2"]
    d = y - mean[row_cell]
    a, b, c = gamma * rstd[row_cell] * dv, k1[row_cell], d * k2[row_cell]
    tol = 2 * (t1[row_cell] + np.abs(d) * t2[row_cell]) + 4 * U * (np.abs(a) + np.abs(b) + np.abs(c))
    return stored(a - b - c, tol, ar)


class BnRowsCase:
    """the rows form of pn_block_bwd: d, y, a (or rg in its place) [E][C], per-cell tables"""

    def __init__(self, C, sizes, stored_a, ar):
        self.C, self.sizes, self.stored_a, self.ar = C, list(sizes), stored_a, ar
        self.E, self.n_cells = int(sum(sizes)), len(sizes)
        seed = (SEED, 3, C, self.E, self.n_cells, int(stored_a))
        self.row_cell = sizes_to_row_cell(sizes)
        self.cnt = np.asarray(sizes, dtype=np.int32)
        self.d = store(gauss(seed + (0,), self.E, C), ar)
        y = gauss(seed + (1,), self.E, C)
        self.mean = f32(0.3 * gauss(seed + (2,), self.n_cells, C))
        self.rstd = f32(0.5 + np.abs(gauss(seed + (3,), self.n_cells, C)))
        self.gamma, self.beta = f32(1.0 + 0.3 * gauss(seed + (4,), C)), f32(0.3 * gauss(seed + (5,), C))
        self.rg = f32(self.rstd * self.gamma)
        self.dgamma0, self.dbeta0 = gauss(seed + (6,), C), gauss(seed + (7,), C)
        if stored_a:
            self.y = store(y, ar)
            pre, _ = fused_pre(self.y, self.mean, self.rg, self.beta, self.row_cell)
            a = store(np.maximum(pre, 0.0), ar)
            a[::5, ::3] = 0.0  # planted exact zeros under a non-zero incoming gradient: `a > 0`, not `a >= 0`
            self.a = a
            self.mask = a > 0
        else:
            self.y = condition_sign(store(y, ar), self.mean, self.rg, self.beta, self.row_cell, ar)
            pre, _ = fused_pre(self.y, self.mean, self.rg, self.beta, self.row_cell)
            self.a, self.mask = None, pre > 0


def condition_sign(y, mean, rg, beta, row_cell, ar):
    """y with every element whose pre-activation (y - mean) rg + beta lies within 8 u (|y - mean| |rg| + |beta|) of zero moved away"""
    return condition_fused(y, mean, rg, beta, row_cell, ar, sign_only=True)


def bn_rows_reference(c, mutant=None):
    """{d, k1, k2, dgamma, dbeta: (ref, tol)} of the rows form. mutant: n_minus_1 | ge_mask (`>=` for `>` in the stored-a mask)"""
    mask = (c.a >= 0) if (mutant == "ge_mask" and c.stored_a) else c.mask
    dv = np.where(mask, c.d, 0.0)
    S, T = bn_backward_sums(dv, c.y, c.mean, c.rstd, c.row_cell, c.n_cells)
    out = bn_backward_tables(S, T, c.cnt, c.gamma, c.rstd, c.dgamma0, c.dbeta0, "n_minus_1" if mutant == "n_minus_1" else None)
    out["d"] = bn_backward_elementwise(dv, c.y, c.mean, c.rstd, c.gamma, out, c.row_cell, c.ar)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# groups: segmax and the groups form of the backward
# ---------------------------------------------------------------------------------------------------------------------------
def group_sizes(G, seed, lo=1, hi=33):
    """G group sizes that run through lo .. hi (every size occurs when G >= hi - lo + 1), shuffled"""
    s = np.arange(G) % (hi - lo + 1) + lo
    return np.random.default_rng((SEED, 4, G, seed)).permutation(s)


class GroupCase:
    """y [E][C] in groups of 1 .. 33 rows, nd groups per object, objects in cells. Planted: a group of exact duplicate rows (the first
    must win), a group whose every pre-activation is negative (xout 0, arg its first row, no gradient), groups of one row."""

    def __init__(self, C, n_obj, nd, n_cells, ar, planted=True):
        self.C, self.n_obj, self.nd, self.n_cells, self.ar = C, n_obj, nd, n_cells, ar
        self.G = G = n_obj * nd
        seed = (SEED, 5, C, n_obj, nd, n_cells)
        sizes = group_sizes(G, C)
        if G == 1:
            sizes = np.array([7])
        self.goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.E = E = int(self.goff[-1])
        self.cell_of_obj = (np.arange(n_obj) * n_cells // n_obj).astype(np.int32)
        self.row_group = np.repeat(np.arange(G), sizes).astype(np.int32)
        self.row_cell = self.cell_of_obj[self.row_group // nd]
        self.cnt = np.bincount(self.row_cell, minlength=n_cells).astype(np.int32)
        assert (self.cnt >= 2).all()
        self.mean = f32(0.3 * gauss(seed + (2,), n_cells, C))
        self.rstd = f32(0.5 + np.abs(gauss(seed + (3,), n_cells, C)))
        self.gamma, self.beta = f32(1.0 + 0.3 * gauss(seed + (4,), C)), f32(0.3 * gauss(seed + (5,), C))
        y = store(gauss(seed + (1,), E, C), ar)
        self.dup = self.neg = None
        big = np.flatnonzero(sizes >= 3)
        if planted and len(big) >= 2:
            self.dup, self.neg = int(big[0]), int(big[-1])
            r = slice(self.goff[self.dup], self.goff[self.dup + 1])
            y[r] = y[r.start]
            r = slice(self.goff[self.neg], self.goff[self.neg + 1])
            s = self.rstd[self.row_cell[r]] * self.gamma
            # every pre-activation of the group at -1 or below: y = mean - sign(s) (1 + |beta|) / |s|, rounded away from the mean
            y[r] = store(self.mean[self.row_cell[r]] - np.sign(s) * (1.5 + np.abs(self.beta) + np.abs(y[r])) / np.abs(s), ar)
        self.y = condition_groups(y, self, ar)
        self.dxout = gauss(seed + (6,), G, C)
        self.dgamma0, self.dbeta0 = gauss(seed + (7,), C), gauss(seed + (8,), C)

    def pre(self, y=None):
        y = self.y if y is None else y
        d = y - self.mean[self.row_cell]
        s = self.rstd[self.row_cell] * self.gamma
        return d * s + self.beta, np.abs(d * s) + np.abs(self.beta)


def group_decisions(c, y=None):
    """bool [E][C]: rows whose ReLU sign, or whose rank against their group's maximum, is in doubt within 8 u mag. Rows bit-equal to
    the maximum tie and the first of them wins on both sides — provided they hold the same y (duplicate rows) or all clamp to 0."""
    y = c.y if y is None else y
    pre, mag = c.pre(y)
    band = fused_band(mag)
    v = np.maximum(pre, 0.0)
    starts = c.goff[:-1]
    vmax = np.maximum.reduceat(v, starts, axis=0)[c.row_group]
    tie = v == vmax
    bad = np.abs(pre) <= band
    bandmax = np.maximum.reduceat(np.where(tie, band, 0.0), starts, axis=0)[c.row_group]
    bad |= ~tie & (vmax - v <= band + bandmax)  # a lower row within the band of the maximum (its own band or the maximum's)
    y_hi = np.maximum.reduceat(np.where(tie, y, -np.inf), starts, axis=0)[c.row_group]
    y_lo = np.minimum.reduceat(np.where(tie, y, np.inf), starts, axis=0)[c.row_group]
    return bad | (tie & (vmax > 0) & (y_hi != y_lo))


def condition_groups(y, c, ar, rounds=60):
    """y with every row in doubt moved: its pre-activation DOWN — away from the maximum and, if negative, from zero — unless it is a
    small positive one inside the band around zero, which goes up"""
    y = y.copy()
    s = np.sign(c.rstd[c.row_cell] * c.gamma)
    for r in range(rounds):
        bad = group_decisions(c, y)
        if not bad.any():
            return y
        pre, mag = c.pre(y)
        up = (pre > 0) & (pre <= fused_band(mag))
        k = _steps(r, y.size, ar).reshape(y.shape)
        y = np.where(bad, np.where(np.where(up, s, -s) > 0, step_away(y, 1.0, ar, steps=k), step_away(y, -1.0, ar, steps=k)), y)
    raise AssertionError("condition_groups did not converge")


def segmax_reference(c, last_wins=False):
    """xout (ref, tol) [G][C], arg int32 [G][C] (global row, the first maximum), ysel = y at arg (exact)"""
    pre, mag = c.pre()
    v = np.maximum(pre, 0.0)
    G, C = c.G, c.C
    xout, arg, tol = np.zeros((G, C)), np.zeros((G, C), np.int32), np.zeros((G, C))
    for g in range(G):
        lo, hi = int(c.goff[g]), int(c.goff[g + 1])
        blk = v[lo:hi]
        a = (hi - lo - 1 - blk[::-1].argmax(axis=0)) if last_wins else blk.argmax(axis=0)
        arg[g] = lo + a
        xout[g] = blk[a, np.arange(C)]
        tol[g] = 4 * U * mag[lo:hi][a, np.arange(C)]
    ysel = c.y[arg, np.arange(C)[None, :]]
    return {"xout": (xout, tol), "arg": arg, "ysel": ysel}


def bn_groups_reference(c, seg, mutant=None):
    """{d, k1, k2, dgamma, dbeta} of the groups form from the exact forward outputs ``seg`` (arg, ysel, xout as float32)"""
    arg, ysel, xout = seg["arg"], seg["ysel"], f32(seg["xout"][0])
    cell_of_group = c.cell_of_obj[np.arange(c.G) // c.nd]
    dvg = np.where(xout > 0, c.dxout, 0.0)
    S, T = bn_backward_sums(dvg, ysel, c.mean, c.rstd, cell_of_group, c.n_cells)
    out = bn_backward_tables(S, T, c.cnt, c.gamma, c.rstd, c.dgamma0, c.dbeta0, "n_minus_1" if mutant == "n_minus_1" else None)
    pre, _ = c.pre()
    rows = np.arange(c.E)[:, None]
    hit = (arg[c.row_group] == rows) & (pre > 0)
    dv = np.where(hit, c.dxout[c.row_group], 0.0)
    out["d"] = bn_backward_elementwise(dv, c.y, c.mean, c.rstd, c.gamma, out, c.row_cell, c.ar)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# exact kernels: row tables + gather, FPS + ball query, layout
# ---------------------------------------------------------------------------------------------------------------------------
def gather_reference(x_src, pos_src, pos_ctr, src, row_group, cin, kp, ar, prev_centre=False):
    """X [E][kp] = [x_src[src] | float32(pos_src[src] - pos_ctr[row_group]) | 0], as stored (bit-exact: one float32 subtraction).
    prev_centre: the WRONG centre (the previous group's), a negative control"""
    E = len(src)
    X = np.zeros((E, kp))
    X[:, :cin] = x_src[src]
    rel = pos_src[src].astype(F32)
    if pos_ctr is not None:
        g = np.maximum(row_group - 1, 0) if prev_centre else row_group
        rel = (rel - pos_ctr[g].astype(F32)).astype(F32)
    X[:, cin:cin + 3] = rel.astype(np.float64)
    return store(X, ar)


def compact_reference(nbr33, goff, nd, cell_of_obj):
    """(src, row_group, row_cell) of the compacted rows: the valid slots 0 .. count - 1 first, the self-loop edge last"""
    G = nbr33.shape[0]
    valid = nbr33 >= 0
    src = nbr33[valid]
    row_group = np.repeat(np.arange(G), valid.sum(axis=1)).astype(np.int32)
    assert np.array_equal(np.concatenate([[0], np.cumsum(valid.sum(axis=1))]), goff)
    return src.astype(np.int32), row_group, cell_of_obj[row_group // nd].astype(np.int32)


def index_reference(pos, cell_offsets, radius, self_loops):
    """(pos_out f32 [n][nd][3], nbr33 int32 [n nd][33], cnt_g int32 [n nd]) of one level through tests/pointnet_blocks.py's restatement"""
    from tests import pointnet_blocks as PB

    n, ns, _ = pos.shape
    nd = ns // 2
    ctr = PB.centres(pos)
    idx, valid = PB.neighbours(pos, ctr, radius)
    o = np.arange(n)[:, None, None]
    nbr = np.where(valid, o * ns + idx, -1).reshape(n * nd, 32)
    base = np.zeros(n, dtype=np.int64)
    for c in range(len(cell_offsets) - 1):
        base[int(cell_offsets[c]):int(cell_offsets[c + 1])] = int(cell_offsets[c])
    loop = (base[:, None] * ns + (np.arange(n) - base)[:, None] * nd + np.arange(nd)[None, :]).reshape(n * nd, 1)
    nbr33 = np.concatenate([nbr, loop if self_loops else np.full_like(loop, -1)], axis=1).astype(np.int32)
    cnt = (valid.reshape(n * nd, 32).sum(axis=1) + (1 if self_loops else 0)).astype(np.int32)
    return ctr, nbr33, cnt, base.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the dev library
# ---------------------------------------------------------------------------------------------------------------------------
def load_blocks():
    import ctypes as C

    lib = TB.load_blocks()
    p, i, q = C.c_void_p, C.c_int, C.c_int64
    sigs = {
        "t2l_blk_pn_rows2": [p, p, p, p, q, i, i, i, p, p, p, p, i, p, p, p, i, q],
        "t2l_blk_pn_tn2": [p, p, p, p, q, i, i, i, i, p, p, p, p, i, i],
        "t2l_blk_pn_block_fwd": [p, p, q, i, i, i, p, p, p, p, p, p, p, i, p, p, p, p, p, p, p, p, p],
        "t2l_blk_pn_block_bwd": [p, p, p, q, i, i, p, p, p, p, p, p, p, p, p, i, p, p, p, p, p, p, p, p, p, q, i],
        "t2l_blk_pn_segmax": [p, p, q, q, i, i, p, i, p, p, p, p, p, p, p, i],
        "t2l_blk_pn_rows": [i, p, p, q, i, i, p, i, q, p, p, p, p, p, p, q, i, i, p, i],
        "t2l_blk_pn_index": [p, i, i, i, C.c_float, p, i, p, p, p],
        "t2l_blk_pn_layout": [i, p, p, q, i, i, i],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    return lib
