"""Float64 reference and test inputs of the pairwise and hardest ranking losses (training/losses.py:192-217 and :321-355;
include/t2l.h: t2l_ranking_loss). Shared by tests/test_ranking_loss_cpu.py and the GPU tiers; numpy only.

c = im^ . s^T (rows re-normalised), d_i = c_ii, m the margin, B the batch, for i != j:
    hA_ij = m - d_i + c_ij,  hB_ij = m - d_j + c_ij
    pairwise  A = [hA > 0],                     Bm = [hB > 0]
    hardest   A_ij = [j == j1_i][hA_ij > 0],    Bm_ij = [j == j2_i][hB_ij > 0],   j1_i = argmax_j c_ij,  j2_i = argmax_j (c_ij - d_j)
              (both maxima along the row, the lowest column on a tie)
    loss = scale/B * sum (A hA + Bm hB);   G = scale/B * (A + Bm) off the diagonal,  G_ii = -scale/B * (sum_j A_ij + sum_k Bm_ki)
    d im = ((G s^) - im^ * rowdot) / |im|,  rowdot_i = sum_k G_ik c_ik;   d s likewise from G^T.

Conditioning. A float32 cosine carries about 3e-7 of error, so a hinge argument or a top-two gap within that distance of zero is
undecidable in float32: no implementation can be held to the float64 decision there. ``conditioned_inputs`` therefore resamples rows of
``s`` until, in float64, every off-diagonal hinge argument is at least ``COND`` = 1e-5 away from 0 and, in every row, the two largest
positive costs of either direction are at least ``COND`` apart. Nothing is skipped or masked in a test: the inputs are what moves.

The gradient bar ``RANK_T``: |err| <= T * rms(reference tensor) + 1e-9 per element, T = 4 x the worst error of the float32 CPU
evaluation of the torch mirror (text2loc_amd.losses, the reference's own arithmetic) against this float64 reference over every case of
tests/test_gpu_ranking_loss.py; the factor 4 is for the MFMA tiles' other summation order. The measured table is in
profiles/ranking_loss.md (tools/bench_ranking_loss.py --bars prints it)."""
import functools

import numpy as np

KINDS = ("pairwise", "hardest")
SCALES = {"pairwise": 1.0, "hardest": 64.0}  # the reference's: PairwiseRankingLoss has none, HardestRankingLoss(scale=64.0)
COND = 1e-5
MAX_ROUNDS = 20
LOSS_RTOL = 3e-5  # as for the contrastive loss (tests/test_gpu_loss.py)
RANK_T = {"pairwise": 4.5e-5, "hardest": 5.6e-5}  # profiles/ranking_loss.md: 4 x (1.11e-5, 1.39e-5), rounded up

# the conditioned cases of the GPU tier: (B, a, margin)
FUSED_B = (1, 2, 3, 31, 33, 64, 128)
CHAIN_B = (129, 300, 1024)
CASES = tuple((B, a, 0.35) for B in FUSED_B + CHAIN_B for a in (0.45, 0.9)) + ((64, 0.45, 0.2), (64, 0.9, 0.2))


def ranking_loss_ref(im, s, kind, margin, scale=None):
    """(loss, d loss/d im, d loss/d s) in float64 from the formulas above."""
    assert kind in KINDS
    scale = SCALES[kind] if scale is None else scale
    im, s = np.asarray(im, np.float64), np.asarray(s, np.float64)
    B = len(im)
    na, ns = np.linalg.norm(im, axis=1), np.linalg.norm(s, axis=1)
    ih, sh = im / na[:, None], s / ns[:, None]
    c = ih @ sh.T
    d = np.diag(c).copy()
    off = ~np.eye(B, dtype=bool)
    hA, hB = margin - d[:, None] + c, margin - d[None, :] + c
    if kind == "pairwise":
        A, Bm = off & (hA > 0), off & (hB > 0)
    else:
        A, Bm = np.zeros((B, B), bool), np.zeros((B, B), bool)
        if B > 1:
            rows = np.arange(B)
            j1 = np.where(off, c, -np.inf).argmax(axis=1)  # numpy's argmax returns the first maximum: the lowest column
            j2 = np.where(off, c - d[None, :], -np.inf).argmax(axis=1)
            A[rows, j1] = hA[rows, j1] > 0
            Bm[rows, j2] = hB[rows, j2] > 0
    sc = scale / B
    loss = sc * (hA[A].sum() + hB[Bm].sum())
    G = sc * (A.astype(np.float64) + Bm)
    G[np.arange(B), np.arange(B)] = -sc * (A.sum(axis=1) + Bm.sum(axis=0))
    Gc = G * c
    g_im = ((G @ sh) - ih * Gc.sum(axis=1)[:, None]) / na[:, None]
    g_s = ((G.T @ ih) - sh * Gc.sum(axis=0)[:, None]) / ns[:, None]
    return float(loss), g_im, g_s


def conditioning(im, s, margin):
    """(min |off-diagonal hinge argument|, min top-two gap of the positive costs over rows that violate, flagged indices)."""
    im, s = np.asarray(im, np.float64), np.asarray(s, np.float64)
    B = len(im)
    if B == 1:
        return np.inf, np.inf, np.zeros(0, np.int64)
    c = (im / np.linalg.norm(im, axis=1, keepdims=True)) @ (s / np.linalg.norm(s, axis=1, keepdims=True)).T
    d = np.diag(c).copy()
    off = ~np.eye(B, dtype=bool)
    flagged = np.zeros(B, bool)
    min_hinge, min_gap = np.inf, np.inf
    for h in (margin - d[:, None] + c, margin - d[None, :] + c):
        near = off & (np.abs(h) < COND)
        min_hinge = min(min_hinge, float(np.abs(h[off]).min()))
        flagged |= near.any(axis=1) | near.any(axis=0)
        cost = np.where(off, np.maximum(h, 0.0), 0.0)  # the diagonal is a cost of 0, as in the reference
        order = np.argsort(-cost, axis=1, kind="stable")
        rows = np.arange(B)
        top, second = cost[rows, order[:, 0]], cost[rows, order[:, 1]]
        live = top > 0
        gap = np.where(live, top - second, np.inf)
        min_gap = min(min_gap, float(gap.min()))
        close = gap < COND
        flagged |= close
        flagged[order[close, 0]] = True
    return min_hinge, min_gap, np.flatnonzero(flagged)


@functools.lru_cache(maxsize=None)
def conditioned_inputs(B, a, margin=0.35, seed=0):
    """im = 1.7 (a base + noise), s = 0.6 (a base + noise'), float32 [B,256], seeded by (seed, B); rows of s resampled until the
    conditioning holds. a = 0.45: nearly every hinge active, every row violated; a = 0.9: about 11 % active. Returns read-only
    (im, s, rounds)."""
    rng = np.random.default_rng([seed, B])
    base = rng.standard_normal((B, 256))
    im = (1.7 * (a * base + rng.standard_normal((B, 256)))).astype(np.float32)
    s = (0.6 * (a * base + rng.standard_normal((B, 256)))).astype(np.float32)
    rounds = 0
    while True:
        min_hinge, min_gap, flagged = conditioning(im, s, margin)
        if len(flagged) == 0:
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, f"B={B} a={a}: still {len(flagged)} ill-conditioned rows after {MAX_ROUNDS} rounds"
        s[flagged] = (0.6 * (a * base[flagged] + rng.standard_normal((len(flagged), 256)))).astype(np.float32)
    assert min_hinge >= COND and min_gap >= COND, (B, a, min_hinge, min_gap)
    im.setflags(write=False)
    s.setflags(write=False)
    return im, s, rounds


@functools.lru_cache(maxsize=None)
def conditioned_reference(B, a, margin, kind, seed=0):
    """The float64 reference on ``conditioned_inputs(B, a, margin, seed)``, computed once per session and read-only."""
    im, s, _ = conditioned_inputs(B, a, margin, seed)
    loss, g_im, g_s = ranking_loss_ref(im, s, kind, margin)
    g_im.setflags(write=False)
    g_s.setflags(write=False)
    return loss, g_im, g_s


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def grad_errors(got, ref):
    """Worst |err| of a gradient tensor in units of the reference tensor's rms (0 for an all-zero reference met exactly)."""
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    r = rms(ref)
    return err / r if r > 0 else (0.0 if err <= 1e-9 else np.inf)


def assert_grad(got, ref, kind, what):
    bound = RANK_T[kind] * rms(ref) + 1e-9
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert err.max() <= bound, f"{what}: worst element off by {err.max():.3e} > {bound:.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def assert_loss(got, ref, what):
    assert abs(got - ref) <= LOSS_RTOL * max(abs(ref), 1e-30) or (ref == 0.0 and got == 0.0), f"{what}: loss {got!r} vs {ref!r}"


def mirror_float32(im, s, kind, margin):
    """The float32 CPU evaluation of the torch mirror with autograd: what the bars are derived from."""
    import torch

    from text2loc_amd.losses import HardestRankingLoss, PairwiseRankingLoss

    crit = PairwiseRankingLoss(margin) if kind == "pairwise" else HardestRankingLoss(margin)
    a = torch.tensor(np.asarray(im), requires_grad=True)
    b = torch.tensor(np.asarray(s), requires_grad=True)
    loss = crit(a, b)
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def bars_table():
    """[(kind, B, a, margin, rounds, loss rel err, worst grad_im err / rms, worst grad_s err / rms)] of the float32 CPU mirror."""
    rows = []
    for kind in KINDS:
        for B, a, m in CASES:
            im, s, rounds = conditioned_inputs(B, a, m)
            rl, rgi, rgs = conditioned_reference(B, a, m, kind)
            l, gi, gs = mirror_float32(im, s, kind, m)
            rows.append((kind, B, a, m, rounds, abs(l - rl) / abs(rl) if rl else abs(l), grad_errors(gi, rgi), grad_errors(gs, rgs)))
    return rows
