"""CPU tier of the pairwise and hardest ranking losses: the float64 reference of tests/ranking_loss_ref.py against the imported
reference's golden and against float64 autograd of the torch mirror, the conditioning of the test inputs, the C header and
``losses.make_criterion``. No GPU: every module call here runs the torch formulation."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import ranking_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_meets_the_imported_reference(golden, kind):
    """tests/golden/loss_ranking.npz (oracle/gen_golden_losses.py): the bars of tests/test_host_logic.py's torch test."""
    g = golden("loss_ranking")
    loss, g_im, g_s = R.ranking_loss_ref(g["im"], g["s"], kind, float(g["margin"]))
    assert abs(loss - float(g[kind + "_loss"])) < 1e-5 * max(1.0, abs(float(g[kind + "_loss"])))
    assert np.abs(g_im - g[kind + "_grad_im"]).max() < 1e-6
    assert np.abs(g_s - g[kind + "_grad_s"]).max() < 1e-6


@pytest.mark.parametrize("a", [0.45, 0.9])
@pytest.mark.parametrize("B", [2, 3, 33, 129])
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_meets_float64_autograd_of_the_mirror(kind, B, a):
    from text2loc_amd.losses import HardestRankingLoss, PairwiseRankingLoss

    im, s, _ = R.conditioned_inputs(B, a)
    crit = PairwiseRankingLoss(0.35) if kind == "pairwise" else HardestRankingLoss(0.35)
    before = (type(crit).engine_calls, type(crit).torch_calls)
    x = torch.tensor(np.asarray(im, np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(s, np.float64), requires_grad=True)
    loss = crit(x, y)
    loss.backward()
    assert (type(crit).engine_calls, type(crit).torch_calls) == (before[0], before[1] + 1)
    rl, rgi, rgs = R.conditioned_reference(B, a, 0.35, kind)
    assert abs(float(loss.detach()) - rl) <= 1e-10 * max(1.0, abs(rl))
    assert np.abs(x.grad.numpy() - rgi).max() <= 1e-10 and np.abs(y.grad.numpy() - rgs).max() <= 1e-10


@pytest.mark.parametrize("B,a,m", R.CASES)
def test_inputs_are_conditioned(B, a, m):
    im, s, rounds = R.conditioned_inputs(B, a, m)
    assert im.dtype == np.float32 and s.dtype == np.float32 and im.shape == s.shape == (B, 256)
    min_hinge, min_gap, flagged = R.conditioning(im, s, m)
    assert len(flagged) == 0 and min_hinge >= R.COND and min_gap >= R.COND
    assert rounds <= 5
    if B >= 31 and m == 0.35:  # what the recipe is for: a = 0.45 nearly every hinge active, a = 0.9 about a tenth
        c = (im / np.linalg.norm(im, axis=1, keepdims=True)).astype(np.float64) @ (s / np.linalg.norm(s, axis=1, keepdims=True)).T
        h = m - np.diag(c)[:, None] + c
        active = (h > 0)[~np.eye(B, dtype=bool)].mean()
        assert (active > 0.8) if a == 0.45 else (0.01 < active < 0.35), active


def test_conditioning_sees_a_near_tie_and_a_near_zero_hinge():
    """The flags fire on inputs built to sit at the edge: the helper is not vacuous."""
    rng = np.random.default_rng(5)
    im = rng.standard_normal((4, 256))
    s = im + 0.5 * rng.standard_normal((4, 256))
    s[2] = s[1]  # columns 1 and 2 tie in every row,
    s[3] = -im[0]  # and are row 0's two largest costs at a margin that makes every cost positive
    _, gap, flagged = R.conditioning(im, s, 1.5)
    assert gap < R.COND and 0 in flagged
    s[3] = im[3] + 0.5 * rng.standard_normal(256)
    ih, sh = im / np.linalg.norm(im, axis=1, keepdims=True), s / np.linalg.norm(s, axis=1, keepdims=True)
    c = ih @ sh.T
    m = float(c[0, 0] - c[0, 3])  # puts hA_03 at 0
    hinge, _, flagged = R.conditioning(im, s, m)
    assert hinge < R.COND and {0, 3} <= set(flagged.tolist())


def test_the_float32_mirror_stays_inside_a_quarter_of_the_bars():
    """RANK_T is 4 x the float32 CPU mirror's worst error over the GPU tier's cases (profiles/ranking_loss.md); held here on the
    cases below 300 rows with the factor 2 that another BLAS's summation order may take."""
    for kind in R.KINDS:
        for B, a, m in R.CASES:
            if B > 129:
                continue
            im, s, _ = R.conditioned_inputs(B, a, m)
            rl, rgi, rgs = R.conditioned_reference(B, a, m, kind)
            loss, gi, gs = R.mirror_float32(im, s, kind, m)
            R.assert_loss(loss, rl, f"{kind} B={B} a={a}")
            assert max(R.grad_errors(gi, rgi), R.grad_errors(gs, rgs)) <= R.RANK_T[kind] / 2


def test_one_flipped_hinge_leaves_the_bar():
    """What the bar can see: one wrong entry of G (a hinge the other way) moves elements of its row by far more than T * rms."""
    B, a, m = 128, 0.9, 0.35
    im, s, _ = R.conditioned_inputs(B, a, m)
    rl, rgi, rgs = R.conditioned_reference(B, a, m, "pairwise")
    ih = im / np.linalg.norm(im, axis=1, keepdims=True)
    sh = s / np.linalg.norm(s, axis=1, keepdims=True)
    c = ih.astype(np.float64) @ sh.T
    i, j = 5, 77
    delta = (1.0 / B) * (sh[j] - ih[i] * c[i, j]) / np.linalg.norm(im[i])  # d im_i of one more unit in G_ij (its diagonal share left out)
    assert np.abs(delta).max() > 100 * R.RANK_T["pairwise"] * R.rms(rgi)


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "t2l.h")).read()
    assert re.search(r"#define\s+T2L_RANK_PAIRWISE\s+0\b", text) and re.search(r"#define\s+T2L_RANK_HARDEST\s+1\b", text)
    decl = re.search(r"int\s+t2l_ranking_loss\s*\(([^;]*)\)\s*;", text)
    assert decl, "include/t2l.h does not declare t2l_ranking_loss"
    args = " ".join(decl.group(1).split())
    assert args == ("t2l_ctx* ctx, const float* im, const float* s, int32_t batch, int32_t kind, float margin, float scale, "
                    "float* out_loss, float* grad_im, float* grad_s, void* stream")
    assert re.search(r"#define\s+T2L_ABI_VERSION\s+2\b", text)  # an addition: the version stays
    from text2loc_amd import engine

    assert "t2l_ranking_loss" in engine.EXPORTS


def test_make_criterion_maps_the_four_values():
    from text2loc_amd import losses

    args = argparse.Namespace(ranking_loss="pairwise", margin=0.35, temperature=0.1)
    c = losses.make_criterion(args)
    assert type(c) is losses.PairwiseRankingLoss and c.margin == 0.35 and not c.gather
    args.ranking_loss = "hardest"
    c = losses.make_criterion(args)
    assert type(c) is losses.HardestRankingLoss and c.margin == 0.35 and c.scale == 64.0
    args.ranking_loss = "contrastive"
    c = losses.make_criterion(args)
    assert type(c) is losses.ContrastiveLoss and c.temperature == 0.1
    args.ranking_loss = "triplet"
    with pytest.raises(NotImplementedError, match="triplet"):
        losses.make_criterion(args)
    args.ranking_loss = "pairwise"
    assert losses.make_criterion(args, gather=True).gather


def test_modules_keep_the_torch_path_off_the_engine_shapes():
    """CPU tensors never reach the engine, whatever ``use_engine`` says; the counters say which path ran."""
    from text2loc_amd.losses import PairwiseRankingLoss

    crit = PairwiseRankingLoss(0.35)
    assert crit.use_engine and PairwiseRankingLoss.use_engine
    n = PairwiseRankingLoss.torch_calls
    e = PairwiseRankingLoss.engine_calls
    crit(torch.randn(5, 256), torch.randn(5, 256))
    crit(torch.randn(5, 128), torch.randn(5, 128))
    assert PairwiseRankingLoss.torch_calls == n + 2 and PairwiseRankingLoss.engine_calls == e
