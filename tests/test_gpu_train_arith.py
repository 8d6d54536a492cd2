"""GPU tier: the bf16 and split-bf16 training steps against float64 oracles that apply the SAME declared roundings at the same points
(oracle/arith.py): option ``train_bf16`` (object branch, PointNet++ backbone) and ``text_train_bf16`` (text head) in mode 2 (split-bf16)
and mode 1 (bf16 operands; PointNet++ also stores its edge rows as bf16).

Mode 2: what remains between a correct kernel and such an oracle is float32 against float64 accumulation, so the bars are the ones the
float32 path meets against the exact oracle (tests/test_gpu_train.py, tests/test_gpu_text_train.py, tests/test_gpu_pointnet_train.py)
unless a comment says what was measured. Negative control: the same engine run misses the bars by >= 10x against split-bf16 WITHOUT
its lo*hi term (a product that rounds one operand to 8 bits).

Mode 1: an operand within float32 round-off of a bf16 rounding midpoint rounds the other way in the emulation, a full bf16 ulp. The
differences this leaves grow with every further rounded product (roughly 0.1 sqrt(d) from a relative difference d), so the deep end of
a step (gradients of the first layers, the output after many products) agrees with the bf16 oracle only to a fraction of bf16's own
noise, while early, heavily averaged quantities (running statistics, the median forward error) agree far better. The mode-1 bars are
therefore calibrated on MI355X (each comment gives the measured range) and 2x .. 150x tighter than the bars of the earlier bf16 tests;
the negative controls compare the engine's distance from the bf16 oracle with its distance from the exact and the truncating models
on the quantity that separates them best, and each of those distances is >= 10x the first (>= 5x for the object branch against the
exact model at 64 cells, where 7-12x is measured)."""
import numpy as np
import pytest
import torch

from oracle import arith as A
from oracle import t2l_oracle_pointnet_train as OPT
from oracle import t2l_oracle_text_train as OTT
from oracle import t2l_oracle_train as OT
from tests.test_gpu_pointnet_train import bind_all
from tests.test_gpu_text_train import P as TP
from tests.test_gpu_text_train import _bind as text_bind
from tests.test_gpu_text_train import _check_grads
from tests.test_gpu_train import assert_grads, bind, to_dev
from text2loc_amd import synth

pytestmark = pytest.mark.gpu
SPLIT = A.SPLIT


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- object branch (train.hip) -------------------------------------------------------------------------------------------------------
def _object_run(eng, arith, block, embed, p_drop, n_cells, min_obj, max_obj):
    cells = synth.make_cells(n_cells, seed=21 + n_cells, with_pn_feat=True, min_obj=min_obj, max_obj=max_obj)
    sd = synth.make_object_branch_weights(3)
    try:
        eng.set_option("train_bf16", arith)
        eng.set_option("train_gemm_block", block)
        tensors = bind(eng, sd, embed)
        seed = 0xC0FFEE + n_cells
        out = eng.encode_cells_train(to_dev(cells, embed), dropout_p=p_drop, seed=seed)
        gout = np.random.default_rng(n_cells).standard_normal((n_cells, 256)).astype(np.float32) * 0.05
        gpn = None if embed else torch.zeros((int(cells["offsets"][-1]), 256), device="cuda")
        eng.encode_cells_backward(torch.from_numpy(gout).cuda(), gpn)
        torch.cuda.synchronize()
    finally:
        eng.set_option("train_bf16", 0)
        eng.set_option("train_gemm_block", 0)
    got = {"out": out.cpu().numpy().astype(np.float64), "pn": None if embed else gpn.cpu().numpy().astype(np.float64),
           "grads": {n: t[1].cpu().numpy().astype(np.float64) for n, t in tensors.items() if t[1] is not None},
           "running": {n: t[0].cpu().numpy().astype(np.float64) for n, t in tensors.items() if "running_" in n}}

    def oracle(a):
        return OT.encode_cells_train(cells, sd, embed, embed, grad_out=gout, p_drop=float(np.float32(p_drop)), seed=seed, arith=a)

    return got, tensors, sd, oracle


def _median_excess(got, ref_grads, bar=2e-3):
    """max over the informative gradient tensors of median(err) / (bar * rms + 1e-8): assert_grads' median bar is 1."""
    worst = 0.0
    for n, g in ref_grads.items():
        exp = np.asarray(g, dtype=np.float64).ravel()
        rms = np.sqrt((exp ** 2).mean())
        if rms < 1e-9 or n.endswith("num_encoder.0.0.weight"):  # (the two families assert_grads bounds separately)
            continue
        worst = max(worst, float(np.median(np.abs(got[n].ravel() - exp)) / (bar * rms + 1e-8)))
    return worst


def _grad_stats(got, ref_grads, skip):
    """(worst median error / rms, worst Frobenius ratio) over the gradient tensors not skipped."""
    med = fro = 0.0
    for n, g in ref_grads.items():
        exp = np.asarray(g, dtype=np.float64).ravel()
        rms = np.sqrt((exp ** 2).mean())
        if skip(n) or rms < 1e-9:
            continue
        err = np.abs(np.asarray(got[n], dtype=np.float64).ravel() - exp)
        med = max(med, float(np.median(err) / rms))
        fro = max(fro, float(np.sqrt((err ** 2).sum()) / np.sqrt((exp ** 2).sum())))
    return med, fro


def _fwd_median(out, ref):
    """median forward error / rms of the reference: the forward quantity the mode-1 chaos (module docstring) reaches least"""
    return float(np.median(np.abs(out - ref)) / np.sqrt((ref ** 2).mean()))


def _object_skip(n):  # the two families assert_grads bounds separately (true gradient 0; scale-invariant [64, 1] Linear)
    return n.endswith("num_encoder.0.0.weight") or (n.startswith("object_encoder.") and n.endswith(".0.bias"))


@pytest.mark.parametrize("block", [32, 64])
@pytest.mark.parametrize("n_cells,min_obj,max_obj", [(5, 3, 33), (64, 6, 35)])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("embed", [True, False], ids=["embed", "pn"])
def test_object_branch_meets_the_rounding_exact_oracle(eng, embed, p_drop, n_cells, min_obj, max_obj, block):
    """Forward (2e-5), every parameter gradient, d/d features2 and the running statistics at the float32 path's bars
    (test_gpu_train.py), both GEMM block forms (64 x 64 is the default with bf16 operands). Measured: the forward at 1e-6 .. 6e-6, the
    worst gradient median at 3e-3 .. 0.57 of its bar."""
    got, tensors, sd, oracle = _object_run(eng, SPLIT, block, embed, p_drop, n_cells, min_obj, max_obj)
    ref_out, info = oracle(SPLIT)
    assert np.abs(got["out"] - ref_out).max() < 2e-5
    assert_grads(tensors, info["grads"])
    if not embed:
        exp = info["grad_pn_feat"]
        err = np.abs(got["pn"] - exp)
        rms = np.sqrt((exp ** 2).mean())
        assert np.median(err) < 2e-3 * rms + 1e-9 and np.quantile(err, 0.9) < 2e-2 * rms + 1e-8
    new = OT.bn_running_update(sd, info["bn_stats"])
    for k, v in new.items():
        if not k.endswith("num_batches_tracked"):
            assert np.allclose(got["running"][k], v, rtol=2e-4, atol=2e-5), k


def test_object_branch_bars_exclude_split_bf16_without_lo_hi(eng):
    """(measured: the forward at 57x its bar, the worst gradient median at 54x)"""
    got, _, _, oracle = _object_run(eng, SPLIT, 0, True, 0.1, 64, 6, 35)
    ref_out, info = oracle(A.SPLIT_NO_LOHI)
    fwd = np.abs(got["out"] - ref_out).max() / 2e-5
    grad = _median_excess(got["grads"], info["grads"])
    assert fwd >= 10 and grad >= 10, (fwd, grad)


@pytest.mark.parametrize("block", [32, 64])
@pytest.mark.parametrize("n_cells,min_obj,max_obj", [(5, 3, 33), (64, 6, 35)])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("embed", [True, False], ids=["embed", "pn"])
def test_object_branch_bf16_tracks_the_bf16_oracle(eng, embed, p_drop, n_cells, min_obj, max_obj, block):
    """Mode 1 against the bf16 oracle, calibrated bars (module docstring). Forward 1e-3 (20x tighter than test_gpu_train.py's 2e-2 against
    the float32 goldens; measured 1.2e-4 .. 7.5e-4); every gradient tensor: median error < 0.08 of its rms (measured <= 0.061) and
    Frobenius ratio < 0.12 (measured <= 0.088; the earlier bars: cosine > 0.98 and the norm within 10 % on the large tensors)."""
    got, _, _, oracle = _object_run(eng, A.BF16, block, embed, p_drop, n_cells, min_obj, max_obj)
    ref_out, info = oracle(A.BF16)
    assert np.abs(got["out"] - ref_out).max() < 1e-3
    med, fro = _grad_stats(got["grads"], info["grads"], _object_skip)
    assert med < 0.08 and fro < 0.12, (med, fro)


@pytest.mark.parametrize("wrong,factor", [(A.EXACT, 5), (A.BF16_TRUNC, 10)], ids=["vs_exact", "vs_truncating"])
def test_object_branch_bf16_is_closest_to_rounding_to_nearest_even(eng, wrong, factor):
    """The published batch (64 cells): the median forward error against the exact / truncating model is >= 5x / >= 10x the one
    against the bf16 oracle (measured 12x / 26x here; 7-12x / 17-29x over the four 64-cell cases, 4-5x against the exact model at 5 cells,
    where fewer chained rows average the flips less)."""
    got, _, _, oracle = _object_run(eng, A.BF16, 32, True, 0.0, 64, 6, 35)
    near = _fwd_median(got["out"], oracle(A.BF16)[0])
    far = _fwd_median(got["out"], oracle(wrong)[0])
    assert far >= factor * near, (far, near)


# ---- text head (train.hip text_* + text_head.hip fast_gemm) ----------------------------------------------------------------------------
ZERO_GRAD = ("inter_mlp.0.0.bias", "intra_module.0.norm2.bias")  # true gradient 0 in exact arithmetic (test_gpu_text_train._check_grads)


def _text_run(arith, n_desc, S, L, p):
    from text2loc_amd.engine import Engine

    sd = synth.make_language_head_weights(6)
    hidden = synth.make_t5_hidden(n_desc * S, L, seed=n_desc * 10 + L)
    G = np.random.default_rng(L).standard_normal((n_desc, 256)).astype(np.float32)
    seed = 1234 + L
    eng = Engine(0)
    try:
        tensors = text_bind(eng, sd)
        eng.set_option("text_train_bf16", arith)
        out = eng.text_head_train(torch.from_numpy(hidden).cuda(), n_desc, dropout_p=p, seed=seed)
        eng.text_head_backward(torch.from_numpy(G).cuda())
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        tensors = {n: (t[0].cpu(), None if t[1] is None else t[1].cpu()) for n, t in tensors.items()}
    finally:
        eng.close()

    def oracle(a):
        return OTT.text_head_train(hidden, sd, n_desc, grad_out=G, p_drop=float(np.float32(p)), seed=seed, arith=a)

    return got, tensors, sd, oracle


def _q90_excess(tensors, ref_grads, tol_rms=1e-2):
    """max over the informative gradient tensors of the 90th-percentile error / (tol_rms * rms): _check_grads(frac=0.9)'s bar is 1."""
    worst = 0.0
    for n, rg in ref_grads.items():
        if n.endswith(ZERO_GRAD + ("in_proj_bias",)):
            continue
        g = tensors[n][1].numpy().astype(np.float64).ravel()
        rg = np.asarray(rg, dtype=np.float64).ravel()
        worst = max(worst, float(np.quantile(np.abs(g - rg), 0.9) / (tol_rms * np.sqrt((rg ** 2).mean()) + 1e-7)))
    return worst


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("n_desc,S,L", [(4, 6, 7), (16, 6, 12), (64, 6, 24)])
def test_text_head_meets_the_rounding_exact_oracle(n_desc, S, L, p):
    """Both GEMM paths of the head (fast_gemm from 64 rows on, gemm_f32.h below) and the published batch (64 descriptions x 6 hints):
    the forward to 1e-4 of its scale (measured 3e-6 .. 5e-6) and every gradient at the bars of test_gpu_text_train.py (measured: the
    90th percentile at <= 0.34 of its bar). The two gradients that are exactly 0 in exact arithmetic are not 0 once the products are
    rounded (a column sum of a rounded operand): they are held to the oracle's value within 5e-4 — the float32 path's 1e-4 holds up to 16
    descriptions; measured at the published batch: 1.1e-4 / 2.1e-4 (p = 0 / 0.1), a cancellation residue summed over 9,216 tokens."""
    got, tensors, sd, oracle = _text_run(SPLIT, n_desc, S, L, p)
    ref, info = oracle(SPLIT)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    _check_grads(tensors, {n: g for n, g in info["grads"].items() if not n.endswith(ZERO_GRAD)}, tol_rms=1e-2, frac=0.9)
    for n in (TP + z for z in ZERO_GRAD):
        assert np.abs(tensors[n][1].numpy() - np.asarray(info["grads"][n]).reshape(tensors[n][1].shape)).max() < 5e-4, n
    new = OT.bn_running_update(sd, info["bn_stats"])
    for k in (TP + "inter_mlp.0.1.running_mean", TP + "inter_mlp.0.1.running_var"):
        assert np.allclose(tensors[k][0].numpy(), new[k], rtol=2e-4, atol=2e-5), k


def test_text_head_bars_exclude_split_bf16_without_lo_hi():
    """(measured: the forward at 71x its bar, the worst 90th percentile at 15x)"""
    got, tensors, _, oracle = _text_run(SPLIT, 16, 6, 12, 0.1)
    ref, info = oracle(A.SPLIT_NO_LOHI)
    fwd = np.abs(got - ref).max() / (1e-4 * max(1.0, np.abs(ref).max()))
    grad = _q90_excess(tensors, info["grads"])
    assert fwd >= 10 and grad >= 10, (fwd, grad)


def _text_skip(n):  # (true gradient 0 in exact arithmetic; the key third of in_proj_bias likewise)
    return n.endswith(ZERO_GRAD + ("in_proj_bias",))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("n_desc,S,L", [(4, 6, 7), (16, 6, 12), (64, 6, 24)])
def test_text_head_bf16_tracks_the_bf16_oracle(n_desc, S, L, p):
    """Mode 1 against the bf16 oracle, calibrated bars (module docstring): the forward to 2e-3 of its scale (10x tighter than
    test_gpu_text_train.py's 2e-2; measured 4.5e-4 .. 1.2e-3) and its median error to 4e-4 of its rms (measured 1.6e-4 .. 2.3e-4); every
    gradient tensor: median error < 0.05 of its rms (measured <= 0.036), Frobenius ratio < 0.08 (measured <= 0.056; the earlier bar: one
    tensor at cosine > 0.9)."""
    got, tensors, _, oracle = _text_run(A.BF16, n_desc, S, L, p)
    ref, info = oracle(A.BF16)
    assert np.abs(got - ref).max() < 2e-3 * max(1.0, np.abs(ref).max())
    assert _fwd_median(got, ref) < 4e-4
    med, fro = _grad_stats({n: t[1].numpy() for n, t in tensors.items() if t[1] is not None}, info["grads"], _text_skip)
    assert med < 0.05 and fro < 0.08, (med, fro)


@pytest.mark.parametrize("wrong", [A.EXACT, A.BF16_TRUNC], ids=["vs_exact", "vs_truncating"])
@pytest.mark.parametrize("n_desc,S,L,p", [(16, 6, 12, 0.0), (64, 6, 24, 0.1)])
def test_text_head_bf16_is_closest_to_rounding_to_nearest_even(n_desc, S, L, p, wrong):
    """The median forward error against the exact / truncating model is >= 10x the one against the bf16 oracle (measured 13x / 24x and
    13x / 23x for these two batches; 11-13x / 20-23x over every measured case)."""
    got, _, _, oracle = _text_run(A.BF16, n_desc, S, L, p)
    near = _fwd_median(got, oracle(A.BF16)[0])
    far = _fwd_median(got, oracle(wrong)[0])
    assert far >= 10 * near, (far, near)


# ---- PointNet++ backbone (pointnet_train.h, gemm_rows2.h) -----------------------------------------------------------------------------
PN = "object_encoder.pointnet."
PN_CASES = {"ragged12": dict(n=12, seed=21, min_obj=1, max_obj=9, pts=5), "large_cells": dict(n=3, seed=8, min_obj=28, max_obj=34, pts=6)}


def _pn_run(eng, arith, case, self_loops):
    c = PN_CASES[case]
    cells = synth.make_cells(c["n"], seed=c["seed"], min_obj=c["min_obj"], max_obj=c["max_obj"])
    pos, rgb = synth.make_sampled_points(cells, c["pts"])
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    sd_pn = synth.make_pointnet_weights(3)
    R = np.random.default_rng(2).standard_normal((pos.shape[0], 256)).astype(np.float32)
    try:
        eng.set_option("train_bf16", arith)
        eng.set_option("pointnet_pyg_self_loops", self_loops)
        tensors = bind_all(eng, synth.make_object_branch_weights(2), sd_pn)
        f2 = eng.pointnet_features_train(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), offs)
        eng.zero_grad()
        eng.pointnet_backward(torch.from_numpy(R).cuda())
        torch.cuda.synchronize()
    finally:
        eng.set_option("train_bf16", 0)
        eng.set_option("pointnet_pyg_self_loops", 1)
    got = {"f2": f2.cpu().numpy().astype(np.float64),
           "grads": {k: t[1].cpu().numpy().astype(np.float64) for k, t in tensors.items() if k.startswith(PN) and t[1] is not None},
           "running": {k: t[0].cpu().numpy().astype(np.float64) for k, t in tensors.items() if k.startswith(PN) and "running_" in k}}

    def oracle(a):
        return OPT.forward_backward(pos, rgb, offs, sd_pn, grad_f2=R.astype(np.float64), pyg_self_loops=bool(self_loops), arith=a)

    return got, oracle


def _pn_metrics(got, ref):
    """(features max error / scale, worst median error / rms, worst Frobenius ratio) over the informative gradient tensors
    (the Linear biases in front of a BatchNorm have true gradient 0 and are bounded separately)."""
    f2, info = ref
    fwd = float(np.abs(got["f2"] - f2).max() / max(np.abs(f2).max(), 1e-30))
    med = fro = 0.0
    for n, g in info["grads"].items():
        if n.endswith(".0.bias") and "lin" not in n:
            continue
        exp = np.asarray(g, dtype=np.float64).ravel()
        err = np.abs(got["grads"][n].ravel() - exp)
        med = max(med, float(np.median(err) / max(np.sqrt((exp ** 2).mean()), 1e-30)))
        fro = max(fro, float(np.sqrt((err ** 2).sum()) / max(np.sqrt((exp ** 2).sum()), 1e-30)))
    return fwd, med, fro


# the float32 path's bars against the exact oracle (test_gpu_pointnet_train.py: 2e-4 of the features' scale, check()'s median 1e-2 of
# the rms and Frobenius 0.03) — 1.7x tighter than the split-bf16 row of test_reduced_precision_gemms_track_the_f32_run_on_a_ragged_batch
# (0.05 of the norm), not 10x: measured on MI355X, the worst tensor sits at 4e-3 .. 7.3e-3 (median) and 6.3e-3 .. 1.2e-2 (Frobenius)
# of its norm — arg-max rows and ReLU signs within float32 rounding of a tie fall the other way, as in the float32 path (check()'s comment)
PN_BARS = (2e-4, 1e-2, 3e-2)


@pytest.mark.parametrize("self_loops", [1, 0])
@pytest.mark.parametrize("case", list(PN_CASES))
def test_pointnet_train_meets_the_rounding_exact_oracle(eng, case, self_loops):
    """The ragged 12-cell batch (every tile shape of tn2_kernel, every pass count of rows2_kernel) and three cells of 28-34 objects, with
    and without PyG's self-loop edge: features, running statistics (one update per cell) and every parameter gradient."""
    got, oracle = _pn_run(eng, SPLIT, case, self_loops)
    ref = oracle(SPLIT)
    fwd, med, fro = _pn_metrics(got, ref)
    assert fwd < PN_BARS[0] and med < PN_BARS[1] and fro < PN_BARS[2], (fwd, med, fro)
    for k, v in ref[1]["running"].items():  # (measured <= 1.4e-6)
        assert np.abs(got["running"][k] - v).max() < 2e-5 * max(1.0, np.abs(v).max()), k
    for n, g in got["grads"].items():  # Linear biases in front of a BatchNorm: noise around a true 0
        if n.endswith(".0.bias") and "lin" not in n:
            assert np.abs(g).max() < 2e-3 * max(1.0, np.abs(got["grads"][n.replace(".0.bias", ".1.bias")]).max()), n


def test_pointnet_train_bars_exclude_split_bf16_without_lo_hi(eng):
    """(measured: features at 62x their bar, the worst median at 41x, the worst Frobenius ratio at 17x)"""
    got, oracle = _pn_run(eng, SPLIT, "ragged12", 1)
    fwd, med, fro = _pn_metrics(got, oracle(A.SPLIT_NO_LOHI))
    assert min(fwd / PN_BARS[0], med / PN_BARS[1], fro / PN_BARS[2]) >= 10, (fwd, med, fro)


def _pn_running(got, info):
    return max(float(np.abs(got["running"][k] - v).max() / max(1.0, np.abs(v).max())) for k, v in info["running"].items())


@pytest.mark.parametrize("self_loops", [1, 0])
@pytest.mark.parametrize("case", list(PN_CASES))
def test_pointnet_train_bf16_tracks_the_bf16_oracle(eng, case, self_loops):
    """Mode 1 (bf16 operands AND bf16-stored edge rows) against the bf16 oracle, calibrated bars (module docstring): running statistics to
    4e-4 (measured 3.2e-5 .. 1.8e-4; 150x tighter than the 6e-2 of test_reduced_precision_gemms_track_the_f32_run_on_a_ragged_batch),
    features to 2e-2 of their scale (measured 6e-3 .. 9.5e-3; 3x tighter), every gradient tensor's median error < 0.2 of its rms (measured
    <= 0.17) and Frobenius ratio < 0.3 (measured 0.19 .. 0.22; 2.2x tighter than 0.65). Four levels of rounded products and stored rows
    below the loss, arg-max rows that tie after the rounding to 8 bits and flipped roundings keep the gradients at a fifth of their norm:
    what a rounding-exact oracle cannot remove (module docstring), and what the negative control below shows is still 3x closer than
    the exact model."""
    got, oracle = _pn_run(eng, A.BF16, case, self_loops)
    f2, info = oracle(A.BF16)
    assert _pn_running(got, info) < 4e-4
    assert np.abs(got["f2"] - f2).max() < 2e-2 * np.abs(f2).max()
    med, fro = _grad_stats(got["grads"], info["grads"], lambda n: n.endswith(".0.bias") and "lin" not in n)
    assert med < 0.2 and fro < 0.3, (med, fro)


@pytest.mark.parametrize("wrong", [A.EXACT, A.BF16_TRUNC], ids=["vs_exact", "vs_truncating"])
@pytest.mark.parametrize("case", list(PN_CASES))
def test_pointnet_train_bf16_is_closest_to_rounding_to_nearest_even(eng, case, wrong):
    """The running statistics (the per-cell BatchNorm sums taken before the rounding of the stored rows, gemm_rows2.h:26-32) against the
    exact / truncating model are >= 10x as far as against the bf16 oracle (measured 19-41x / 64-196x)."""
    got, oracle = _pn_run(eng, A.BF16, case, 1)
    near = _pn_running(got, oracle(A.BF16)[1])
    far = _pn_running(got, oracle(wrong)[1])
    assert far >= 10 * near, (far, near)
