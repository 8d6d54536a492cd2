"""GPU tier: the training step of the object branch through the C ABI —
t2l_train_bind / t2l_encode_cells_train / t2l_encode_cells_backward / t2l_adam_step — against the float64 oracle
(same counter-based dropout masks) and against the goldens of the reference's own train step."""
import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from oracle import t2l_oracle_train as OT
from text2loc_amd import synth
from tests.test_oracle_train import golden_view, load_case, margin_grad_check

pytestmark = pytest.mark.gpu

# float32 MFMA accumulation order on the device vs torch's CPU kernels: the margin fixtures are asserted at GPU_MARGIN_SCALE x 1e-4
# of each gradient tensor's rms (the float64 / float32 numpy oracles meet 1e-4, tests/test_oracle_train.py)
GPU_MARGIN_SCALE = 10.0


def used_names(sd, embed, color_embed=None):
    """embed: class_embed, and color_embed too unless that is given apart"""
    color_embed = embed if color_embed is None else color_embed
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or k.startswith("object_encoder.pointnet."):
            continue
        if (color_embed and ".color_encoder." in k) or (embed and ".mlp_pointnet." in k):
            continue
        if (not embed and k.endswith("class_embedding.weight")) or (not color_embed and k.endswith("color_embedding.weight")):
            continue
        out[k] = v
    return out


def bind(eng, sd, embed, color_embed=None):
    """name -> (param tensor, grad tensor | None) on the GPU, bound to the engine."""
    color_embed = embed if color_embed is None else color_embed
    tensors = {}
    for k, v in used_names(sd, embed, color_embed).items():
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tensors, class_embed=embed, color_embed=color_embed)
    return tensors


def to_dev(cells, embed):
    """embed: class_embed (without it the class branch reads pn_feat)"""
    keys = ["offsets", "class_idx", "color_idx", "rgb", "center", "n_pts"] + ([] if embed else ["pn_feat"])
    return {k: torch.from_numpy(np.ascontiguousarray(cells[k])).cuda() for k in keys}


def assert_grads(tensors, ref_grads, tol=2e-3):
    for n, g in ref_grads.items():
        got = tensors[n][1].cpu().numpy().astype(np.float64).ravel()
        exp = np.asarray(g, dtype=np.float64).ravel()
        rms = max(np.sqrt((exp ** 2).mean()), 1e-30)
        if n.startswith("object_encoder.") and n.endswith(".0.bias") and rms < 1e-9:
            # Linear bias in front of a BatchNorm: true gradient 0, float32 leaves cancellation noise
            assert np.abs(got).max() < 1e-3 * max(1.0, np.abs(tensors[n.replace(".0.bias", ".1.bias")][1].cpu().numpy()).max()), n
            continue
        err = np.abs(got - exp)
        if n.endswith("num_encoder.0.0.weight"):
            # [64,1] Linear in front of a BatchNorm: y = w*x + b is scale-invariant in w, so the true gradient is only
            # the eps/(var+eps) residual of terms that cancel to ~1e-5 of their size; float32 leaves noise of that order
            assert err.max() < 2e-4, (n, err.max())
            continue
        # float32 kernels vs the float64 oracle: a ReLU input within float32 rounding of 0 may land on the other side,
        # which moves the gradients of everything upstream by a fraction of a percent of their rms and one row/column of the
        # neighbouring weight gradients by one token's contribution (measured: the imported float32 reference differs
        # from the float64 oracle in the same way, tests/test_oracle_train.py). A wrong formula is O(1) everywhere, so:
        # tight median, loose tail.
        assert np.median(err) < 2e-3 * rms + 1e-8, (n, np.median(err), rms)
        assert np.quantile(err, 0.9) < tol * 10 * rms + 1e-7, (n, np.quantile(err, 0.9), rms)
        assert np.sqrt((err ** 2).sum()) < 0.15 * np.sqrt((exp ** 2).sum()) + 1e-6 and err.max() < 2.0 * rms + 1e-6, (n, err.max(), rms)


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("embed", [True, False])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("n_cells,min_obj,max_obj", [(5, 3, 33), (64, 6, 35)])
def test_forward_backward_match_the_float64_oracle(eng, embed, p_drop, n_cells, min_obj, max_obj):
    forward_backward_case(eng, embed, embed, p_drop, n_cells, min_obj, max_obj)


@pytest.mark.parametrize("embed,color_embed", [(True, False), (False, True)], ids=["class", "color"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_forward_backward_match_the_float64_oracle_in_the_mixed_configurations(eng, embed, color_embed, p_drop):
    """The same check, same bars, with the two flags apart, at the small shape (5 cells of 3 to 33 objects: across the 28-slot cut):
    class_embed only — one embedding job beside three small branches — and color_embed only — the PointNet-feature block, one
    embedding job and two small branches."""
    forward_backward_case(eng, embed, color_embed, p_drop, 5, 3, 33)


def forward_backward_case(eng, embed, color_embed, p_drop, n_cells, min_obj, max_obj):  # embed: class_embed
    cells = synth.make_cells(n_cells, seed=21 + n_cells, with_pn_feat=True, min_obj=min_obj, max_obj=max_obj)
    sd = synth.make_object_branch_weights(3)
    tensors = bind(eng, sd, embed, color_embed)
    dcells = to_dev(cells, embed)
    seed = 0xC0FFEE + n_cells
    p32 = float(np.float32(p_drop))
    out = eng.encode_cells_train(dcells, dropout_p=p_drop, seed=seed)
    rng = np.random.default_rng(n_cells)
    gout = rng.standard_normal((n_cells, 256)).astype(np.float32) * 0.05
    gpn = None if embed else torch.zeros((int(cells["offsets"][-1]), 256), device="cuda")
    eng.encode_cells_backward(torch.from_numpy(gout).cuda(), gpn)
    torch.cuda.synchronize()
    ref_out, info = OT.encode_cells_train(cells, sd, embed, color_embed, grad_out=gout, p_drop=p32, seed=seed)
    assert np.abs(out.cpu().numpy() - ref_out).max() < 2e-5
    assert_grads(tensors, info["grads"])
    if not embed:
        exp = info["grad_pn_feat"]
        err = np.abs(gpn.cpu().numpy() - exp)
        rms = np.sqrt((exp ** 2).mean())
        assert np.median(err) < 2e-3 * rms + 1e-9 and np.quantile(err, 0.9) < 2e-2 * rms + 1e-8
    # BatchNorm running statistics (momentum 0.1, unbiased variance)
    new = OT.bn_running_update(sd, info["bn_stats"])
    checked = 0
    for k, v in new.items():
        if k.endswith("num_batches_tracked"):
            continue
        assert np.allclose(tensors[k][0].cpu().numpy(), v, rtol=2e-4, atol=2e-5), k
        checked += 1
    assert checked >= {(True, True): 10, (False, False): 14, (True, False): 14, (False, True): 12}[(embed, color_embed)]  # (mixed: 10 + 4 / 10 + 2)


def test_gradients_accumulate_and_zero_grad(eng):
    cells = synth.make_cells(4, seed=2, with_pn_feat=True)
    sd = synth.make_object_branch_weights(1)
    tensors = bind(eng, sd, True)
    dcells = to_dev(cells, True)
    g = torch.randn(4, 256, device="cuda") * 0.1
    eng.encode_cells_train(dcells, dropout_p=0.0, seed=1)
    eng.encode_cells_backward(g)
    one = {n: t[1].clone() for n, t in tensors.items() if t[1] is not None}
    eng.encode_cells_backward(g)  # a second backward through the same graph adds, like autograd with retain_graph
    for n, t in tensors.items():
        if t[1] is not None:
            # float atomics: the summation order differs between the two passes; gradients that are exactly 0 in exact
            # arithmetic (Linear biases in front of a BatchNorm, key biases) are pure cancellation noise of ~1e-6
            assert torch.allclose(t[1], 2 * one[n], rtol=1e-3, atol=1e-3 * float(one[n].abs().max()) + 2e-5), n
    eng.zero_grad()
    torch.cuda.synchronize()
    assert all(float(t[1].abs().max()) == 0.0 for t in tensors.values() if t[1] is not None)


def test_adam_two_steps_match_torch_adam_arithmetic(eng):
    cells = synth.make_cells(6, seed=8, with_pn_feat=True)
    sd = synth.make_object_branch_weights(4)
    tensors = bind(eng, sd, True)
    dcells = to_dev(cells, True)
    g = torch.randn(6, 256, device="cuda") * 0.1
    state = {n: (t[0].cpu().numpy().astype(np.float64), 0.0, 0.0) for n, t in tensors.items() if t[1] is not None}
    for step in (1, 2):
        eng.zero_grad()
        eng.encode_cells_train(dcells, dropout_p=0.1, seed=step)
        eng.encode_cells_backward(g)
        grads = {n: t[1].cpu().numpy().astype(np.float64) for n, t in tensors.items() if t[1] is not None}
        eng.adam_step(1e-3)
        torch.cuda.synchronize()
        for n, (p, m, v) in state.items():
            state[n] = OT.adam_step(p, grads[n], m, v, step, 1e-3)
            # elements whose gradient is ~0 sit on Adam's eps knee: compare where the update is well conditioned
            ok = np.abs(grads[n]) > 1e-6
            if ok.any():
                assert np.abs(tensors[n][0].cpu().numpy() - state[n][0])[ok].max() < 5e-6, (n, step)


@pytest.mark.parametrize("mode", ["embed", "pn"])
def test_train_step_matches_the_reference_run(eng, golden, mode):
    g = golden(f"train_step_{mode}")
    cells, sd, embed = load_case(g, mode)
    tensors = bind(eng, sd, embed)
    dcells = to_dev(cells, embed)
    positive = eng.encode_cells_train(dcells, dropout_p=0.0, seed=0)
    assert np.abs(positive.cpu().numpy() - g["positive"]).max() < 2e-5
    anchor = torch.from_numpy(g["anchor"]).cuda()
    loss, ga, gp = eng.contrastive_loss(anchor, positive, float(g["temperature"]))
    assert abs(float(loss) - float(g["loss"])) < 2e-5
    assert np.abs(ga.cpu().numpy() - g["grad_anchor"]).max() < 2e-6
    eng.encode_cells_backward(gp)
    torch.cuda.synchronize()
    for n in [str(x) for x in g["used_params"]]:
        exp, got = golden_view(g, "grad", n, tensors[n][1].cpu().numpy())
        rms = float(g[f"grad_norm/{n}"]) / np.sqrt(tensors[n][1].numel())
        if n.startswith("object_encoder.") and n.endswith(".0.bias"):
            assert np.abs(got).max() < 1e-4 and np.abs(exp).max() < 1e-4, n  # true gradient 0 (BatchNorm follows)
            continue
        err = np.abs(got - exp)
        # float32 vs float32 with different summation orders; a ReLU input within rounding of 0 may flip (see
        # tests/test_oracle_train.py), which moves upstream gradients by ~1e-3 of their rms
        assert (err < 1e-2 * rms + 1e-5).mean() >= 0.95 and err.max() < 0.2 * rms + 1e-5, (n, err.max(), rms)
        nrm = float(tensors[n][1].double().norm())
        assert abs(nrm - float(g[f"grad_norm/{n}"])) < 2e-3 * float(g[f"grad_norm/{n}"]) + 2e-4, n
    for k in g.files:
        if k.startswith("buf/") and "running_" in k and k[4:] in tensors:
            assert np.allclose(tensors[k[4:]][0].cpu().numpy(), g[k], rtol=2e-4, atol=2e-5), k
    # Adam step from the reference's gradients would be ill-conditioned to compare (lr*sign(g)); pin it where |g| is large
    before = {n: tensors[n][0].clone() for n in [str(x) for x in g["used_params"]]}
    eng.adam_step(float(g["lr"]))
    torch.cuda.synchronize()
    for n, b in before.items():
        gr = tensors[n][1]
        ok = gr.abs() > 1e-5
        if ok.any():
            delta = (tensors[n][0] - b)[ok]
            assert torch.allclose(delta, -float(g["lr"]) * torch.sign(gr[ok]), rtol=2e-2, atol=1e-6), n


@pytest.mark.parametrize("mode", ["embed", "pn"])
def test_margin_fixture_gradients_at_rounding_level(eng, golden, mode):
    """The reference run whose ReLU inputs all stay >= 1e-4 away from 0 (tests/golden/train_step_margin_*.npz): no unit can
    flip, so the HIP backward has to meet the reference's parameter gradients to 1e-4 of each tensor's rms — element-wise
    maximum over every tensor (the two BatchNorm-degenerate families keep the bounds of margin_grad_check)."""
    g = golden(f"train_step_margin_{mode}")
    cells, sd, embed = load_case(g, mode)
    tensors = bind(eng, sd, embed)
    dcells = to_dev(cells, embed)
    positive = eng.encode_cells_train(dcells, dropout_p=0.0, seed=0)
    assert np.abs(positive.cpu().numpy() - g["positive"]).max() < 2e-5
    anchor = torch.from_numpy(g["anchor"]).cuda()
    loss, ga, gp = eng.contrastive_loss(anchor, positive, float(g["temperature"]))
    assert abs(float(loss) - float(g["loss"])) < 2e-5
    # B = 3: BatchNorm over ~13 object rows amplifies float32 rounding (forward 7e-6 on 0.1-sized outputs), and 1/temperature = 10
    # carries it into the loss gradients (|grad| ~ 0.3)
    assert np.abs(ga.cpu().numpy() - g["grad_anchor"]).max() < 1e-4
    eng.encode_cells_backward(gp)
    torch.cuda.synchronize()
    for n in [str(x) for x in g["used_params"]]:
        margin_grad_check(g, n, tensors[n][1].cpu().numpy(), scale=GPU_MARGIN_SCALE)
        nrm = float(tensors[n][1].double().norm())
        if not (n.startswith("object_encoder.") and n.endswith((".0.bias", ".0.weight"))):
            assert abs(nrm - float(g[f"grad_norm/{n}"])) < 1e-4 * GPU_MARGIN_SCALE * float(g[f"grad_norm/{n}"]) + 1e-7, n


def test_error_paths(eng):
    from text2loc_amd.engine import Engine, T2LError

    e = Engine(0)
    cells = synth.make_cells(2, seed=1)
    dcells = to_dev(cells, True)
    with pytest.raises(T2LError, match="t2l_train_bind first"):
        e.encode_cells_train(dcells, dropout_p=0.0, seed=0)
    sd = synth.make_object_branch_weights(0)
    tens = {}
    for k, v in used_names(sd, True).items():
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
    broken = dict(tens)
    del broken["obj_inter_module.1.norm2.bias"]
    with pytest.raises(T2LError, match="missing tensor 'obj_inter_module.1.norm2.bias'"):
        e.train_bind(broken, class_embed=True, color_embed=True)
    broken = dict(tens)
    w = broken["object_encoder.pos_encoder.1.0.weight"][0]
    broken["object_encoder.pos_encoder.1.0.weight"] = (w[:100].contiguous(), torch.zeros_like(w[:100]))
    with pytest.raises(T2LError, match="expected 16384"):
        e.train_bind(broken, class_embed=True, color_embed=True)
    broken = dict(tens)
    broken["obj_inter_module.0.linear1.weight"] = (tens["obj_inter_module.0.linear1.weight"][0], None)
    with pytest.raises(T2LError, match="needs a gradient buffer"):
        e.train_bind(broken, class_embed=True, color_embed=True)
    e.train_bind(tens, class_embed=True, color_embed=True)
    with pytest.raises(T2LError, match="no forward pass"):
        e.encode_cells_backward(torch.zeros(2, 256, device="cuda"))
    with pytest.raises(T2LError, match=r"dropout_p must be in \[0,1\)"):
        e.encode_cells_train(dcells, dropout_p=1.0, seed=0)
    one = {k: (v[:1] if k != "offsets" else torch.tensor([0, 1], dtype=torch.int32, device="cuda")).contiguous()
           for k, v in dcells.items()}
    with pytest.raises(T2LError, match=">= 2 objects"):  # BatchNorm1d in training mode rejects a single row, as torch does
        e.encode_cells_train(one, dropout_p=0.0, seed=0)
    with pytest.raises(T2LError, match="at least two"):
        e.train_bind(tens, class_embed=True, color_embed=True, use_features=("position",))
    e.close()


@pytest.mark.parametrize("mode", ["embed", "pn"])
def test_bf16_variant_tracks_the_reference_run(golden, mode):
    """BASELINE config 4's "bf16": option train_bf16 rounds the GEMM operands to bf16 (f32 accumulation, everything else f32).
    Against the reference's f32 train-step goldens the tolerances are bf16's: 2^-8 relative per operand, i.e. ~1e-2 on the
    unit-norm embeddings' elements after the stack of layers, ~1e-2 relative on the loss, and gradient tensors that agree
    in direction (cosine) and norm to a few percent."""
    from text2loc_amd.engine import Engine

    g = golden(f"train_step_{mode}")
    cells, sd, embed = load_case(g, mode)
    e = Engine(0)
    try:
        e.set_option("train_bf16", 1)
        tensors = bind(e, sd, embed)
        dcells = to_dev(cells, embed)
        positive = e.encode_cells_train(dcells, dropout_p=0.0, seed=0)
        err = np.abs(positive.cpu().numpy() - g["positive"]).max()
        assert 1e-6 < err < 2e-2, err  # really bf16 (not the f32 path), and within bf16's reach
        anchor = torch.from_numpy(g["anchor"]).cuda()
        loss, ga, gp = e.contrastive_loss(anchor, positive, float(g["temperature"]))
        assert abs(float(loss) - float(g["loss"])) < 2e-2 * abs(float(g["loss"]))
        e.encode_cells_backward(gp)
        torch.cuda.synchronize()
        worst_cos, n_checked = 1.0, 0
        for n in [str(x) for x in g["used_params"]]:
            exp, got = golden_view(g, "grad", n, tensors[n][1].cpu().numpy())
            ref_norm = float(g[f"grad_norm/{n}"])
            if ref_norm < 1e-4 or got.shape != exp.shape or tensors[n][1].numel() < 4096:
                continue  # zero-gradient tensors (Linear biases in front of BatchNorm), sampled views, and the small tensors
                          # whose true gradient is a cancellation residue ([64,1] / [64,3] Linears in front of a BatchNorm)
            cos = float((got * exp).sum() / (np.linalg.norm(got) * np.linalg.norm(exp) + 1e-30))
            worst_cos = min(worst_cos, cos)
            n_checked += 1
            assert abs(float(np.linalg.norm(tensors[n][1].cpu().numpy())) - ref_norm) < 0.1 * ref_norm, n
        assert n_checked >= 10 and worst_cos > 0.98, (n_checked, worst_cos)
        e.adam_step(float(g["lr"]))
        torch.cuda.synchronize()
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["embed", "pn"])
def test_split_bf16_variant_stays_at_f32_accuracy(golden, mode):
    """train_bf16 = 2: every GEMM operand as hi + lo bf16, three MFMAs per 16-step (relative product error <= 2^-16 + 2^-18,
    f32's exponent range): the reference's f32 goldens are met to ~1e-5 — two orders closer than the plain bf16 variant —
    while the matrix pipe does 2.7x less work than with f32 MFMAs."""
    from text2loc_amd.engine import Engine

    g = golden(f"train_step_{mode}")
    cells, sd, embed = load_case(g, mode)
    e = Engine(0)
    try:
        e.set_option("train_bf16", 2)
        tensors = bind(e, sd, embed)
        dcells = to_dev(cells, embed)
        positive = e.encode_cells_train(dcells, dropout_p=0.0, seed=0)
        err = np.abs(positive.cpu().numpy() - g["positive"]).max()
        assert err < 1e-4, err
        anchor = torch.from_numpy(g["anchor"]).cuda()
        loss, ga, gp = e.contrastive_loss(anchor, positive, float(g["temperature"]))
        assert abs(float(loss) - float(g["loss"])) < 2e-4 * abs(float(g["loss"])) + 1e-6
        e.encode_cells_backward(gp)
        torch.cuda.synchronize()
        worst_cos, n_checked = 1.0, 0
        for n in [str(x) for x in g["used_params"]]:
            exp, got = golden_view(g, "grad", n, tensors[n][1].cpu().numpy())
            ref_norm = float(g[f"grad_norm/{n}"])
            if ref_norm < 1e-4 or got.shape != exp.shape or tensors[n][1].numel() < 4096:
                continue
            cos = float((got * exp).sum() / (np.linalg.norm(got) * np.linalg.norm(exp) + 1e-30))
            worst_cos = min(worst_cos, cos)
            n_checked += 1
            assert abs(float(np.linalg.norm(tensors[n][1].cpu().numpy())) - ref_norm) < 5e-3 * ref_norm, n
        assert n_checked >= 10 and worst_cos > 0.9999, (n_checked, worst_cos)
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["embed", "pn"])
def test_gemm_block_64_equals_32(eng, golden, mode):
    """The 64 x 64-block form of the tile GEMMs (2 x 2 accumulator tiles per wave; the default with bf16 operands) against the
    32 x 32 form in float32 on the reference's train-step case: forward, loss gradients and every parameter gradient agree to
    float32 summation order (the same products, partial sums met in a different order)."""
    g = golden(f"train_step_{mode}")
    cells, sd, embed = load_case(g, mode)
    res = {}
    try:
        for blk in (32, 64):
            eng.set_option("train_gemm_block", blk)
            tensors = bind(eng, sd, embed)
            positive = eng.encode_cells_train(to_dev(cells, embed), dropout_p=0.1, seed=5)
            anchor = torch.from_numpy(g["anchor"]).cuda()
            loss, ga, gp = eng.contrastive_loss(anchor, positive, float(g["temperature"]))
            eng.encode_cells_backward(gp)
            torch.cuda.synchronize()
            res[blk] = (positive.clone(), {n: t[1].clone() for n, t in tensors.items() if t[1] is not None})
    finally:
        eng.set_option("train_gemm_block", 0)
    assert float((res[32][0] - res[64][0]).abs().max()) < 2e-6
    for n, a in res[32][1].items():
        b = res[64][1][n]
        if n.startswith("object_encoder.") and n.endswith(".0.bias"):
            continue  # in front of a BatchNorm: noise around a zero gradient
        assert float((a - b).norm()) <= 2e-4 * float(a.norm()) + 1e-9, n
