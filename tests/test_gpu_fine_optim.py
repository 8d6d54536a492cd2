"""GPU tier of the fine stage's optimizer on the engine: t2l_fine_adam_step / t2l_fine_zero_grad / t2l_fine_adam_state against the
reference's own post-Adam parameters (the goldens of tests/test_gpu_fine_train.py) and the oracle's Adam arithmetic, and
``text2loc_amd.optim.Adam(CrossMatch)`` against ``torch.optim.Adam(model.parameters())``: steps, checkpoints, re-binds."""
import copy

import numpy as np
import pytest
import torch

from oracle import t2l_oracle_train as OT
from tests.test_gpu_fine_train import ALL, bind, drop_in
from tests.test_oracle_fine_train import fine_args, golden_case, problem
from tests.test_oracle_train import golden_view
from text2loc_amd import optim
from text2loc_amd.engine import T2LError

pytestmark = pytest.mark.gpu
BACKBONE = "object_encoder.pointnet."
# a Linear in front of a BatchNorm: the true gradient of its bias is 0 and num_encoder's [64,1] weight keeps an eps residual, so
# Adam's first step (lr * sign(grad)) is decided by float32 noise there — the exclusions of test_step_matches_the_reference_goldens
NOISE = (".0.bias", "num_encoder.0.0.weight")


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def forward_backward(eng, cells, hints, pn, gout):
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    h = torch.from_numpy(hints).cuda()
    pnt = None if pn is None else torch.from_numpy(pn).cuda()
    out = eng.fine_train_forward(packed, pnt, h, dropout_p=0.0, seed=0)
    eng.fine_train_backward(gout(out) if callable(gout) else torch.from_numpy(gout).cuda())
    torch.cuda.synchronize()
    return packed, h, pnt  # (the engine reads them until the last backward)


def trained(tensors):
    return [n for n, (_, g) in tensors.items() if g is not None]


@pytest.mark.parametrize("name", ["embed", "pn", "embed_l0"])
def test_engine_step_reproduces_the_reference_adam(eng, golden, name):
    """One engine step from the reference's batch lands on the reference's post-Adam parameters (the goldens' param/ fields; 2e-5
    where the reference's gradient is live); a second step follows oracle.t2l_oracle_train.adam_step on the engine's own gradients."""
    g = golden(f"fine_train_{name}")
    embed, L, sd, cells, pn = golden_case(g)
    tensors = bind(eng, sd, embed, ALL, L)
    lr = float(g["lr"])
    target = torch.from_numpy(g["targets"]).cuda()

    def mse_grad(out):
        o = out.detach().clone().requires_grad_(True)
        (float(g["offset_lambda"]) * torch.nn.MSELoss()(o, target)).backward()
        return o.grad.contiguous()

    names = trained(tensors)
    state = {n: (tensors[n][0].cpu().numpy().astype(np.float64), 0.0, 0.0) for n in names}
    for step in (1, 2):
        eng.fine_zero_grad()
        keep = forward_backward(eng, cells, g["hint_encodings"], pn, mse_grad)
        grads = {n: tensors[n][1].cpu().numpy().astype(np.float64) for n in names}
        eng.fine_adam_step(lr)
        torch.cuda.synchronize()
        del keep
        for n in names:
            state[n] = OT.adam_step(state[n][0], grads[n], state[n][1], state[n][2], step, lr)
            ok = np.abs(grads[n]) > 1e-6  # (elsewhere the update sits on Adam's eps knee)
            got = tensors[n][0].cpu().numpy()
            assert np.abs(got - state[n][0])[ok].max(initial=0.0) < 5e-6, (n, step)
        if step == 1:
            for n in [str(x) for x in g["used_params"]]:
                if n.startswith("object_encoder.") and n.endswith(NOISE):
                    continue
                q = tensors[n][0].cpu().numpy()
                exp, got = golden_view(g, "param", n, q)
                gexp, _ = golden_view(g, "grad", n, q)
                big = np.abs(gexp) > 1e-2 * float(g[f"grad_norm/{n}"]) / np.sqrt(q.size)
                assert np.abs(got - exp)[big].max(initial=0.0) < 2e-5, n
    m, v, packed_step = eng.fine_adam_state()
    assert packed_step == 2 and m.numel() == sum(tensors[n][0].numel() for n in names)
    off = 0
    for n in names:  # the moments: bind order (no backbone here)
        k = tensors[n][0].numel()
        assert np.abs(m[off:off + k].cpu().numpy() - np.ravel(state[n][1])).max() < 1e-6 * max(1.0, np.abs(state[n][1]).max()), n
        off += k


def test_zero_grad_and_step_leave_frozen_tensors_and_buffers_alone(eng):
    sd, cells, hints, pn, gout = problem(True, 2)
    tensors = {}
    frozen = ("mlp_offsets.0.weight", "cross_hints.1.norm2.bias", "object_encoder.pos_encoder.0.0.weight")
    for k, v in sd.items():
        if k.startswith(("language_encoder.", BACKBONE)) or k.endswith("num_batches_tracked"):
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if ("running_" in k or k in frozen) else torch.full_like(t, 3.0))
    eng.fine_train_bind(tensors, class_embed=True, color_embed=True, use_features=ALL, num_layers=2)
    ptrs = {n: g.data_ptr() for n, (_, g) in tensors.items() if g is not None}
    before = {n: t.clone() for n, (t, g) in tensors.items() if g is None}
    eng.fine_zero_grad()
    torch.cuda.synchronize()
    for n, (t, g) in tensors.items():
        if g is not None:
            assert g.data_ptr() == ptrs[n] and not bool(g.any()), n
    assert all(torch.equal(tensors[n][0], b) for n, b in before.items())
    m, v, step = eng.fine_adam_state()
    assert step == 0 and m.numel() == sum(t.numel() for t, g in tensors.values() if g is not None)
    for _, g in tensors.values():
        if g is not None:
            g.fill_(0.25)
    w0 = {n: t.clone() for n, (t, g) in tensors.items() if g is not None}
    eng.fine_adam_step(1e-3)
    torch.cuda.synchronize()
    assert all(torch.equal(tensors[n][0], b) for n, b in before.items())  # frozen parameters and running buffers: in neither call
    for n, w in w0.items():  # Adam's first step is lr * sign(grad)
        assert float((tensors[n][0] - (w - 1e-3)).abs().max()) < 1e-6, n
    assert all(float((g - 0.25).abs().max()) == 0.0 for _, g in tensors.values() if g is not None)  # the step reads the gradients only


def test_a_step_before_any_bind_is_refused():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    try:
        for call in (e.fine_zero_grad, lambda: e.fine_adam_step(1e-3), e.fine_adam_state):
            with pytest.raises(T2LError, match="t2l_fine_train_bind first"):
                call()
        sd, _, _, _, _ = problem(True, 2)
        bind(e, sd, True, ALL, 2)
        with pytest.raises(T2LError, match="beta"):
            e.fine_adam_step(1e-3, beta1=1.0)
    finally:
        e.close()


def test_rebind_keeps_or_resets_the_moments_and_a_refused_bind_changes_nothing(eng):
    sd, cells, hints, pn, gout = problem(True, 2)
    tensors = bind(eng, sd, True, ALL, 2)
    keep = forward_backward(eng, cells, hints, pn, gout)
    eng.fine_adam_step(1e-3)
    m0, v0, step0 = eng.fine_adam_state()
    assert step0 == 1 and float(m0.abs().max()) > 0
    # one tensor mis-sized: refused, and the binding with its moments stands
    bad = dict(tensors)
    w = tensors["mlp_offsets.2.weight"][0]
    bad["mlp_offsets.2.weight"] = (w[:1].contiguous(), torch.zeros_like(w[:1]))
    with pytest.raises(T2LError, match="mlp_offsets.2.weight"):
        eng.fine_train_bind(bad, class_embed=True, color_embed=True, use_features=ALL, num_layers=2)
    m1, v1, step1 = eng.fine_adam_state()
    assert step1 == 1 and torch.equal(m1, m0) and torch.equal(v1, v0)
    eng.fine_adam_step(1e-3)  # ... and still steps the tensors it was bound to
    assert eng.fine_adam_state()[2] == 2
    m2, v2, _ = eng.fine_adam_state()
    # the same list on moved storage
    moved = {n: (t.clone(), None if g is None else g.clone()) for n, (t, g) in tensors.items()}
    eng.set_option("train_keep_adam_state", 1)
    eng.fine_train_bind(moved, class_embed=True, color_embed=True, use_features=ALL, num_layers=2)
    m3, v3, step3 = eng.fine_adam_state()
    assert step3 == 2 and torch.equal(m3, m2) and torch.equal(v3, v2)
    # a different list (one more frozen tensor) under the option, and the same list without it: both start over
    fewer = dict(moved)
    fewer["mlp_offsets.0.bias"] = (moved["mlp_offsets.0.bias"][0], None)
    eng.fine_train_bind(fewer, class_embed=True, color_embed=True, use_features=ALL, num_layers=2)
    m4, _, step4 = eng.fine_adam_state()
    assert step4 == 0 and m4.numel() == m3.numel() - 64 and not bool(m4.any())
    eng.fine_adam_step(1e-3)
    eng.set_option("train_keep_adam_state", 0)
    eng.fine_train_bind(fewer, class_embed=True, color_embed=True, use_features=ALL, num_layers=2)
    m5, v5, step5 = eng.fine_adam_state()
    assert step5 == 0 and not bool(m5.any()) and not bool(v5.any())
    del keep


# ---- model level: optim.Adam(CrossMatch) ---------------------------------------------------------------------------------------
class Pose:
    def __init__(self, xy):
        self.pose = np.array([xy[0], xy[1], 0.0])


def test_optim_adam_in_train_epoch_halves_the_loss():
    from text2loc_amd.fine_training import eval_epoch, train_epoch

    torch.manual_seed(0)
    model, objects, texts, pts, target = drop_in()
    batch = {"objects": objects, "texts": texts, "offsets": target, "poses": [Pose(t) for t in target], "object_points": pts}
    opt = optim.Adam(model, lr=3e-3)
    assert isinstance(opt, optim.FineAdam) and isinstance(opt, optim.Adam) and isinstance(opt, torch.optim.Optimizer)
    kinds = [g["t2l_engine"] for g in opt.param_groups]
    assert kinds == [True, False]  # the engine's parameters; the stand-in text branch's table (and what never gets a gradient)
    args = fine_args(True)
    losses = [train_epoch(model, [batch], args, opt, torch.nn.MSELoss())["loss"] for _ in range(12)]
    assert losses[-1] < 0.5 * losses[0], losses
    flat = model.train_flat_grad()
    assert flat is not None and flat.numel() % 64 == 0
    lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
    for n, q in model.named_parameters():
        if model.engine_steps(n, q):
            assert q.grad is not None and lo <= q.grad.data_ptr() < hi and (q.grad.data_ptr() - lo) % 256 == 0, n
    assert eval_epoch(model, [batch], args)["pose_offsets"] >= 0.0  # the eval path re-loaded the stepped weights


def step_with_grads_of(model, opt, followers, objects, texts, pts, target, seed):
    """One step of all: the gradients come from ``model``'s engine step and are copied to the ``followers`` [(model, optimizer)], so
    what is compared is the optimizers' arithmetic and bookkeeping, not the float atomics of several backward passes."""
    for o in [opt] + [o for _, o in followers]:
        o.zero_grad()
    torch.manual_seed(seed)
    torch.nn.functional.mse_loss(model(objects, texts, pts), target).backward()
    for other, _ in followers:
        for (n, q), (_, r) in zip(model.named_parameters(), other.named_parameters()):
            r.grad = None if q.grad is None else q.grad.detach().clone()
    for o in [opt] + [o for _, o in followers]:
        o.step()


def assert_same_parameters(model, twin, bound=2e-5):
    for (n, q), (_, r) in zip(model.named_parameters(), twin.named_parameters()):
        assert float((q.detach() - r.detach()).abs().max()) < bound, n


def test_two_steps_match_torch_adam_on_a_twin():
    model, objects, texts, pts, target = drop_in()
    twin = drop_in()[0]
    twin.load_state_dict(model.state_dict())  # (the fixture leaves what this configuration never runs at its random initialisation)
    tgt = torch.from_numpy(target).cuda()
    model.train(), twin.train()
    opt, topt = optim.Adam(model, lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3)
    w0 = {n: q.detach().clone() for n, q in model.named_parameters()}
    for seed in (1, 2):
        step_with_grads_of(model, opt, [(twin, topt)], objects, texts, pts, tgt, seed)
        assert_same_parameters(model, twin)
    moved = {n for n, q in model.named_parameters() if not torch.equal(q.detach(), w0[n])}
    assert "cross_objects.0.linear1.weight" in moved and "language_encoder.table" in moved
    assert "object_encoder.color_encoder.0.0.weight" not in moved  # color_embed: never runs, never steps


def test_state_dict_round_trips_with_torch_adam():
    """A checkpoint of either optimizer loads into the other, and the third step after a reload is the third step without one."""
    model, objects, texts, pts, target = drop_in()
    twin = drop_in()[0]
    twin.load_state_dict(model.state_dict())  # (the fixture leaves what this configuration never runs at its random initialisation)
    tgt = torch.from_numpy(target).cuda()
    model.train(), twin.train()
    opt, topt = optim.Adam(model, lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3)
    for seed in (1, 2):
        step_with_grads_of(model, opt, [(twin, topt)], objects, texts, pts, tgt, seed)
    # (copies, as a checkpoint on disk is: torch's load_state_dict aliases the tensors it is handed when device and dtype already fit)
    sd, tsd = copy.deepcopy(opt.state_dict()), copy.deepcopy(topt.state_dict())
    assert sorted(sd["state"]) == sorted(tsd["state"]) and len(sd["param_groups"]) == 1
    assert sd["param_groups"][0]["params"] == tsd["param_groups"][0]["params"]
    for i, e in tsd["state"].items():
        assert float(sd["state"][i]["step"]) == float(e["step"]) == 2.0
        assert float((sd["state"][i]["exp_avg"] - e["exp_avg"]).abs().max()) < 1e-6 * max(1.0, float(e["exp_avg"].abs().max())), i
    # fresh models at the stepped weights; each optimizer takes the OTHER one's checkpoint
    model2, twin2 = drop_in()[0], drop_in()[0]
    model2.load_state_dict(twin.state_dict())
    twin2.load_state_dict(model.state_dict())
    model2.train(), twin2.train()
    opt2, topt2 = optim.Adam(model2, lr=5e-2), torch.optim.Adam(twin2.parameters(), lr=1e-3)
    opt2.load_state_dict(tsd)
    topt2.load_state_dict(sd)
    assert all(g["lr"] == 1e-3 for g in opt2.param_groups)
    # the third step, without a reload (model, twin) and after one (model2, twin2), all four on model's gradients
    step_with_grads_of(model, opt, [(twin, topt), (model2, opt2), (twin2, topt2)], objects, texts, pts, tgt, 3)
    assert_same_parameters(twin, model)
    assert_same_parameters(model2, model, 5e-6)
    assert_same_parameters(twin2, model, 2e-5)
    with pytest.raises(ValueError, match="not a checkpoint"):
        opt2.load_state_dict({"state": {}, "param_groups": [dict(tsd["param_groups"][0], params=[0, 1])]})


def test_model_to_and_set_to_none_keep_the_moments():
    model, objects, texts, pts, target = drop_in()
    tgt = torch.from_numpy(target).cuda()
    model.train()
    opt = optim.Adam(model, lr=1e-3)

    def step(seed):
        opt.zero_grad()
        torch.manual_seed(seed)
        torch.nn.functional.mse_loss(model(objects, texts, pts), tgt).backward()
        opt.step()

    step(1)
    eng = model._fine_train_engine()
    m1, v1, s1 = eng.fine_adam_state()
    assert s1 == 1
    model.zero_grad(set_to_none=True)  # drops the references: the bound buffers come back with the next bind
    for q in model.parameters():  # moved storage, as model.to() leaves it
        q.data = q.data.clone()
    model._fine_train_grads, model._fine_train_flat = {}, None  # ... gradient buffers included
    eng2 = model._fine_train_engine()
    assert eng2 is eng
    m2, v2, s2 = eng.fine_adam_state()
    assert s2 == 1 and torch.equal(m2, m1) and torch.equal(v2, v1)
    step(2)
    assert eng.fine_adam_state()[2] == 2
    # without the option the same re-bind starts over (what a first bind of another model under the same names must get)
    model._fine_train_grads, model._fine_train_flat = {}, None
    model._fine_train_bound = None
    model._fine_train_engine()
    m3, _, s3 = eng.fine_adam_state()
    assert s3 == 0 and not bool(m3.any())


def test_a_replaced_parameter_is_the_one_that_trains():
    """``module.weight = nn.Parameter(...)`` between two steps: the next forward binds the module's CURRENT tensors, so the new one is
    differentiated and stepped (its moments start over: another tensor under the same name); the orphan stays as it was."""
    model, objects, texts, pts, target = drop_in()
    tgt = torch.from_numpy(target).cuda()
    model.train()
    opt = optim.Adam(model, lr=1e-3)
    assert opt._grad_reduce == "mean"  # the fine loss is a mean over the local rows

    def step():
        opt.zero_grad()
        torch.manual_seed(1)
        torch.nn.functional.mse_loss(model(objects, texts, pts), tgt).backward()
        opt.step()

    model.train()
    step()
    lin = model.cross_hints[1].linear2
    old = lin.weight
    lin.weight = torch.nn.Parameter(old.detach().clone())
    new, before = lin.weight, old.detach().clone()
    step()  # (the same optimizer: the engine steps what the model's bind walks, not a list of parameter objects)
    assert torch.equal(old.detach(), before)  # the orphan: neither read for the step nor stepped
    assert new.grad is not None and float(new.grad.abs().max()) > 0
    assert float((new.detach() - before).abs().max()) > 1e-4  # lr * sign(grad) on the tensor the module holds now
    model.eval()
    with torch.no_grad():
        a = model(objects, texts, pts)
        lin.weight.copy_(before)
        model._train_generation += 1
        b = model(objects, texts, pts)
    assert float((a - b).abs().max()) > 0  # the eval path reads the same tensor the step moved


def test_point_batches_step_the_backbone_unless_frozen():
    from tests.test_gpu_fine_train_points import backbone_params, model_problem

    B = 3
    model, objects, texts, batches, target, _ = model_problem(B)
    opt = optim.Adam(model, lr=1e-3)
    w0 = {n: q.detach().clone() for n, q in model.named_parameters()}
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, batches), target).backward()
    opt.step()
    bp = backbone_params(model)
    moved = {n for n, q in model.named_parameters() if not torch.equal(q.detach(), w0[n])}
    assert {n for n in bp if n.endswith(".weight")} <= moved
    assert not any("classifier" in n for n in moved)
    eng = model._fine_train_engine()
    m, _, step = eng.fine_adam_state()
    assert step == 1 | (1 << 32)
    n_bb = sum(q.numel() for q in bp.values())
    assert float(m[-n_bb:].abs().max()) > 0  # the backbone's group: behind the rest
    # a step fed features2 leaves the backbone's weights AND moments alone (torch skips a .grad of None), and its count behind
    feats = [torch.from_numpy(np.abs(np.random.default_rng(i).standard_normal((16, 256))).astype(np.float32)).cuda() for i in range(B)]
    w1 = {n: q.detach().clone() for n, q in bp.items()}
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, feats), target).backward()
    opt.step()
    m2, _, step2 = eng.fine_adam_state()
    assert step2 == 2 | (1 << 32) and torch.equal(m2[-n_bb:], m[-n_bb:])
    assert all(torch.equal(q.detach(), w1[n]) for n, q in bp.items())
    sd = opt.state_dict()  # per-parameter steps, as torch.optim.Adam keeps them
    names = [n for n, _ in model.named_parameters()]
    assert float(sd["state"][names.index(BACKBONE + "lin2.weight")]["step"]) == 1.0
    assert float(sd["state"][names.index("mlp_offsets.0.weight")]["step"]) == 2.0
    # --pointnet_freeze: forward only, not in the moments
    frozen, _, _, _, _, _ = model_problem(B, freeze=True)
    fopt = optim.Adam(frozen, lr=1e-3)
    f0 = {n: q.detach().clone() for n, q in backbone_params(frozen).items()}
    fopt.zero_grad()
    torch.nn.functional.mse_loss(frozen(objects, texts, batches), target).backward()
    fopt.step()
    assert all(torch.equal(q.detach(), f0[n]) for n, q in backbone_params(frozen).items())
    mf, _, stepf = frozen._fine_train_engine().fine_adam_state()
    assert stepf == 1 and mf.numel() == m.numel() - n_bb
