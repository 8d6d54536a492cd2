"""GPU tier of the fine stage's training step (t2l_fine_train_*, CrossMatch under model.train()) against the float64 twin
(tests/fine_train_twin.py), which tests/test_oracle_fine_train.py pins to torch's own modules."""
import numpy as np
import pytest
import torch

from tests.fine_train_twin import Twin
from tests.test_oracle_fine_train import fine_args, golden_case, grad_errors, problem
from tests.test_oracle_train import golden_view
from text2loc_amd import synth

pytestmark = pytest.mark.gpu
ALL = ("class", "color", "position", "num")


def bind(eng, sd, embed, use, L):
    tensors = {}
    for k, v in sd.items():
        if k.startswith(("language_encoder.", "object_encoder.pointnet.")) or k.endswith("num_batches_tracked"):
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.fine_train_bind(tensors, class_embed=embed, color_embed=embed, use_features=use, num_layers=L)
    return tensors


def engine_step(eng, cells, hints, pn, gout, p, seed):
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    h = torch.from_numpy(hints).cuda()
    pnt = None if pn is None else torch.from_numpy(pn).cuda()
    off = eng.fine_train_forward(packed, pnt, h, dropout_p=p, seed=seed)
    gh = torch.empty_like(h)
    gp = None if pn is None else torch.empty_like(pnt)
    eng.fine_train_backward(torch.from_numpy(gout).cuda(), gh, gp)
    torch.cuda.synchronize()
    return off.cpu().numpy(), gh.cpu().numpy(), None if gp is None else gp.cpu().numpy()


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.sqrt((b ** 2).mean()), 1e-30))


def check_grads(tensors, ref, tol=2e-3):
    for n, g in ref.items():
        got = tensors[n][1].cpu().numpy()
        if n.startswith("object_encoder.") and n.endswith(".0.bias") and np.sqrt((g ** 2).mean()) < 1e-9:
            # Linear bias in front of a BatchNorm: true gradient 0, float32 leaves cancellation noise
            assert np.abs(got).max() < 1e-3 * max(1.0, np.abs(tensors[n.replace(".0.bias", ".1.bias")][1].cpu().numpy()).max()), n
            continue
        if n.endswith("num_encoder.0.0.weight"):  # scale-invariant [64,1] Linear before a BatchNorm: only an eps residual
            assert np.abs(got - g).max() < 2e-4, n
            continue
        assert rel(got, g) < tol, (n, rel(got, g))


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("mode,embed,L", [("embed", True, 2), ("pn", False, 2), ("embed_l0", True, 0)])
def test_step_matches_the_twin(eng, mode, embed, L):
    sd, cells, hints, pn, gout = problem(embed, L)
    tensors = bind(eng, sd, embed, ALL, L)
    off, gh, gp = engine_step(eng, cells, hints, pn, gout, 0.0, 0)
    twin = Twin(sd, embed, embed, ALL, L)
    off_t, g_t, gh_t, gp_t = twin.step(cells, hints, gout, pn)
    assert np.abs(off - off_t).max() < 1e-4
    assert rel(gh, gh_t) < 2e-3
    if not embed:
        assert rel(gp, gp_t) < 2e-3
    check_grads(tensors, g_t)
    for n, v in twin.running().items():
        assert np.abs(tensors[n][0].cpu().numpy() - v).max() < 1e-5 * max(1.0, np.abs(v).max()), n
    # torch.optim.Adam on the live tensors vs the same step on the twin's float64 parameters
    names = sorted(g_t)
    live = [torch.nn.Parameter(tensors[n][0]) for n in names]
    for q, n in zip(live, names):
        q.grad = tensors[n][1]
    torch.optim.Adam(live, lr=1e-3).step()
    ref = [torch.nn.Parameter(twin.t[n].detach().clone()) for n in names]
    for q, n in zip(ref, names):
        q.grad = torch.from_numpy(g_t[n])
    torch.optim.Adam(ref, lr=1e-3).step()
    for q, r, n in zip(live, ref, names):
        d = np.abs(q.detach().cpu().numpy() - r.detach().numpy())
        # Adam's first step is lr * sign(grad): an element whose true gradient is ~0 (the key part of in_proj_bias, a Linear
        # bias in front of a BatchNorm) may step either way; every other element must take the twin's step
        if n.startswith("object_encoder.") and n.endswith((".0.bias", "num_encoder.0.0.weight")):
            continue  # in front of a BatchNorm: true gradient 0 / an eps residual (check_grads bounds their noise)
        g = np.abs(g_t[n])
        live_mask = g > 1e-3 * max(np.sqrt((g ** 2).mean()), 1e-12)
        assert (d[live_mask] > 1e-5).mean() < 0.01 if live_mask.any() else True, (n, (d[live_mask] > 1e-5).mean())


@pytest.mark.parametrize("name", ["embed", "pn", "embed_l0"])
def test_step_matches_the_reference_goldens(eng, golden, name):
    """The reference's own CrossMatch step (tools/gen_golden_fine_train.py): offsets, offset_lambda * MSE, backward,
    running statistics and torch.optim.Adam."""
    g = golden(f"fine_train_{name}")
    embed, L, sd, cells, pn = golden_case(g)
    tensors = bind(eng, sd, embed, ALL, L)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    h = torch.from_numpy(g["hint_encodings"]).cuda()
    pnt = None if pn is None else torch.from_numpy(pn).cuda()
    out = eng.fine_train_forward(packed, pnt, h, dropout_p=0.0, seed=0)
    assert np.abs(out.cpu().numpy() - g["offsets_out"]).max() < 1e-4
    o = out.detach().clone().requires_grad_(True)
    loss = float(g["offset_lambda"]) * torch.nn.MSELoss()(o, torch.from_numpy(g["targets"]).cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4 * max(1.0, float(g["loss"]))
    gh = torch.empty_like(h)
    gp = None if pnt is None else torch.empty_like(pnt)
    eng.fine_train_backward(o.grad.contiguous(), gh, gp)
    torch.cuda.synchronize()
    assert rel(gh.cpu().numpy(), g["grad_hint"]) < 2e-3
    if gp is not None:
        assert rel(gp.cpu().numpy(), g["grad_pn"]) < 2e-3
    used = [str(x) for x in g["used_params"]]
    for n in used:
        full = tensors[n][1].cpu().numpy()
        err, rms = grad_errors(g, n, full)
        if n.startswith("object_encoder.") and n.endswith(".0.bias"):
            assert err < 1e-4, n  # true gradient 0 (a BatchNorm follows)
            continue
        if n.endswith("num_encoder.0.0.weight"):
            assert err < 2e-4, n  # scale-invariant [64,1] Linear before a BatchNorm: an eps residual
            continue
        assert err < 2e-3 * rms + 1e-9, (n, err, rms)
        assert abs(float(np.sqrt((full.astype(np.float64) ** 2).sum())) - float(g[f"grad_norm/{n}"])) < 2e-3 * float(g[f"grad_norm/{n}"]), n
    for k in g.files:
        if k.startswith("buf/"):
            assert np.allclose(tensors[k[4:]][0].cpu().numpy(), g[k], rtol=2e-4, atol=2e-5), k
    # torch.optim.Adam on the live tensors with the engine's gradients vs the reference's post-Adam parameters. Adam's first
    # step is lr * sign(grad): compare where the reference's gradient is clearly non-zero
    live = [torch.nn.Parameter(tensors[n][0]) for n in used]
    for q, n in zip(live, used):
        q.grad = tensors[n][1]
    torch.optim.Adam(live, lr=float(g["lr"])).step()
    for q, n in zip(live, used):
        exp, got = golden_view(g, "param", n, q.detach().cpu().numpy())
        gexp, _ = golden_view(g, "grad", n, q.detach().cpu().numpy())
        rms = float(g[f"grad_norm/{n}"]) / np.sqrt(q.numel())
        big = np.abs(gexp) > 1e-2 * rms
        if n.startswith("object_encoder.") and n.endswith((".0.bias", "num_encoder.0.0.weight")):
            continue
        assert np.abs(got - exp)[big].max(initial=0.0) < 2e-5, n


GRID = [(1, 3, 0, ALL, True), (5, 6, 1, ALL, False), (32, 8, 2, ALL, True), (33, 6, 4, ALL, True),
        (5, 3, 2, ("class", "position"), False), (32, 6, 1, ("color", "num"), True), (33, 8, 2, ALL, False),
        (5, 6, 1, ("color", "position"), False)]


@pytest.mark.parametrize("B,H,L,use,embed", GRID)
def test_dropout_step_matches_the_twin_replaying_the_masks(eng, B, H, L, use, embed):
    sd, cells, hints, pn, gout = problem(embed, L, P=B, H=H, seed=B + H, use=use)
    tensors = bind(eng, sd, embed, use, L)
    off, gh, gp = engine_step(eng, cells, hints, pn, gout, 0.1, 1234 + B)
    twin = Twin(sd, embed, embed, use, L)
    off_t, g_t, gh_t, gp_t = twin.step(cells, hints, gout, pn, p=float(np.float32(0.1)), seed=1234 + B)
    assert np.abs(off - off_t).max() < 1e-4
    assert rel(gh, gh_t) < 2e-3
    if gp_t is not None:
        assert rel(gp, gp_t) < 2e-3
    elif gp is not None:  # features2 fed mlp_pointnet's statistics only (class_embed off without "class")
        assert not np.any(gp)
    check_grads(tensors, g_t)


# ---------------------------------------------------------------------------------------------------------------
class HintParams(torch.nn.Module):
    """Text-branch stand-in with a trainable table: the hint encodings of pose i are row i; the index rides in the text."""

    def __init__(self, table):
        super().__init__()
        self.table = torch.nn.Parameter(torch.from_numpy(table))

    def forward(self, texts):
        import re

        return self.table[torch.as_tensor([int(re.search(r"q(\d+)x", t).group(1)) for t in texts], device=self.table.device)]


def drop_in(embed=True, B=6, H=6, seed=4):
    from tests.test_host_logic import make_objects
    from text2loc_amd.cross_matcher import CrossMatch, pad_objects

    args = fine_args(embed)
    cells = synth.make_cells(B, seed=seed, min_obj=3, max_obj=20)
    objects = [pad_objects(o) for o in make_objects(cells, seed)]
    rng = np.random.default_rng(seed)
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args,
                       language_encoder=HintParams(rng.standard_normal((B, H, 128)).astype(np.float32)))
    sd = synth.make_fine_weights(seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda()
    texts = [f"The pose is north of a red q{i}x." for i in range(B)]
    pts = None if embed else [torch.from_numpy(rng.standard_normal((16, 256)).astype(np.float32)).cuda() for _ in range(B)]
    target = rng.random((B, 2)).astype(np.float32)
    return model, objects, texts, pts, target


def test_train_epoch_lowers_the_loss():
    from text2loc_amd.fine_training import eval_epoch, train_epoch

    torch.manual_seed(0)
    model, objects, texts, pts, target = drop_in()

    class Pose:
        def __init__(self, xy):
            self.pose = np.array([xy[0], xy[1], 0.0])

    batch = {"objects": objects, "texts": texts, "offsets": target, "poses": [Pose(t) for t in target], "object_points": pts}
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    crit = torch.nn.MSELoss()
    args = fine_args(True)
    losses = [train_epoch(model, [batch], args, opt, crit)["loss"] for _ in range(12)]
    assert set(train_epoch(model, [batch], args, opt, crit)) == {"loss", "loss_offsets", "pose_offsets"}
    assert losses[-1] < 0.5 * losses[0], losses
    assert eval_epoch(model, [batch], args)["pose_offsets"] >= 0.0


def test_drop_in_gradient_semantics():
    torch.manual_seed(0)
    model, objects, texts, pts, target = drop_in(embed=False)
    model.mlp_offsets[0].weight.requires_grad_(False)
    model.train()
    tgt = torch.from_numpy(target).cuda()

    def step(seed):
        torch.manual_seed(seed)
        out = model(objects, texts, pts)
        torch.nn.functional.mse_loss(out, tgt).backward()

    step(1)
    assert model.mlp_offsets[0].weight.grad is None  # frozen: no gradient
    assert model.object_encoder.class_embedding.weight.grad is None  # not part of this configuration: untouched, as in the reference
    g1 = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
    assert "language_encoder.table" in g1 and "cross_hints.1.linear2.weight" in g1 and "object_encoder.mlp_pointnet.0.0.weight" in g1
    assert float(g1["language_encoder.table"].abs().max()) > 0
    step(1)  # no zero_grad in between: every gradient doubles
    for n, q in model.named_parameters():
        if n in g1:
            assert torch.allclose(q.grad, 2 * g1[n], rtol=1e-4, atol=1e-6 * float(g1[n].abs().max())), n
    model.zero_grad(set_to_none=True)
    step(1)  # zero_grad(set_to_none=True): the bound buffers come back, zeroed
    for n, q in model.named_parameters():
        if n in g1:
            assert torch.allclose(q.grad, g1[n], rtol=1e-4, atol=1e-6 * float(g1[n].abs().max())), n
    # features2 supplied as leaves receive their gradient through autograd
    leaves = [p.detach().clone().requires_grad_(True) for p in pts]
    model(objects, texts, leaves).sum().backward()
    assert all(l.grad is not None and float(l.grad.abs().max()) > 0 for l in leaves)
    # a backward of an older forward is refused
    a = model(objects, texts, pts)
    model(objects, texts, pts)
    with pytest.raises(Exception, match="stale"):
        a.sum().backward()


def test_eval_after_a_step_sees_the_new_weights_and_statistics():
    from text2loc_amd import packing

    torch.manual_seed(0)
    model, objects, texts, pts, target = drop_in()
    model.eval()
    before = model(objects, texts, pts).cpu().numpy()  # loads the eval weights once
    model.train()
    nbt = int(model.object_encoder.pos_encoder[0][1].num_batches_tracked)
    nbt_unused = int(model.object_encoder.color_encoder[0][1].num_batches_tracked)  # color_embed on: color_encoder never runs
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, pts), torch.from_numpy(target).cuda()).backward()
    opt.step()
    assert int(model.object_encoder.pos_encoder[0][1].num_batches_tracked) == nbt + 1
    assert int(model.object_encoder.color_encoder[0][1].num_batches_tracked) == nbt_unused
    assert model.object_encoder.color_encoder[0][0].weight.grad is None
    model.eval()
    after = model(objects, texts, pts).cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if not k.startswith("language_encoder.")}
    twin = Twin(sd, True, True, ALL, 2)
    cells = packing.pack_cells(objects, model.object_encoder.known_classes, model.object_encoder.known_colors)
    hints = torch.from_numpy(model.language_encoder.table.detach().cpu().numpy().astype(np.float64))
    ref = twin.forward(cells, hints, train=False).detach().numpy()
    assert np.abs(after - ref).max() < 1e-4 and np.abs(after - before).max() > 1e-3
