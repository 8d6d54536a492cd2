"""GPU tier: the fine stage's training step with the PointNet++ backbone trained jointly (the published fine command: no
--class_embed, no --pointnet_freeze) — t2l_fine_train_forward_points / t2l_fine_train_backward and CrossMatch.train() on point
batches — against the float64 chain built from the committed restatements:
oracle/t2l_oracle_pointnet_train.py (backbone, per-cell BatchNorm) -> tests/fine_train_twin.py (fine step, dropout masks
replayed) -> the backbone's backward. PARITY of the backbone with torch_geometric stays UNPINNED, as for the coarse stage's:
what is checked is self-consistency of the HIP kernels with the build's own restatement."""
import numpy as np
import pytest
import torch

from oracle import t2l_oracle_pointnet as OP
from oracle import t2l_oracle_pointnet_train as OPT
from tests.fine_train_twin import Twin
from tests.test_gpu_fine_train import HintParams, check_grads, rel
from tests.test_oracle_fine_train import fine_args
from text2loc_amd import packing, synth
from text2loc_amd.engine import T2LError

pytestmark = pytest.mark.gpu
ALL = ("class", "color", "position", "num")
P = "object_encoder.pointnet."
H = 6


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def weights(seed, L, use=ALL):
    sd = dict(synth.make_fine_weights(seed, num_layers=L))
    sd["object_encoder.mlp_merge.0.0.weight"] = np.ascontiguousarray(sd["object_encoder.mlp_merge.0.0.weight"][:, :128 * len(use)])
    sd.update(synth.make_pointnet_weights(seed))
    return sd


def scene(B, seed):
    """B padded cells of 16 objects (pads included), their packed arrays and per-cell point batches ("fixed" FixedPoints)."""
    from tests.test_host_logic import make_objects
    from text2loc_amd.cross_matcher import pad_objects

    cells = synth.make_cells(B, seed=seed, min_obj=3, max_obj=20)
    objects = [pad_objects(o) for o in make_objects(cells, seed)]
    packed = packing.pack_cells(objects, packing.class_table(synth.KNOWN_CLASS), packing.color_table())
    batches = packing.sample_object_points(objects, 256, np.random.default_rng(seed + 1), "fixed")
    pos = np.concatenate([b["pos"] for b in batches]).reshape(-1, 256, 3)
    rgb = np.concatenate([b["x"] for b in batches]).reshape(-1, 256, 3)
    return objects, packed, batches, pos, rgb


def backbone_ratios(grad_of, ref, min_tight=10):
    """The criterion of test_gpu_pointnet_train.py::test_model_train_step_reaches_the_backbone: every ratio |err| / |ref| < 0.03,
    at least `min_tight` below 1e-3 (a float32 flip of a discrete decision moves what lies upstream of it by ~1 %)."""
    tight = 0
    for name, g in ref.items():
        got = grad_of(name)
        assert got is not None, name
        if name.endswith(".0.bias") and "lin" not in name:  # Linear bias in front of a BatchNorm: true gradient 0
            continue
        err = np.abs(got.cpu().numpy().astype(np.float64) - g)
        ratio = np.sqrt((err ** 2).sum()) / max(np.sqrt((g ** 2).sum()), 1e-30)
        assert ratio < 0.03, (name, ratio)
        tight += ratio < 1e-3
    assert tight >= min_tight, tight


def coarse_backbone_grads(eng, sd, pos, rgb, offs, grad_f2):
    """The coarse step's backbone (t2l_train_bind + t2l_pointnet_features_train + t2l_pointnet_backward) on the same weights,
    points, cells and upstream gradient -> its parameter gradients."""
    coarse = {}
    for k, v in list(synth.make_object_branch_weights(2).items()) + [(k, v) for k, v in sd.items() if k.startswith(P)]:
        if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight") or "classifier" in k:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        coarse[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(coarse, class_embed=False, color_embed=False)
    eng.pointnet_features_train(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), offs)
    eng.pointnet_backward(grad_f2)
    torch.cuda.synchronize()
    return {k: g for k, (_, g) in coarse.items() if k.startswith(P) and g is not None}


# ---- 1. the ABI step against the float64 chain ---------------------------------------------------------------------------
# (k shifts the scene's seed: with k = 0 the B = 1 case has a near-tie in the decoder whose side flips under a 3e-7
# perturbation of features2 — a float32 engine cannot be held to a float64 chain there)
@pytest.mark.parametrize("B,L,p,k", [(1, 2, 0.1, 1), (3, 0, 0.0, 0), (5, 2, 0.0, 0), (5, 0, 0.1, 0)])
def test_points_step_matches_the_float64_chain(eng, B, L, p, k):
    sd = weights(B, L)
    objects, cells, _, pos, rgb = scene(B, 40 + B + k)
    rng = np.random.default_rng(B + L + k)
    hints = rng.standard_normal((B, H, 128)).astype(np.float32)
    gout = rng.standard_normal((B, 2)).astype(np.float32)
    seed = 777 + B
    tensors = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or "classifier" in k:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.fine_train_bind(tensors, class_embed=False, color_embed=False, use_features=ALL, num_layers=L)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    h = torch.from_numpy(hints).cuda()
    off = eng.fine_train_forward_points(packed, torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), h, dropout_p=p, seed=seed)
    gh = torch.empty_like(h)
    gp = torch.empty(16 * B, 256, device="cuda")
    eng.fine_train_backward(torch.from_numpy(gout).cuda(), gh, gp)
    torch.cuda.synchronize()
    # the chain: backbone (train) -> fine step -> backbone backward
    offs = np.arange(0, 16 * B + 1, 16, dtype=np.int32)
    f2, _ = OPT.forward_backward(pos, rgb, offs, sd)
    twin = Twin(sd, False, False, ALL, L)
    off_t, g_t, gh_t, gp_t = twin.step(cells, hints, gout, f2, p=float(np.float32(p)), seed=seed)
    _, pinfo = OPT.forward_backward(pos, rgb, offs, sd, grad_f2=gp_t)
    assert np.abs(off.cpu().numpy() - off_t).max() < 1e-4
    assert rel(gh.cpu().numpy(), gh_t) < 2e-3
    assert rel(gp.cpu().numpy(), gp_t) < 2e-3
    check_grads(tensors, g_t)
    assert sorted(pinfo["grads"]) == sorted(k for k in tensors if k.startswith(P) and tensors[k][1] is not None)
    # Measured on these scenes (objects as sampled with the "fixed" transform: positions in the cell frame, not rescaled, plus
    # the pads' 8 points): lin1, lin2 and ga.mlp.1.1 agree to ~1e-5; below them the weight products sum dA·a over groups of
    # near-identical rows whose dA sums to 0 (a Linear in front of a BatchNorm), and float32 keeps 0.2-1 % of the true value.
    # The coarse step's own backbone scores exactly the same on these inputs (checked below), so the bound is the
    # kernels' float32 arithmetic on such rows, not the fine path; synth.make_sampled_points' normalised blobs give 27 of 28.
    backbone_ratios(lambda n: tensors[n][1], pinfo["grads"], min_tight=6)
    # the same backbone code as the coarse step: its gradients on the same points, cells and d features2 agree to atomics noise
    ref = coarse_backbone_grads(eng, sd, pos, rgb, offs, gp)
    for k, g in ref.items():
        if k.endswith(".0.bias") and "lin" not in k:
            continue
        assert float((tensors[k][1] - g).norm() / g.norm()) < 1e-4, k
    for k, v in pinfo["running"].items():  # once per pair, in pair order
        r = tensors[k][0].cpu().numpy().astype(np.float64)
        assert np.abs(r - v).max() < 2e-5 * max(1.0, np.abs(v).max()), (k, np.abs(r - v).max())
    for k, v in twin.running().items():
        assert np.abs(tensors[k][0].cpu().numpy() - v).max() < 1e-5 * max(1.0, np.abs(v).max()), k
    # a second backward of the same forward adds again: every gradient doubles
    one = {k: g.clone() for k, (_, g) in tensors.items() if g is not None}
    eng.fine_train_backward(torch.from_numpy(gout).cuda(), None, None)
    torch.cuda.synchronize()
    for k, v in one.items():
        if k.endswith(".0.bias") and "lin" not in k and "mlp_offsets" not in k:
            continue  # in front of a BatchNorm: float32 atomics noise around a true 0
        assert torch.allclose(tensors[k][1], 2 * v, rtol=1e-3, atol=1e-5 * float(v.abs().max()) + 1e-12), k


def test_the_fine_backbone_state_is_independent_of_the_coarse_step(eng):
    """The fine context's backbone state is its own: a coarse bind + backbone step between the fine forward and its backward
    changes nothing the fine backward computes."""
    L, B = 1, 2
    sd = weights(3, L)
    _, cells, _, pos, rgb = scene(B, 9)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    h = torch.from_numpy(np.random.default_rng(1).standard_normal((B, H, 128)).astype(np.float32)).cuda()
    gout = torch.ones(B, 2, device="cuda")

    def run(interleave):
        tensors = {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or "classifier" in k:
                continue
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
        eng.fine_train_bind(tensors, class_embed=False, color_embed=False, use_features=ALL, num_layers=L)
        off = eng.fine_train_forward_points(packed, dpos, drgb, h, dropout_p=0.0, seed=0)
        if interleave:
            coarse = {}
            for k, v in list(synth.make_object_branch_weights(2).items()) + list(synth.make_pointnet_weights(5).items()):
                if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight") or "classifier" in k:
                    continue
                t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
                coarse[k] = (t, None if "running_" in k else torch.zeros_like(t))
            eng.train_bind(coarse, class_embed=False, color_embed=False)
            cpos = dpos[:3].contiguous()
            eng.pointnet_features_train(cpos, drgb[:3].contiguous(), np.array([0, 1, 3], dtype=np.int32))
            eng.pointnet_backward(torch.randn(3, 256, device="cuda"))
        eng.fine_train_backward(gout, None, None)
        torch.cuda.synchronize()
        return off.cpu().numpy(), {k: g.cpu().numpy() for k, (_, g) in tensors.items() if g is not None and k.startswith(P)}

    off_a, g_a = run(False)
    off_b, g_b = run(True)
    assert np.abs(off_a - off_b).max() < 1e-6
    for k, v in g_a.items():
        if k.endswith(".0.bias") and "lin" not in k:
            continue
        assert np.abs(g_b[k] - v).max() <= 1e-4 * max(np.abs(v).max(), 1e-12), k


# ---- model level: CrossMatch.train() on point batches --------------------------------------------------------------------
class PointBatch:
    """A PyG ``Batch``-like cell batch: attributes .pos / .x."""

    def __init__(self, pos, x):
        self.pos, self.x = torch.from_numpy(pos), torch.from_numpy(x)


def model_problem(B=3, seed=4, freeze=False, use=ALL, L=2):
    from text2loc_amd.cross_matcher import CrossMatch

    args = fine_args(False, L, use)
    args.pointnet_freeze = freeze
    objects, cells, batches, pos, rgb = scene(B, seed)
    rng = np.random.default_rng(seed)
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args,
                       language_encoder=HintParams(rng.standard_normal((B, H, 128)).astype(np.float32)))
    sd = weights(seed, L, use)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda().train()
    texts = [f"The pose is north of a red q{i}x." for i in range(B)]
    target = torch.from_numpy(rng.random((B, 2)).astype(np.float32)).cuda()
    return model, objects, texts, batches, target, (cells, pos, rgb)


def backbone_params(model):
    return {n: q for n, q in model.named_parameters() if n.startswith(P) and "classifier" not in n}


def bn_tracked(model):
    pn = model.object_encoder.pointnet
    return int(pn.sa1.point_conv.local_nn[0][1].num_batches_tracked), int(pn.ga.mlp[1][1].num_batches_tracked), \
        int(model.object_encoder.pos_encoder[0][1].num_batches_tracked)


@pytest.mark.parametrize("kind", ["dict", "attr"])
def test_model_step_trains_the_backbone(kind):
    B = 3
    model, objects, texts, batches, target, _ = model_problem(B)
    if kind == "attr":
        batches = [PointBatch(b["pos"], b["x"]) for b in batches]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    nbt0 = bn_tracked(model)

    def step(seed):
        torch.manual_seed(seed)
        out = model(objects, texts, batches)
        torch.nn.functional.mse_loss(out, target).backward()
        return out

    opt.zero_grad()
    step(1)
    assert bn_tracked(model) == (nbt0[0] + B, nbt0[1] + B, nbt0[2] + 1)
    bp = backbone_params(model)
    assert len(bp) == 36  # sa1..sa3, ga: 8 x (Linear + BatchNorm) weight and bias; lin1, lin2
    assert all(q.grad is not None for q in bp.values())
    assert float(bp[P + "sa1.point_conv.local_nn.0.0.weight"].grad.abs().max()) > 0
    heads = [q for n, q in model.named_parameters() if "classifier" in n]
    assert heads and all(q.grad is None for q in heads)
    g1 = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
    step(1)  # no zero_grad in between: every gradient doubles, the backbone's included
    for n, q in model.named_parameters():
        if n not in g1 or (n.startswith("object_encoder.") and n.endswith(".0.bias") and "lin" not in n):
            continue
        assert torch.allclose(q.grad, 2 * g1[n], rtol=1e-3, atol=1e-5 * float(g1[n].abs().max()) + 1e-12), n
    model.zero_grad(set_to_none=True)
    assert all(q.grad is None for q in bp.values())
    step(1)  # the bound buffers come back zeroed
    for n, q in model.named_parameters():
        if n not in g1 or (n.startswith("object_encoder.") and n.endswith(".0.bias") and "lin" not in n):
            continue
        assert torch.allclose(q.grad, g1[n], rtol=1e-3, atol=1e-5 * float(g1[n].abs().max()) + 1e-12), n
    a = model(objects, texts, batches)
    model(objects, texts, batches)
    with pytest.raises(Exception, match="stale"):
        a.sum().backward()
    assert bn_tracked(model) == (nbt0[0] + 5 * B, nbt0[1] + 5 * B, nbt0[2] + 5)  # five training-mode forwards
    before = {n: q.detach().clone() for n, q in model.named_parameters() if n.startswith(P)}
    opt.step()
    moved = {n for n in before if not torch.equal(before[n], dict(model.named_parameters())[n].detach())}
    assert {n for n in bp if n.endswith(".weight")} <= moved, sorted({n for n in bp if n.endswith(".weight")} - moved)
    assert moved <= set(bp)  # sa1 ... lin2 move, the classifier heads do not


def test_pointnet_freeze_runs_the_backbone_forward_only():
    B = 3
    trained, objects, texts, batches, target, _ = model_problem(B)
    torch.manual_seed(1)
    out_t = trained(objects, texts, batches)
    frozen, _, _, _, _, _ = model_problem(B, freeze=True)
    rm0 = frozen.object_encoder.pointnet.sa2.point_conv.local_nn[1][1].running_mean.clone()
    w0 = {n: q.detach().clone() for n, q in backbone_params(frozen).items()}
    nbt0 = bn_tracked(frozen)
    opt = torch.optim.Adam(frozen.parameters(), lr=1e-3)
    opt.zero_grad()
    torch.manual_seed(1)
    out_f = frozen(objects, texts, batches)
    assert float((out_f - out_t).detach().abs().max()) < 1e-5  # the trainable model's first-step forward
    torch.nn.functional.mse_loss(out_f, target).backward()
    opt.step()
    assert all(q.grad is None for q in backbone_params(frozen).values())
    assert all(torch.equal(q.detach(), w0[n]) for n, q in backbone_params(frozen).items())
    assert frozen.cross_hints[0].linear1.weight.grad is not None
    assert not torch.equal(frozen.object_encoder.pointnet.sa2.point_conv.local_nn[1][1].running_mean, rm0)  # batch statistics ran
    assert bn_tracked(frozen)[:2] == (nbt0[0] + B, nbt0[1] + B)


def test_class_feature_off_moves_the_backbone_statistics_only():
    B = 3
    use = ("color", "position", "num")
    model, objects, texts, batches, target, _ = model_problem(B, use=use, L=1)
    rm0 = model.object_encoder.pointnet.ga.mlp[0][1].running_var.clone()
    w0 = {n: q.detach().clone() for n, q in backbone_params(model).items()}
    nbt0 = bn_tracked(model)
    mp0 = int(model.object_encoder.mlp_pointnet[0][1].num_batches_tracked)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, batches), target).backward()
    opt.step()
    assert bn_tracked(model)[:2] == (nbt0[0] + B, nbt0[1] + B)
    assert int(model.object_encoder.mlp_pointnet[0][1].num_batches_tracked) == mp0 + 1
    assert all(q.grad is None for q in backbone_params(model).values())
    assert all(torch.equal(q.detach(), w0[n]) for n, q in backbone_params(model).items())
    assert not torch.equal(model.object_encoder.pointnet.ga.mlp[0][1].running_var, rm0)


def test_color_feature_off_voids_the_colours_without_touching_the_batches():
    use = ("class", "position", "num")
    model, objects, texts, batches, target, _ = model_problem(3, use=use, L=1)
    keep = [{k: v.copy() for k, v in b.items()} for b in batches]
    torch.manual_seed(3)
    a = model(objects, texts, batches).detach()
    assert all(np.array_equal(b[k], c[k]) for b, c in zip(batches, keep) for k in b)  # the caller's arrays are unchanged
    black = [{"pos": b["pos"], "x": np.zeros_like(b["x"])} for b in keep]
    torch.manual_seed(3)
    b = model(objects, texts, black).detach()
    assert float((a - b).abs().max()) < 1e-5


def test_features2_tensors_leave_the_backbone_gradients_at_none():
    B = 3
    model, objects, texts, _, target, _ = model_problem(B)
    feats = [torch.from_numpy(np.abs(np.random.default_rng(i).standard_normal((16, 256))).astype(np.float32)).cuda() for i in range(B)]
    w0 = {n: q.detach().clone() for n, q in model.named_parameters() if n.startswith(P)}
    nbt0 = bn_tracked(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, feats), target).backward()
    opt.step()
    assert all(q.grad is None for n, q in model.named_parameters() if n.startswith(P))
    assert all(torch.equal(q.detach(), w0[n]) for n, q in model.named_parameters() if n.startswith(P))
    assert model.object_encoder.mlp_pointnet[0][0].weight.grad is not None
    assert bn_tracked(model)[:2] == nbt0[:2]  # the backbone did not run


def test_eval_after_a_points_step_sees_the_updated_backbone():
    B = 3
    model, objects, texts, batches, target, (cells, pos, rgb) = model_problem(B)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, batches), target).backward()
    opt.step()
    model.eval()
    got = model(objects, texts, batches).cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if not k.startswith("language_encoder.")}
    f2 = OP.pointnet_features(pos, rgb, np.arange(0, 16 * B + 1, 16, dtype=np.int32), sd)
    twin = Twin(sd, False, False, ALL, 2)
    hints = torch.from_numpy(model.language_encoder.table.detach().cpu().numpy().astype(np.float64))
    ref = twin.forward(cells, hints, torch.from_numpy(np.asarray(f2, dtype=np.float64)), train=False).detach().numpy()
    assert np.abs(got - ref).max() < 1e-4, np.abs(got - ref).max()


def test_train_epoch_on_point_batches_lowers_the_loss():
    from text2loc_amd.fine_training import train_epoch

    torch.manual_seed(0)
    B = 6
    model, objects, texts, batches, target, _ = model_problem(B, seed=4)

    class Pose:
        def __init__(self, xy):
            self.pose = np.array([xy[0], xy[1], 0.0])

    tgt = target.cpu().numpy()
    batch = {"objects": objects, "texts": texts, "offsets": tgt, "poses": [Pose(t) for t in tgt], "object_points": batches}
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    crit = torch.nn.MSELoss()
    nbt0 = bn_tracked(model)
    losses = [train_epoch(model, [batch], fine_args(False), opt, crit)["loss"] for _ in range(12)]
    assert losses[-1] < 0.5 * losses[0], losses
    assert bn_tracked(model)[0] == nbt0[0] + 12 * B
    assert model.object_encoder.pointnet.lin2.weight.grad is not None


def test_point_batch_refusals():
    model, objects, texts, batches, _, _ = model_problem(2, L=1)
    short = [{"pos": b["pos"][:15 * 256], "x": b["x"][:15 * 256]} for b in batches]
    with pytest.raises(T2LError, match="16\\*256 points"):
        model(objects, texts, short)
    mixed = [batches[0], torch.zeros(16, 256, device="cuda")]
    with pytest.raises(T2LError, match="mixes point batches and features2"):
        model(objects, texts, mixed)
