"""GPU tier: the PointNet++ object backbone under model.train() (SURVEY.md §8 rows a3 + a9) through the C ABI —
t2l_pointnet_features_train / t2l_pointnet_backward — against the float64 oracle oracle/t2l_oracle_pointnet_train.py
(per-cell BatchNorm statistics, sequential running-statistics updates, max aggregation with arg-max replay).
PARITY UNPINNED like the eval path (the index structure is this build's reading of torch_cluster / PyG): what is checked
here is self-consistency of the HIP kernels with the build's own restatement, whose backward is checked against central
differences in tests/test_oracle_train.py."""
import numpy as np
import pytest
import torch

from oracle import t2l_oracle_pointnet_train as OPT
from text2loc_amd import synth

pytestmark = pytest.mark.gpu

P = "object_encoder.pointnet."


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def bind_all(eng, sd_obj, sd_pn):
    tensors = {}
    for k, v in list(sd_obj.items()) + list(sd_pn.items()):
        if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight") or "classifier" in k:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tensors, class_embed=False, color_embed=False)
    return tensors


def check(tensors, name, exp, med=1e-2, fro=0.03):
    """-> True when the tensor agrees to float32 rounding (1e-4 of its norm). The per-kernel bounds live in the block tier
    (tests/test_gpu_pointnet_train_blocks.py: every kernel of the chain as one launch against float64, element by element); the
    chain bars below stay as they are."""
    got = tensors[name][1].cpu().numpy().astype(np.float64).ravel()
    exp = np.asarray(exp, dtype=np.float64).ravel()
    rms = max(np.sqrt((exp ** 2).mean()), 1e-30)
    err = np.abs(got - exp)
    if name.endswith(".0.bias") and "lin" not in name:  # Linear bias in front of a BatchNorm: true gradient 0
        scale = np.abs(tensors[name.replace(".0.bias", ".1.bias")][1].cpu().numpy()).max()
        assert np.abs(got).max() < 2e-3 * max(1.0, scale), (name, np.abs(got).max(), scale)
        return False
    # float32 MFMA kernels against float64. Measured: ~1e-6 of the norm on every tensor, EXCEPT upstream of a discrete decision
    # (arg-max row, ReLU sign, 32nd neighbour) that falls the other way within float32 rounding: one such flip in SA3 of the
    # ragged case moves everything upstream by ~1% of its norm. A wrong formula is O(1) everywhere.
    assert np.median(err) < med * rms + 1e-9, (name, np.median(err), rms)
    ratio = np.sqrt((err ** 2).sum()) / max(np.sqrt((exp ** 2).sum()), 1e-30)
    assert ratio < fro, (name, ratio)
    return ratio < 1e-4


@pytest.mark.parametrize("n_cells,min_obj,max_obj,self_loops", [(2, 2, 2, 1), (3, 1, 4, 1), (2, 3, 3, 0)])
def test_pointnet_train_forward_backward_match_the_float64_oracle(eng, n_cells, min_obj, max_obj, self_loops):
    cells = synth.make_cells(n_cells, seed=3 + n_cells, min_obj=min_obj, max_obj=max_obj)
    pos, rgb = synth.make_sampled_points(cells, 3)
    sd_pn = synth.make_pointnet_weights(1)
    sd_obj = synth.make_object_branch_weights(2)
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    n = pos.shape[0]
    eng.set_option("pointnet_pyg_self_loops", self_loops)
    tensors = bind_all(eng, sd_obj, sd_pn)
    rng = np.random.default_rng(0)
    R = rng.standard_normal((n, 256))
    f2_ref, info = OPT.forward_backward(pos, rgb, offs, sd_pn, grad_f2=R, pyg_self_loops=bool(self_loops))

    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    f2 = eng.pointnet_features_train(dpos, drgb, offs)
    torch.cuda.synchronize()
    got = f2.cpu().numpy().astype(np.float64)
    scale = np.abs(f2_ref).max()
    assert np.abs(got - f2_ref).max() < 2e-4 * scale, (np.abs(got - f2_ref).max(), scale)
    # running statistics: one momentum update per cell, in cell order
    for k, v in info["running"].items():
        r = tensors[k][0].cpu().numpy().astype(np.float64)
        assert np.abs(r - v).max() < 2e-5 * max(1.0, np.abs(v).max()), (k, np.abs(r - v).max())
        assert np.abs(v - np.asarray(sd_pn[k], dtype=np.float64)).max() > 0  # they did move
    eng.zero_grad()
    eng.pointnet_backward(torch.from_numpy(R.astype(np.float32)).cuda())
    torch.cuda.synchronize()
    assert sorted(info["grads"].keys()) == sorted(k for k in tensors if k.startswith(P) and tensors[k][1] is not None)
    tight = sum(check(tensors, name, g) for name, g in info["grads"].items())
    assert tight >= 10, tight  # (28 tensors are not Linear biases in front of a BatchNorm; a flip leaves its downstream side tight)
    eng.set_option("pointnet_pyg_self_loops", 1)


def test_pointnet_train_backward_accumulates_and_repeats(eng):
    """Two backward calls double the gradients (they ADD, as autograd does); a second forward gives identical features."""
    cells = synth.make_cells(2, seed=9, min_obj=2, max_obj=3)
    pos, rgb = synth.make_sampled_points(cells, 1)
    tensors = bind_all(eng, synth.make_object_branch_weights(2), synth.make_pointnet_weights(4))
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    g = torch.randn(pos.shape[0], 256, device="cuda")
    a = eng.pointnet_features_train(dpos, drgb, offs).clone()
    eng.zero_grad()
    eng.pointnet_backward(g)
    one = {k: v[1].clone() for k, v in tensors.items() if k.startswith(P) and v[1] is not None}
    eng.pointnet_backward(g)
    for k, v in one.items():
        two = tensors[k][1]
        if k.endswith(".0.bias") and "lin" not in k:  # in front of a BatchNorm: atomics-ordered float32 noise around 0
            continue
        assert torch.allclose(two, 2 * v, rtol=1e-3, atol=1e-5 * float(v.abs().max()) + 1e-9), k
    b = eng.pointnet_features_train(dpos, drgb, offs)
    assert torch.equal(a, b)  # batch statistics do not depend on the running statistics; every kernel is deterministic in forward


def test_pointnet_train_needs_the_backbone_bound(eng):
    from text2loc_amd.engine import T2LError

    sd = synth.make_object_branch_weights(2)
    tensors = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight"):
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tensors, class_embed=False, color_embed=False)
    pos = torch.zeros(1, 256, 3, device="cuda")
    with pytest.raises(T2LError, match="bind the object_encoder.pointnet"):
        eng.pointnet_features_train(pos, pos, np.array([0, 1], dtype=np.int32))
    # a partial binding is refused
    pn = synth.make_pointnet_weights(1)
    k = P + "lin2.weight"
    t = torch.from_numpy(pn[k]).cuda()
    tensors[k] = (t, torch.zeros_like(t))
    with pytest.raises(T2LError, match="completely"):
        eng.train_bind(tensors, class_embed=False, color_embed=False)


def _model(freeze=False):
    from tests.test_gpu_train_loop import TableText, _args
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    args = _args(class_embed=False, color_embed=False, pointnet_freeze=freeze)
    model = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=TableText(8, 1))
    sd = dict(synth.make_object_branch_weights(6))
    sd.update(synth.make_pointnet_weights(2))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    for layer in model.obj_inter_module:  # the oracle chain below runs without dropout
        layer.dropout.p = layer.dropout1.p = layer.dropout2.p = 0.0
        layer.self_attn.dropout = 0.0
    return model.to("cuda"), sd


def test_model_train_step_reaches_the_backbone():
    """CellRetrievalNetwork.train(): encode_objects(objects, point batches) -> loss.backward() -> optim.Adam.step() with the
    backbone trained jointly (the published configuration), against the float64 oracle chain
    PointNet++(train) -> encode_cells_train -> backward -> PointNet++ backward; then --pointnet_freeze."""
    from oracle import t2l_oracle_train as OT
    from tests.test_host_logic import make_objects
    from text2loc_amd import packing
    from text2loc_amd.optim import Adam

    B = 3
    cells = synth.make_cells(B, seed=21, min_obj=2, max_obj=3)
    objects = make_objects(cells, 21)
    pos, rgb = synth.make_sampled_points(cells, 5)
    offs = cells["offsets"]
    batches = [{"pos": torch.from_numpy(pos[offs[i]:offs[i + 1]].reshape(-1, 3)), "x": torch.from_numpy(rgb[offs[i]:offs[i + 1]].reshape(-1, 3))}
               for i in range(B)]
    model, sd = _model()
    opt = Adam(model, lr=1e-3)
    model.train()
    nbt0 = int(model.object_encoder.pointnet.sa1.point_conv.local_nn[0][1].num_batches_tracked)
    R = torch.randn(B, 256, generator=torch.Generator().manual_seed(0)).cuda()
    opt.zero_grad()
    out = model.encode_objects(objects, batches)
    (out * R).sum().backward()
    # oracle chain on the same inputs
    packed = packing.pack_cells(objects, model.object_encoder.known_classes, model.object_encoder.known_colors)
    f2, _ = OPT.forward_backward(pos, rgb, offs, sd)
    c2 = dict(packed)
    c2["pn_feat"] = f2
    sd64 = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    out_ref, info = OT.encode_cells_train(c2, sd64, False, False, grad_out=R.cpu().numpy().astype(np.float64))
    assert np.abs(out.detach().cpu().numpy() - out_ref).max() < 5e-5
    _, pinfo = OPT.forward_backward(pos, rgb, offs, sd, grad_f2=info["grad_pn_feat"])
    params = dict(model.named_parameters())
    tight = 0
    for name, g in pinfo["grads"].items():
        got = params[name].grad
        assert got is not None, name
        if name.endswith(".0.bias") and "lin" not in name:
            continue
        err = np.abs(got.cpu().numpy().astype(np.float64) - g)
        ratio = np.sqrt((err ** 2).sum()) / max(np.sqrt((g ** 2).sum()), 1e-30)
        assert ratio < 0.03, (name, ratio)
        tight += ratio < 1e-3
    assert tight >= 10
    assert params[P + "class_classifier.weight"].grad is None  # not on the path, as in the reference
    before = {n: p.detach().clone() for n, p in params.items() if n.startswith(P)}
    opt.step()
    moved = [n for n in before if not torch.equal(before[n], params[n].detach())]
    assert P + "sa1.point_conv.local_nn.0.0.weight" in moved and P + "lin2.weight" in moved
    assert P + "class_classifier.weight" not in moved
    bn = model.object_encoder.pointnet.sa1.point_conv.local_nn[0][1]
    assert int(bn.num_batches_tracked) - nbt0 == B  # one backbone call per cell in the reference
    # eval after the step: the fused eval path sees the updated backbone (running statistics, not batch statistics)
    model.eval()
    with torch.no_grad():
        ev = model.encode_objects(objects, batches)
    assert torch.isfinite(ev).all() and float((ev - out.detach()).abs().max()) > 1e-4

    # --pointnet_freeze: weights frozen, BatchNorm still in training mode (object_encoder.py:53-55 + model.train())
    frozen, _ = _model(freeze=True)
    frozen.train()
    opt2 = Adam(frozen, lr=1e-3)
    opt2.zero_grad()
    rm0 = frozen.object_encoder.pointnet.sa2.point_conv.local_nn[1][1].running_mean.clone()
    out2 = frozen.encode_objects(objects, batches)
    assert float((out2 - out).detach().abs().max()) < 1e-6  # same forward as the trainable model's first step
    (out2 * R).sum().backward()
    opt2.step()
    fp = dict(frozen.named_parameters())
    assert all(fp[n].grad is None for n in fp if n.startswith(P))
    assert all(torch.equal(fp[n].detach().cpu(), torch.from_numpy(np.asarray(sd[n]))) for n in fp if n.startswith(P))
    assert not torch.equal(rm0, frozen.object_encoder.pointnet.sa2.point_conv.local_nn[1][1].running_mean)
    assert fp["object_encoder.mlp_pointnet.0.0.weight"].grad.abs().max() > 0


class _DictText(torch.nn.Module):
    """Trainable stand-in for the text branch (T5 weights are not in the image): one embedding row per distinct description."""

    def __init__(self, n, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.table = torch.nn.Parameter(torch.randn(n, 256, generator=g))
        self.rows = {}

    def forward(self, texts):
        idx = [self.rows.setdefault(t, len(self.rows)) for t in texts]
        return self.table[torch.as_tensor(idx, device=self.table.device)]

    @property
    def device(self):
        return self.table.device


def test_train_and_eval_epochs_on_a_kitti360pose_directory():
    """The reference's training script, end to end, on a KITTI360Pose directory (the tiny fixture written by the reference's own
    classes): Kitti360PoseDataset(object_points="sample") -> DataLoader(collate_fn) -> train_epoch (published feature mode:
    PointNet++ trained jointly, no --pointnet_freeze) -> eval_epoch. Loss falls, the backbone's weights move, retrieval runs."""
    import os.path as osp

    from tests.test_gpu_train_loop import _args
    from text2loc_amd import kitti360pose as K
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork
    from text2loc_amd.coarse import eval_epoch, train_epoch
    from text2loc_amd.losses import ContrastiveLoss
    from text2loc_amd.optim import Adam

    base = osp.join(osp.dirname(osp.abspath(__file__)), "golden", "k360_tiny")
    g = np.load(osp.join(osp.dirname(base), "k360_tiny.npz"), allow_pickle=False)
    scenes = [str(s) for s in g["scenes"]]
    ds = K.Kitti360PoseDataset(base, scenes, object_points="sample", seed=3)
    args = _args(class_embed=False, color_embed=False, pointnet_freeze=False, batch_size=4, top_k=[1, 3], ranking_loss="contrastive")
    model = CellRetrievalNetwork(ds.get_known_classes(), synth.COLOR_NAMES, args, language_encoder=_DictText(len(ds))).to("cuda")
    dl = torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=K.Kitti360PoseDataset.collate_fn, shuffle=False, drop_last=True)
    opt = Adam(model, lr=1e-3)
    w0 = model.object_encoder.pointnet.sa2.point_conv.local_nn[0][0].weight.detach().clone()
    torch.manual_seed(0)
    losses = [train_epoch(model, dl, args, opt, ContrastiveLoss(0.1))[0] for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
    w1 = model.object_encoder.pointnet.sa2.point_conv.local_nn[0][0].weight.detach()
    assert float((w1 - w0).abs().max()) > 1e-4  # the backbone trained
    dl_val = torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=K.Kitti360PoseDataset.collate_fn, shuffle=False)
    acc, acc_close, retrievals = eval_epoch(model, dl_val, args)
    assert set(acc) == {1, 3} and all(0.0 <= v <= 1.0 for v in acc.values()) and len(retrievals) == len(ds)


def test_batch_of_64_cells_equals_its_parts(eng):
    """The published batch (64 cells, ~1,300 objects, 2.7 M edge rows at SA1: beyond one GEMM launch's 65,535 row tiles): every
    cell's BatchNorm is its own, so features of a cell and the parameter gradients summed over parts of the batch must equal
    those of the whole batch (to float32 summation order)."""
    cells = synth.make_cells(64, seed=1)
    pos, rgb = synth.make_sampled_points(cells, 1)
    tensors = bind_all(eng, synth.make_object_branch_weights(2), synth.make_pointnet_weights(3))
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    g = torch.randn(pos.shape[0], 256, generator=torch.Generator().manual_seed(1)).cuda()
    names = [k for k in tensors if k.startswith(P) and tensors[k][1] is not None]
    run0 = {k: tensors[k][0].clone() for k in tensors if "running_" in k}

    full = eng.pointnet_features_train(dpos, drgb, offs).clone()
    eng.zero_grad()
    eng.pointnet_backward(g)
    torch.cuda.synchronize()
    g_full = {k: tensors[k][1].clone() for k in names}
    run_full = {k: tensors[k][0].clone() for k in run0}

    for k, v in run0.items():  # the same starting running statistics for the run in parts
        tensors[k][0].copy_(v)
    eng.zero_grad()
    parts = []
    for c0 in range(0, 64, 16):
        lo, hi = int(offs[c0]), int(offs[c0 + 16])
        sub = (offs[c0:c0 + 17] - offs[c0]).astype(np.int32)
        parts.append(eng.pointnet_features_train(dpos[lo:hi].contiguous(), drgb[lo:hi].contiguous(), sub).clone())
        eng.pointnet_backward(g[lo:hi].contiguous())
    torch.cuda.synchronize()
    got = torch.cat(parts)
    assert float((got - full).abs().max()) < 2e-5 * max(1.0, float(full.abs().max()))
    for k in names:
        a, b = tensors[k][1], g_full[k]
        if k.endswith(".0.bias") and "lin" not in k:
            continue  # in front of a BatchNorm: float32 noise around a zero gradient
        err = float((a - b).norm() / (b.norm() + 1e-30))
        # the BatchNorm sums meet in a different order (float64 atomics of float32 partials): among 2.7 M edge rows a few
        # arg-max / ReLU decisions fall the other way and move single gradients by a few 1e-3; a mis-sliced GEMM would lose
        # a quarter of the rows
        assert err < 1e-2, (k, err)
    for k in run0:  # sequential per-cell momentum updates: the same sequence either way
        assert float((tensors[k][0] - run_full[k]).abs().max()) < 1e-5 * max(1.0, float(run_full[k].abs().max())), k


def test_bf16_rows_bind_the_backward_to_the_forwards_arithmetic(eng):
    """With bf16 operands (``train_bf16 = 1``) the forward leaves its edge rows in memory as bf16; a backward under another setting would
    read them as float32. The library refuses (T2L_ESTATE) instead of differentiating garbage; the matching pair runs."""
    from text2loc_amd.engine import T2LError

    cells = synth.make_cells(3, seed=4, min_obj=2, max_obj=5)
    pos, rgb = synth.make_sampled_points(cells, 2)
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    g = torch.randn(pos.shape[0], 256, generator=torch.Generator().manual_seed(1)).cuda()
    try:
        for fwd, bwd in ((1, 0), (0, 1), (2, 1)):
            bind_all(eng, synth.make_object_branch_weights(2), synth.make_pointnet_weights(3))
            eng.set_option("train_bf16", fwd)
            eng.pointnet_features_train(dpos, drgb, offs)
            eng.set_option("train_bf16", bwd)
            with pytest.raises(T2LError, match="train_bf16 changed"):
                eng.pointnet_backward(g)
            eng.set_option("train_bf16", fwd)
            eng.pointnet_backward(g)  # the forward's own arithmetic: fine
        torch.cuda.synchronize()
    finally:
        eng.set_option("train_bf16", 0)


@pytest.mark.parametrize("mode,tol", [(2, 2e-3), (1, 6e-2)])
def test_reduced_precision_gemms_track_the_f32_run_on_a_ragged_batch(eng, mode, tol):
    """The training GEMMs (weights resident in LDS, BatchNorm sums in the epilogue, the first layer's BatchNorm + ReLU applied by
    whoever loads it) with split-bf16 / bf16 operands against the SAME kernels in float32 (which the float64 oracle pins above) on a
    ragged 12-cell batch — every tile shape of tn2_kernel and every pass count of rows2_kernel occurs: features, running statistics
    and parameter gradients (tolerances = the arithmetic's; bf16 rounds operands, so a few discrete decisions fall the other way).
    (Until round 5 this compared against the first version's kernels, option pointnet_train_v1 — removed: 26 vs 17 ms per step.)"""
    cells = synth.make_cells(12, seed=21, min_obj=1, max_obj=9)
    pos, rgb = synth.make_sampled_points(cells, 5)
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    dpos, drgb = torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()
    g = torch.randn(pos.shape[0], 256, generator=torch.Generator().manual_seed(2)).cuda()
    res = {}
    try:
        for m in (0, mode):
            eng.set_option("train_bf16", m)
            tensors = bind_all(eng, synth.make_object_branch_weights(2), synth.make_pointnet_weights(3))
            f2 = eng.pointnet_features_train(dpos, drgb, offs).clone()
            eng.zero_grad()
            eng.pointnet_backward(g)
            torch.cuda.synchronize()
            res[m] = (f2, {k: t[1].clone() for k, t in tensors.items() if k.startswith(P) and t[1] is not None},
                      {k: t[0].clone() for k, t in tensors.items() if "running_" in k and k.startswith(P)})
    finally:
        eng.set_option("train_bf16", 0)
    (fa, ga, ra), (fb, gb, rb) = res[0], res[mode]
    assert float((fa - fb).abs().max()) < tol * max(1.0, float(fa.abs().max()))
    for k in ra:
        assert float((ra[k] - rb[k]).abs().max()) < tol * max(1.0, float(ra[k].abs().max())), k
    worst = 0.0
    for k in ga:
        if k.endswith(".0.bias") and "lin" not in k:
            continue  # in front of a BatchNorm: noise around a zero gradient
        err = float((ga[k] - gb[k]).norm() / (ga[k].norm() + 1e-30))
        worst = max(worst, err)
        # four levels of 8-bit products below the first layer's weights leave up to 0.4 of its gradient's norm in bf16 against the f32
        # run (measured 0.41 on sa1's first layer; a wrong kernel is O(1) AND loses the direction): split-bf16 is held to 5 %, bf16 to
        # the direction (cosine) — the float32 run is pinned by the oracle, these rows pin the operand conversions
        if mode == 2:
            assert err < 0.05, (k, err)
        else:
            # (round 6: with bf16 operands the edge-row tensors are STORED as bf16 too — what torch.autocast keeps between its Linear and
            # BatchNorm modules. Rounded to 8 bits many rows of a group tie for a channel's maximum and the first one wins: the gradient of
            # such a channel takes another edge than in the f32 run. Measured on sa1's first BatchNorm weight, four levels below the loss:
            # 0.41 -> 0.555 of the norm, cosine 0.87 -> 0.844; every other tensor stays above 0.9.)
            cos = float((ga[k] * gb[k]).sum() / (ga[k].norm() * gb[k].norm() + 1e-30))
            assert err < 0.65 and cos > 0.8, (k, err, cos)
    assert worst > 0.0  # different operand arithmetic, not the same run twice
