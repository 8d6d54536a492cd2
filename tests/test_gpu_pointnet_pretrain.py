"""GPU tier of the backbone's pretraining step: t2l_pointnet_cls_bind / _forward / _heads / _backward through the C ABI against the
float64 references of tests/pointnet_cls_ref.py (heads, loss: derived bounds) and oracle/t2l_oracle_pointnet_train.py (backbone: the
bars of tests/test_gpu_pointnet_train.py), then ``text2loc_amd.pointnet_pretrain`` on top: the short trajectory, the checkpoint
round trip into CellRetrievalNetwork and CrossMatch, the batch loop, the error paths. PARITY UNPINNED like the rest of PointNet++:
self-consistency with the build's own restatement."""
import argparse
import os.path as osp

import numpy as np
import pytest
import torch

from tests import pointnet_cls_ref as R
from text2loc_amd import synth

pytestmark = pytest.mark.gpu

P = R.P
TINY = osp.join(osp.dirname(osp.abspath(__file__)), "golden", "k360_tiny")
SCENES = ["2013_05_28_drive_0003_sync", "2013_05_28_drive_0010_sync"]


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def bind(eng, sd, frozen=False, drop=(), head_grads=True):
    """name -> (live tensor, gradient buffer | None) of every tensor of ``sd`` but ``drop``, bound by t2l_pointnet_cls_bind."""
    tensors = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or k in drop:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        head = "classifier" in k
        grad = None if "running_" in k or (head and not head_grads) or (frozen and not head) else torch.zeros_like(t)
        tensors[k] = (t, grad)
    eng.pointnet_cls_bind(tensors)
    return tensors


def grad_of(tensors, name):
    return tensors[name][1].cpu().numpy().astype(np.float64)


def assert_heads(got, ref, b, tensors=None, what=""):
    """(logits, loss, correct, dx) of a heads call and, with ``tensors``, the four head gradients (buffers zero before the call)
    against the float64 reference, every element inside its derived bound (each figure is printed before it is asserted)."""
    logits, loss, correct, dx = got
    figures = [("logits", logits, ref["logits"], b["logits"]), ("loss", loss, ref["loss"], b["loss"])]
    if dx is not None:
        figures.append(("dx", dx, ref["dx"], b["dx"]))
    if tensors is not None:
        figures += [(k, tensors[k][1], ref["grads"][k], b["grads"][k]) for k in ref["grads"]]
    worst = {}
    for name, g, r, tol in figures:
        err = np.abs(g.cpu().numpy().astype(np.float64) - r)
        worst[name] = float((err / np.maximum(tol, 1e-300)).max())  # (a zero bound — a zero loss weight — admits a zero error only)
    print(what, "worst err / bound:", {k: f"{v:.3f}" for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (what, name, v)
    assert correct.cpu().numpy().tolist() == ref["correct"].tolist(), what


# ---- 1. the heads alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", R.HEAD_CLASSES)
@pytest.mark.parametrize("n", R.HEAD_ROWS)
def test_heads_match_float64_within_the_derived_bounds(eng, n, classes):
    x, sd, lc, lk, ref, b = R.heads_case(n, classes)
    tensors = bind(eng, sd)
    dx = torch.from_numpy(x).cuda()
    got = eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR)
    torch.cuda.synchronize()
    assert got[0].shape == (n, sum(classes))
    assert_heads(got, ref, b, tensors, f"n={n} classes={classes}")
    # a second backward call doubles the head gradients (they ADD, as autograd does)
    one = {k: tensors[k][1].clone() for k in ref["grads"]}
    again = eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR)
    for k, v in one.items():
        assert torch.allclose(tensors[k][1], 2 * v, rtol=1e-3, atol=1e-5 * float(v.abs().max()) + 1e-9), k
    # everything but the atomically summed head gradients has a fixed order: the same bits
    for a, c in zip(got, again):
        assert torch.equal(a, c)
    # the forward-only form: the same logits, loss and counts, and no gradient buffer touched
    pattern = {k: v[1].clone() for k, v in tensors.items() if v[1] is not None}
    fwd = eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR, need_grad=False)
    torch.cuda.synchronize()
    assert fwd[3] is None and all(torch.equal(fwd[i], got[i]) for i in range(3))
    assert all(torch.equal(tensors[k][1], v) for k, v in pattern.items())
    # the backbone's buffers were never touched at all
    assert all(not v[1].any() for k, v in tensors.items() if v[1] is not None and "classifier" not in k)


def test_heads_loss_weights_scale_the_gradients_only(eng):
    x, sd, lc, lk, _, _ = R.heads_case(5, (22, 8))
    tensors = bind(eng, sd)
    ref = R.heads_ref(x, sd, lc, lk, 0.0, 2.0)
    b = R.heads_bounds(x, ref, 0.0, 2.0)
    got = eng.pointnet_cls_heads(torch.from_numpy(x).cuda(), lc, lk, 0.0, 2.0)
    assert_heads(got, ref, b, tensors, "w = (0, 2)")
    assert not tensors[P + "class_classifier.weight"][1].any() and tensors[P + "color_classifier.weight"][1].any()


# ---- 2. the whole step -------------------------------------------------------------------------------------------------------------
def check(tensors, name, exp, med=1e-2, fro=0.03):
    """tests/test_gpu_pointnet_train.py's ``check``, restated: -> True when the tensor agrees to float32 rounding (1e-4 of its norm)."""
    got = grad_of(tensors, name).ravel()
    exp = np.asarray(exp, dtype=np.float64).ravel()
    rms = max(np.sqrt((exp ** 2).mean()), 1e-30)
    err = np.abs(got - exp)
    if name.endswith(".0.bias") and "lin" not in name:  # Linear bias in front of a BatchNorm: true gradient 0
        scale = np.abs(tensors[name.replace(".0.bias", ".1.bias")][1].cpu().numpy()).max()
        assert np.abs(got).max() < 2e-3 * max(1.0, scale), (name, np.abs(got).max(), scale)
        return False
    assert np.median(err) < med * rms + 1e-9, (name, np.median(err), rms)
    ratio = np.sqrt((err ** 2).sum()) / max(np.sqrt((exp ** 2).sum()), 1e-30)
    assert ratio < fro, (name, ratio)
    return ratio < 1e-4


def step_inputs(n_obj, seed):
    cells = synth.make_cells(1, seed=seed, min_obj=n_obj, max_obj=n_obj)
    pos, rgb = synth.make_sampled_points(cells, seed + 1)
    rng = np.random.default_rng([seed, 0x57E9])
    return pos, rgb, synth.make_pointnet_weights(seed + 2), rng.integers(0, 22, n_obj).astype(np.int32), rng.integers(0, 8, n_obj).astype(np.int32)


@pytest.mark.parametrize("n_obj", [6, 1])
def test_whole_step_matches_the_float64_oracle(eng, n_obj):
    pos, rgb, sd, lc, lk = step_inputs(n_obj, 30 + n_obj)
    f2_ref, ref64, info = R.step_ref(pos, rgb, sd, lc, lk, R.W_CLASS, R.W_COLOR)
    tensors = bind(eng, sd)
    f2 = eng.pointnet_cls_forward(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda())
    torch.cuda.synchronize()
    got = f2.cpu().numpy().astype(np.float64)
    scale = np.abs(f2_ref).max()
    print("features2 err / scale", np.abs(got - f2_ref).max() / scale)
    assert np.abs(got - f2_ref).max() < 2e-4 * scale
    for k, v in info["running"].items():  # ONE segment: one momentum update of every BatchNorm
        r = tensors[k][0].cpu().numpy().astype(np.float64)
        assert np.abs(r - v).max() < 2e-5 * max(1.0, np.abs(v).max()), (k, np.abs(r - v).max())
        assert np.abs(v - np.asarray(sd[k], dtype=np.float64)).max() > 0
    # the heads against float64 heads fed the KERNEL's features2: the tight bounds of the heads tests
    ref = R.heads_ref(f2.cpu().numpy(), sd, lc, lk)
    heads = eng.pointnet_cls_heads(f2, lc, lk, R.W_CLASS, R.W_COLOR)
    assert_heads(heads, ref, R.heads_bounds(f2.cpu().numpy(), ref), tensors, f"whole step, {n_obj} objects")
    # the backbone's gradients against the oracle fed the float64 heads' d features2
    eng.pointnet_cls_backward(heads[3])
    torch.cuda.synchronize()
    assert sorted(info["grads"].keys()) == sorted(k for k in tensors if tensors[k][1] is not None and "classifier" not in k)
    tight = sum(check(tensors, name, g) for name, g in info["grads"].items())
    print("tight tensors", tight)
    assert tight >= 10, tight


def test_frozen_backbone_trains_the_heads_only(eng):
    from text2loc_amd.engine import T2LError

    pos, rgb, sd, lc, lk = step_inputs(3, 50)
    tensors = bind(eng, sd, frozen=True)
    before = {k: v[0].clone() for k, v in tensors.items()}
    f2 = eng.pointnet_cls_forward(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda())
    heads = eng.pointnet_cls_heads(f2, lc, lk)
    with pytest.raises(T2LError, match="frozen"):
        eng.pointnet_cls_backward(heads[3])
    torch.cuda.synchronize()
    assert all(tensors[P + h + s][1].any() for h in R.HEADS for s in (".weight", ".bias"))  # the heads train
    for k, v in tensors.items():
        if "running_" in k:
            assert not torch.equal(v[0], before[k]), k  # the statistics still move
        else:
            assert torch.equal(v[0], before[k]), k  # every tensor bit-equal (there are no moments in the engine for this step)
    # the same forward as a trainable binding's
    bind(eng, sd)
    assert torch.equal(f2, eng.pointnet_cls_forward(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda()))


# ---- 3. the trajectory -------------------------------------------------------------------------------------------------------------
def model_from(sd, c1=22, c2=8):
    from text2loc_amd.pointnet_pretrain import PointNet2

    model = PointNet2(c1, c2)
    model.load_state_dict({k[len(P):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    return model.to("cuda")


def test_trajectory_first_loss_and_strict_decrease():
    """The CPU tier's case (4 objects, one segment, Adam lr 1e-3) through train_epoch with torch.optim.Adam. The first loss against
    float64: features2 agrees to the backbone's bar e = 2e-4 max|f2| (tests/test_gpu_pointnet_train.py), a logit therefore to
    g = max_c sum_k |W_ck| e beside its own bound, and CE is 2-Lipschitz in the largest logit error of its row
    (tests/pointnet_cls_ref.py): 2 g per head + the heads' own loss bounds. The counts are float64's because every top-two gap
    exceeds 2 (g + d) (asserted). Later losses are only required to fall (a ReLU or arg-max flip legitimately moves them)."""
    from text2loc_amd.pointnet_pretrain import ClassifierLoss, train_epoch

    pos, rgb, sd, lc, lk = R.make_trajectory_inputs()
    f2_ref, ref, _ = R.step_ref(pos, rgb, sd, lc, lk, 1.0, 1.0, backward=False)
    b = R.heads_bounds(f2_ref, ref, 1.0, 1.0)
    e = 2e-4 * np.abs(f2_ref).max()
    g = [np.abs(h["W"]).sum(axis=1).max() * e for h in ref["heads"]]
    tol = 2 * sum(g) + b["loss"].sum()
    assert all((b["gap"][:, i] > 2 * (g[i] + b["d"])).all() for i in range(2))
    model = model_from(sd)
    opt = torch.optim.Adam(model.parameters(), lr=R.TRAJ_LR)
    crit = ClassifierLoss()
    batch = [(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), lc, lk)]
    nbt0 = int(model.sa1.point_conv.local_nn[0][1].num_batches_tracked)
    stats = [train_epoch(model, batch, opt, crit) for _ in range(R.TRAJ_STEPS + 1)]
    losses = [s["loss"] for s in stats]
    print("losses", losses, "float64 first", ref["loss"].sum(), "bound", tol)
    assert abs(losses[0] - ref["loss"].sum()) <= tol
    assert all(y < x for x, y in zip(losses, losses[1:])), losses
    assert abs(stats[0]["loss_class"] + stats[0]["loss_color"] - losses[0]) < 1e-5 * max(1.0, losses[0])
    assert stats[0]["acc_class"] == ref["correct"][0] / len(lc) and stats[0]["acc_color"] == ref["correct"][1] / len(lc)
    assert int(model.sa1.point_conv.local_nn[0][1].num_batches_tracked) - nbt0 == R.TRAJ_STEPS + 1
    assert all(p.grad is not None for p in model.parameters())


def test_one_forward_per_backward():
    from text2loc_amd.engine import T2LError
    from text2loc_amd.pointnet_pretrain import ClassifierLoss

    pos, rgb, sd, lc, lk = R.make_trajectory_inputs()
    model = model_from(sd).train()
    batch = {"pos": torch.from_numpy(pos).cuda(), "x": torch.from_numpy(rgb).cuda()}
    crit = ClassifierLoss()
    first = crit(model(batch), lc, lk)
    second = crit(model(batch), lc, lk)
    with pytest.raises(T2LError, match="stale PointNet2 training forward.*LAST training-mode forward only"):
        first.backward()
    second.backward()
    assert model.lin2.weight.grad is not None and model.lin2.weight.grad.abs().max() > 0


# ---- 4. round trip and surface -----------------------------------------------------------------------------------------------------
class _Text(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.table = torch.nn.Parameter(torch.zeros(1, 256))

    @property
    def device(self):
        return self.table.device


def test_checkpoint_round_trip_into_both_models(tmp_path):
    """torch.save(model.state_dict()) is a pointnet_path file: loaded into CellRetrievalNetwork and CrossMatch as the reference loads
    it (object_encoder.py:50), the three eval-mode features2 of the same 16 objects (one cell) are bit-equal."""
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork
    from text2loc_amd.cross_matcher import CrossMatch

    cells = synth.make_cells(1, seed=70, min_obj=16, max_obj=16)
    pos, rgb = synth.make_sampled_points(cells, 71)
    model = model_from(synth.make_pointnet_weights(72)).eval()
    path = str(tmp_path / "pointnet.pth")
    torch.save(model.state_dict(), path)
    batch = {"pos": torch.from_numpy(pos.reshape(-1, 3)), "x": torch.from_numpy(rgb.reshape(-1, 3))}
    with torch.no_grad():
        mine = model(batch).features2
    a = argparse.Namespace(coarse_embed_dim=256, object_size=28, object_inter_module_num_heads=4, object_inter_module_num_layers=2,
                           hungging_model=None, fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4,
                           inter_module_num_layers=1, inter_module_num_heads=4, class_embed=False, color_embed=False,
                           use_features=["class", "color", "position", "num"])
    net = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, a, language_encoder=_Text())
    net.object_encoder.pointnet.load_state_dict(torch.load(path))
    net = net.to("cuda").eval()
    with torch.no_grad():
        coarse = net._pn_features([batch], net.engine())
    f = argparse.Namespace(fine_embed_dim=128, fine_num_decoder_heads=4, fine_num_decoder_layers=2, pad_size=16,
                           fine_intra_module_num_layers=1, fine_intra_module_num_heads=4, hungging_model=None, fixed_embedding=True,
                           class_embed=False, color_embed=False, use_features=["class", "color", "position", "num"])
    cm = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, f, language_encoder=torch.nn.Identity())
    cm.object_encoder.pointnet.load_state_dict(torch.load(path))
    cm = cm.to("cuda").eval()
    fine = cm.engine().pointnet_features(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), np.array([0, 16], dtype=np.int32))
    assert mine.shape == (16, 256) and mine.abs().max() > 0
    assert torch.equal(mine, coarse) and torch.equal(mine, fine)


def test_eval_epoch_counts_are_those_of_the_returned_logits():
    from text2loc_amd.pointnet_pretrain import ClassifierLoss, Kitti360ObjectDataset, eval_epoch, object_batches

    ds = Kitti360ObjectDataset(TINY, SCENES)
    model = model_from(synth.make_pointnet_weights(80)).eval()
    crit = ClassifierLoss()
    batches = list(object_batches(ds, 5, seed=3, transform="normalize", shuffle=False))
    assert [len(b[2]) for b in batches] == [5, 5, 4]
    stats = eval_epoch(model, batches, crit)
    ok = np.zeros(2)
    with torch.no_grad():
        for pos, rgb, lc, lk in batches:
            out = model({"pos": pos, "x": rgb})
            assert out.class_pred.shape == (len(lc), 22) and out.color_pred.shape == (len(lc), 8)
            ok += [(out.class_pred.argmax(1).cpu().numpy() == lc).sum(), (out.color_pred.argmax(1).cpu().numpy() == lk).sum()]
    assert stats["acc_class"] == ok[0] / len(ds) and stats["acc_color"] == ok[1] / len(ds)
    assert np.isfinite([stats["loss"], stats["loss_class"], stats["loss_color"]]).all()
    assert abs(stats["loss"] - stats["loss_class"] - stats["loss_color"]) < 1e-5 * max(1.0, stats["loss"])


def test_object_batches_rows_are_the_whole_set_samplers(eng):
    """Row r of a batch = object ``order[r]`` under ``seed ^ draw_salts(epoch, order[r], 1)[0]``: bit for bit that row of a whole-set
    t2l_sample_object_points call with that seed. The colour labels of the device reduction are the host restatement's."""
    from text2loc_amd.kitti360pose import draw_salts
    from text2loc_amd.pointnet_pretrain import Kitti360ObjectDataset, epoch_permutation, object_batches

    ds = Kitti360ObjectDataset(TINY, SCENES)
    seed, epoch = 11, 2
    order = epoch_permutation(len(ds), seed, epoch)
    d = ds.cell_set.on_device("cuda")
    seen = 0
    for pos, rgb, lc, lk in object_batches(ds, 4, seed=seed, epoch=epoch, engine=eng):
        chunk = order[seen:seen + len(lc)]
        assert pos.shape == (len(chunk), 256, 3) and pos.is_cuda and isinstance(lc, np.ndarray) and isinstance(lk, np.ndarray)
        assert lc.tolist() == ds.class_labels[chunk].tolist() and lk.tolist() == ds.color_labels_host()[chunk].tolist()
        for r in (0, len(chunk) - 1):
            item = int(chunk[r])
            whole = eng.sample_object_points(d["xyz"], d["rgb"], d["point_offsets"], seed=seed ^ int(draw_salts(epoch, item, 1)[0]),
                                             transform="rotate_normalize")
            assert torch.equal(pos[r], whole[0][item]) and torch.equal(rgb[r], whole[1][item])
        seen += len(chunk)
    assert seen == len(ds)


def test_out_of_range_label_names_its_row_and_writes_nothing(eng):
    from text2loc_amd.engine import T2LError

    x, sd, lc, lk, _, _ = R.heads_case(5, (22, 8))
    tensors = bind(eng, sd)
    dx = torch.from_numpy(x).cuda()
    outs = {"logits": torch.full((5, 30), 7.0, device="cuda"), "loss": torch.full((2,), 7.0, device="cuda"),
            "correct": torch.full((2,), 7, dtype=torch.int32, device="cuda"), "grad": torch.full((5, 256), 7.0, device="cuda")}
    for head, bad, C in (("class_labels", 22, 22), ("color_labels", -1, 8)):
        l1, l2 = lc.copy(), lk.copy()
        (l1 if head == "class_labels" else l2)[3] = bad
        rc = eng.lib.t2l_pointnet_cls_heads(eng._h, dx.data_ptr(), 5, l1.ctypes.data, l2.ctypes.data, 1.0, 1.0, outs["logits"].data_ptr(),
                                            outs["loss"].data_ptr(), outs["correct"].data_ptr(), outs["grad"].data_ptr(), None)
        assert rc == -1
        msg = eng.lib.t2l_last_error(eng._h).decode()
        assert f"{head}[3] = {bad} is outside [0, {C})" in msg, msg
        with pytest.raises(T2LError, match=r"\[3\]"):
            eng.pointnet_cls_heads(dx, l1, l2)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert all(not v[1].any() for v in tensors.values() if v[1] is not None)


# ---- 5. bind errors ----------------------------------------------------------------------------------------------------------------
def test_refused_binds_leave_the_previous_binding_serving(eng):
    from text2loc_amd.engine import T2LError

    x, sd, lc, lk, ref, b = R.heads_case(5, (22, 8))
    tensors = bind(eng, sd)
    dx = torch.from_numpy(x).cuda()
    want = eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR, need_grad=False)

    def still_serves():
        got = eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR, need_grad=False)
        assert all(torch.equal(got[i], want[i]) for i in range(3))
        assert eng._cls_classes == (22, 8)

    with pytest.raises(T2LError, match="completely"):  # an incomplete backbone
        bind(eng, sd, drop=(P + "sa2.point_conv.local_nn.1.0.weight",))
    still_serves()
    with pytest.raises(T2LError, match="completely"):  # no backbone at all
        bind(eng, {k: v for k, v in sd.items() if "classifier" in k})
    still_serves()
    with pytest.raises(T2LError, match="completely"):  # a backbone with gradients for some tensors only
        t = {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            d = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            t[k] = (d, None if "running_" in k or "lin1" in k else torch.zeros_like(d))
        eng.pointnet_cls_bind(t)
    still_serves()
    with pytest.raises(T2LError, match="must be bound with gradient buffers"):  # heads without gradients
        bind(eng, sd, head_grads=False)
    still_serves()
    with pytest.raises(T2LError, match="missing tensor"):
        bind(eng, sd, drop=(P + "color_classifier.bias",))
    still_serves()
    big = synth.make_pointnet_weights(0, n_classes=33, n_colors=8)
    with pytest.raises(T2LError, match="2 <= C <= 32"):  # C > 32
        bind(eng, big)
    still_serves()
    one = synth.make_pointnet_weights(0, n_classes=22, n_colors=1)
    with pytest.raises(T2LError, match="2 <= C <= 32"):
        bind(eng, one)
    still_serves()
    assert_heads(eng.pointnet_cls_heads(dx, lc, lk, R.W_CLASS, R.W_COLOR), ref, b, None, "after the refused binds")
    assert tensors[P + "class_classifier.weight"][1].any()  # ... into the FIRST binding's buffers


def test_calls_before_a_bind_are_refused():
    from text2loc_amd.engine import Engine, T2LError

    e = Engine(0)
    try:
        z = torch.zeros(1, 256, 3, device="cuda")
        with pytest.raises(T2LError, match="t2l_pointnet_cls_bind"):
            e.pointnet_cls_forward(z, z)
        with pytest.raises(T2LError, match="t2l_pointnet_cls_bind"):
            e.pointnet_cls_heads(torch.zeros(1, 256, device="cuda"), [0], [0])
        with pytest.raises(T2LError, match="t2l_pointnet_cls_bind"):
            e.pointnet_cls_backward(torch.zeros(1, 256, device="cuda"))
        bind(e, synth.make_pointnet_weights(0))
        with pytest.raises(T2LError, match="no t2l_pointnet_cls_forward to differentiate"):
            e.pointnet_cls_backward(torch.zeros(1, 256, device="cuda"))
    finally:
        e.close()
