"""CPU tier: text2loc_amd.plumbing, the one copy of the host plumbing between the nn.Modules and the engine. No engine is
created here: every function under test works on plain CPU tensors (or raises before it would need one)."""
import types

import numpy as np
import pytest
import torch

from text2loc_amd import plumbing
from text2loc_amd.engine import T2LError


def test_adopt_grad_hands_the_buffer_back_in_all_three_cases():
    p = torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3))
    buf = torch.full((2, 3), 7.0)
    plumbing.adopt_grad(p, buf)  # .grad None: the buffer, zeroed
    assert p.grad is buf and float(buf.abs().max()) == 0.0
    buf.fill_(3.0)
    plumbing.adopt_grad(p, buf)  # .grad already the buffer: untouched
    assert p.grad is buf and torch.equal(buf, torch.full((2, 3), 3.0))
    foreign = torch.arange(6, dtype=torch.float32).reshape(2, 3) + 0.5
    p.grad = foreign
    plumbing.adopt_grad(p, buf)  # a foreign .grad: its value, the buffer's storage
    assert p.grad.data_ptr() == buf.data_ptr() and p.grad.data_ptr() != foreign.data_ptr()
    assert torch.equal(p.grad, foreign) and torch.equal(buf, foreign)
    view = buf.view(6).view(2, 3)  # another tensor object over the same storage is the buffer too
    p.grad = view
    buf.fill_(2.0)
    plumbing.adopt_grad(p, buf)
    assert torch.equal(buf, torch.full((2, 3), 2.0))


def test_bind_key_follows_the_pointers_and_nothing_else():
    w, gw, b, rm = torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4), torch.zeros(4)
    tensors = {"w": (w, gw), "b": (b, None), "rm": (rm, None)}
    key = plumbing.bind_key(tensors)
    assert plumbing.bind_key(dict(tensors)) == key
    w.add_(1.0)  # in-place writes (an optimizer step, a backward) move no pointer
    gw.fill_(2.0)
    rm.mul_(0.9)
    assert plumbing.bind_key(tensors) == key
    assert plumbing.bind_key({"w": (w.view(16).view(4, 4), gw), "b": (b, None), "rm": (rm, None)}) == key  # same storage
    for name, pair in (("w", (w.clone(), gw)), ("w", (w, gw.clone())), ("b", (b.clone(), None)), ("b", (b, torch.zeros(4))),
                       ("w", (w, None)), ("rm", (rm.clone(), None))):
        moved = dict(tensors)
        moved[name] = pair
        assert plumbing.bind_key(moved) != key, name
    v0 = plumbing.tensors_version([w, b])
    assert plumbing.tensors_version([w, b]) == v0
    b.add_(1.0)
    assert plumbing.tensors_version([w, b]) != v0  # ... while the weights' version does see an in-place write


def _batches(rng, n_cells, per_cell):
    return [{"pos": rng.standard_normal((per_cell * 256, 3)).astype(np.float32), "x": rng.random((per_cell * 256, 3)).astype(np.float32)}
            for _ in range(n_cells)]


def test_read_object_points_round_trips_both_kinds():
    rng = np.random.default_rng(0)
    cpu = torch.device("cpu")
    feats = [rng.standard_normal((3, 256)).astype(np.float32), torch.from_numpy(rng.standard_normal((2, 256)).astype(np.float32))]
    got = plumbing.read_object_points(feats, True, cpu)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (5, 256)
    assert np.array_equal(got.numpy(), np.concatenate([feats[0], feats[1].numpy()]))
    same = [rng.standard_normal((4, 256)) for _ in range(2)]  # float64 in, float32 out
    got = plumbing.read_object_points(same, False, cpu, per_cell=4)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), np.concatenate(same).astype(np.float32))

    batches = _batches(rng, 2, 3) + _batches(rng, 1, 1)
    pos, rgb, counts = plumbing.read_object_points(batches, True, cpu)
    assert counts == [3, 3, 1] and tuple(pos.shape) == (7, 256, 3) and tuple(rgb.shape) == (7, 256, 3)
    assert pos.is_contiguous() and rgb.is_contiguous() and pos.dtype == rgb.dtype == torch.float32
    assert np.array_equal(pos.numpy().reshape(-1, 3), np.concatenate([b["pos"] for b in batches]))
    assert np.array_equal(rgb.numpy().reshape(-1, 3), np.concatenate([b["x"] for b in batches]))


def test_read_object_points_voids_the_colours_without_touching_the_callers_arrays():
    rng = np.random.default_rng(1)
    batches = _batches(rng, 2, 2)
    keep = [{k: v.copy() for k, v in b.items()} for b in batches]
    as_tensors = [{k: torch.from_numpy(v.copy()) for k, v in b.items()} for b in batches]
    for given in (batches, as_tensors):
        pos, rgb, counts = plumbing.read_object_points(given, False, torch.device("cpu"), per_cell=2)
        assert counts == [2, 2] and float(rgb.abs().max()) == 0.0 and tuple(rgb.shape) == (4, 256, 3)
        assert np.array_equal(pos.numpy().reshape(-1, 3), np.concatenate([b["pos"] for b in keep]))
    assert all(np.array_equal(b[k], c[k]) for b, c in zip(batches, keep) for k in b)
    assert all(np.array_equal(b[k].numpy(), c[k]) for b, c in zip(as_tensors, keep) for k in b)
    assert float(np.abs(keep[0]["x"]).max()) > 0  # (there were colours to void)


def test_read_object_points_takes_attributes_and_keys_alike():
    rng = np.random.default_rng(2)
    batches = _batches(rng, 3, 2)
    attrs = [types.SimpleNamespace(pos=torch.from_numpy(b["pos"]), x=torch.from_numpy(b["x"])) for b in batches]
    assert plumbing.is_point_batch(batches[0]) and plumbing.is_point_batch(attrs[0])
    assert not plumbing.is_point_batch(batches[0]["pos"]) and not plumbing.is_point_batch(torch.zeros(2, 256))
    for use_color in (True, False):
        a = plumbing.read_object_points(batches, use_color, torch.device("cpu"), per_cell=2)
        b = plumbing.read_object_points(attrs, use_color, torch.device("cpu"), per_cell=2)
        assert a[2] == b[2] == [2, 2, 2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_read_object_points_refusals():
    rng = np.random.default_rng(3)
    cpu = torch.device("cpu")
    batches = _batches(rng, 2, 16)
    feats = [torch.zeros(16, 256), torch.zeros(16, 256)]
    for bad in (None, [feats[0], None], [None, batches[1]]):
        with pytest.raises(T2LError, match="object_points must hold"):
            plumbing.read_object_points(bad, True, cpu)
    for bad in ([batches[0], feats[1]], [feats[0], batches[1]], [batches[0], np.zeros((16, 256), np.float32)]):
        with pytest.raises(T2LError, match="mixes point batches and features2"):
            plumbing.read_object_points(bad, True, cpu, per_cell=16)
    short = [{"pos": b["pos"][:15 * 256], "x": b["x"][:15 * 256]} for b in batches]
    with pytest.raises(T2LError, match="16\\*256 points"):
        plumbing.read_object_points(short, True, cpu, per_cell=16)
    with pytest.raises(T2LError, match="16\\*256 points"):  # .x shorter than .pos
        plumbing.read_object_points([{"pos": batches[0]["pos"], "x": batches[0]["x"][:256]}], True, cpu, per_cell=16)
    with pytest.raises(T2LError, match="16\\*256 points"):  # no .x at all
        plumbing.read_object_points([types.SimpleNamespace(pos=batches[0]["pos"])], True, cpu, per_cell=16)
    with pytest.raises(T2LError, match="features2 must be \\[16,256\\] per cell"):
        plumbing.read_object_points([torch.zeros(15, 256), torch.zeros(16, 256)], True, cpu, per_cell=16)
    with pytest.raises(T2LError, match="features2 must be \\[16,256\\] per cell"):  # the right count of numbers in the wrong shape
        plumbing.read_object_points([torch.zeros(8, 512), torch.zeros(8, 512)], True, cpu, per_cell=16)
    assert tuple(plumbing.read_object_points(short, True, cpu)[0].shape) == (30, 256, 3)  # no per_cell: ragged cells are the coarse stage's


def test_bump_batches_tracked_counts_the_backbone_once_per_cell():
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.BatchNorm1d(4))
            self.head = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))
            self.unused = torch.nn.Sequential(torch.nn.BatchNorm1d(4))
            self.untracked = torch.nn.BatchNorm1d(4, track_running_stats=False)

    net = Net()
    tracked = lambda: {n: int(m.num_batches_tracked) for n, m in net.named_modules()
                       if isinstance(m, torch.nn.BatchNorm1d) and m.num_batches_tracked is not None}
    assert set(tracked()) == {"backbone.1", "backbone.2", "head.1", "unused.0"}
    used = lambda name: not name.startswith("unused.")
    plumbing.bump_batches_tracked(net.named_modules(), used, "backbone.", 5)
    assert tracked() == {"backbone.1": 5, "backbone.2": 5, "head.1": 1, "unused.0": 0}
    plumbing.bump_batches_tracked(net.named_modules(), used, "backbone.", 0)  # a step that did not run the backbone
    assert tracked() == {"backbone.1": 5, "backbone.2": 5, "head.1": 2, "unused.0": 0}
    plumbing.bump_batches_tracked(net.named_modules(), lambda name: False, "backbone.", 3)
    assert tracked() == {"backbone.1": 5, "backbone.2": 5, "head.1": 2, "unused.0": 0}
    assert net.backbone[1].num_batches_tracked.dtype == torch.int64


def test_engine_for_refuses_a_cpu_device_before_it_needs_an_engine():
    for match in ("MI355X only", "no CPU fallback", "the widget runs on the MI355X"):
        with pytest.raises(T2LError, match=match):
            plumbing.engine_for(None, torch.device("cpu"), "the widget")


def test_the_losses_refuse_cpu_tensors_by_name():
    from text2loc_amd import losses

    with pytest.raises(T2LError, match="the loss runs on the MI355X only"):
        losses._engine_for(torch.device("cpu"))
    with pytest.raises(T2LError, match="no CPU fallback"):
        losses.ContrastiveLoss(0.1)(torch.randn(4, 256, requires_grad=True), torch.randn(4, 256))


def test_fine_stage_refuses_object_points_for_another_number_of_cells():
    """The engine takes the cell count from ``objects`` and reads 16 rows of features2 per cell: a list for fewer (or more) cells must
    be refused on the host, in both modes, before anything reaches the device (here: before the device error of a CPU model)."""
    from tests.test_host_logic import make_objects
    from tests.test_oracle_fine_train import fine_args
    from text2loc_amd import synth
    from text2loc_amd.cross_matcher import CrossMatch, pad_objects

    cells = synth.make_cells(2, seed=1, min_obj=16, max_obj=16)
    objects = [pad_objects(o) for o in make_objects(cells, 1)]
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, fine_args(False), language_encoder=torch.nn.Identity()).train()
    hints = torch.zeros(2, 6, 128)
    batch = lambda: {"pos": np.zeros((16 * 256, 3), np.float32), "x": np.zeros((16 * 256, 3), np.float32)}
    for n in (1, 3):
        with pytest.raises(T2LError, match="exactly the objects of each cell: 2 cells of 16, got %d objects" % (16 * n)):
            model(objects, hints, [torch.zeros(16, 256) for _ in range(n)])
        with pytest.raises(T2LError, match="exactly the objects of each cell: 2 cells of 16"):
            model(objects, hints, [batch() for _ in range(n)])
    with pytest.raises(T2LError, match="MI355X only"):  # the right count gets as far as the device check
        model(objects, hints, [torch.zeros(16, 256) for _ in range(2)])
    for n in (1, 3):
        with pytest.raises(T2LError, match="2 cells of 16, got %d objects" % (16 * n)):
            model._read_points(objects, [torch.zeros(16, 256) for _ in range(n)])
    assert tuple(model._read_points(objects, [torch.zeros(16, 256)] * 2).shape) == (32, 256)


def test_stale_forward_token():
    owner = types.SimpleNamespace(_tok=None)
    first = plumbing.new_token(owner, "_tok")
    plumbing.check_token(owner, "_tok", first, "widget call")
    second = plumbing.new_token(owner, "_tok")
    assert second is not first and owner._tok is second
    with pytest.raises(T2LError, match="stale widget call"):
        plumbing.check_token(owner, "_tok", first, "widget call")
    plumbing.check_token(owner, "_tok", second, "widget call")


def test_helpers_stay_importable_from_cell_retrieval():
    from text2loc_amd import cell_retrieval

    assert cell_retrieval.is_point_batch is plumbing.is_point_batch
    assert cell_retrieval.point_batch_tensors is plumbing.point_batch_tensors
    assert cell_retrieval._point_field is plumbing._point_field
