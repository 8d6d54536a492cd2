"""CPU tier of the backbone's pretraining step (text2loc_amd/pointnet_pretrain.py, t2l_pointnet_cls_*): the float64 reference of
the heads and their loss against central differences, the committed cases' arg-max gaps, the model's key layout, the dataset of
labelled objects, the epoch permutation, and the short float64 trajectory the GPU tier leans on."""
import os.path as osp

import numpy as np
import pytest
import torch

from tests import pointnet_cls_ref as R

TINY = osp.join(osp.dirname(osp.abspath(__file__)), "golden", "k360_tiny")
SCENES = ["2013_05_28_drive_0003_sync", "2013_05_28_drive_0010_sync"]


def test_reference_gradients_match_central_differences():
    """d (w_class loss[0] + w_color loss[1]) / d {features2, weights, biases} and d / d logits (G) of the float64 reference against
    central differences of its own forward: the step and the bar of the oracle's backward (tests/test_oracle_train.py: 1e-6 scaled
    steps, 1e-5 relative)."""
    x, sd, lc, lk = R.make_heads_inputs(5, (22, 8), 1)
    sd = {k: R.f64(v) for k, v in sd.items() if "classifier" in k}
    ref = R.heads_ref(x, sd, lc, lk)

    def total(xm, sdm):
        r = R.heads_ref(xm, sdm, lc, lk)
        return R.W_CLASS * r["loss"][0] + R.W_COLOR * r["loss"][1]

    def quotient(base, idx, run):
        eps = 1e-6 * max(1.0, abs(base.ravel()[idx]))
        vals = []
        for sgn in (+1, -1):
            mod = base.copy()
            mod.ravel()[idx] += sgn * eps
            vals.append(run(mod))
        return (vals[0] - vals[1]) / (2 * eps)

    checked = 0
    x64 = R.f64(x)
    for idx in np.argsort(-np.abs(ref["dx"]).ravel())[:6]:
        num = quotient(x64, idx, lambda m: total(m, sd))
        assert abs(num - ref["dx"].ravel()[idx]) < 1e-5 * max(1.0, abs(num)), (idx, num)
        checked += 1
    for name, g in ref["grads"].items():
        for idx in np.argsort(-np.abs(g).ravel())[:4]:
            num = quotient(sd[name], idx, lambda m: total(x64, {**sd, name: m}))
            assert abs(num - g.ravel()[idx]) < 1e-5 * max(1.0, abs(num)), (name, idx, num)
            checked += 1
    # w.r.t. the logits: perturb a bias-free copy of the forward (logits + e)
    for h, (head, w) in enumerate(zip(ref["heads"], (R.W_CLASS, R.W_COLOR))):
        l = head["logits"]

        def ce_of(lm):
            m = lm.max(axis=1, keepdims=True)
            return w * float(((np.log(np.exp(lm - m).sum(axis=1)) + m[:, 0]) - lm[np.arange(len(lm)), head["labels"]]).mean())

        for idx in np.argsort(-np.abs(ref["G"][h]).ravel())[:4]:
            num = quotient(l, idx, ce_of)
            assert abs(num - ref["G"][h].ravel()[idx]) < 1e-5 * max(1.0, abs(num)), (h, idx, num)
            checked += 1
    assert checked == 6 + 4 * 4 + 2 * 4


@pytest.mark.parametrize("classes", R.HEAD_CLASSES)
@pytest.mark.parametrize("n", R.HEAD_ROWS)
def test_committed_cases_keep_every_arg_max_clear_of_rounding(n, classes):
    """Every row's top-two logit gap in float64 exceeds 100 x the row's logit bound, for both heads and no row left out: the counts
    of the GPU tier are then float64's whatever the summation order."""
    x, sd, lc, lk, ref, b = R.heads_case(n, classes)
    assert b["gap"].shape == (n, 2) and (b["gap"] > 100 * b["d"][:, None]).all()
    assert ref["logits"].shape == (n, sum(classes)) and (x >= 0).all()
    assert 70 > 2 * R.ROWS_PER_WG and 70 % R.ROWS_PER_WG  # two whole workgroups and a ragged one


def test_key_layout_is_the_reference_modules():
    """PointNet2(22, 9).state_dict() == the reference's own PointNet2(22, 9, args) (tests/golden/pointnet_keys.npz was taken with 22
    classes and 9 colours: its classifier rows say so)."""
    from text2loc_amd.pointnet_pretrain import PointNet2

    g = np.load(osp.join(osp.dirname(TINY), "pointnet_keys.npz"))
    want = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["names"], g["shapes"])}
    assert want["class_classifier.weight"] == (22, 256) and want["color_classifier.weight"] == (9, 256)
    have = {k: tuple(v.shape) for k, v in PointNet2(22, 9).state_dict().items()}
    assert have == want
    assert list(PointNet2(22, 9).state_dict().keys()) == [str(n) for n in g["names"]]


def test_model_has_no_cpu_path_and_the_criterion_has():
    from text2loc_amd.engine import T2LError
    from text2loc_amd.pointnet_pretrain import ClassifierLoss, PointNet2
    from types import SimpleNamespace

    with pytest.raises(T2LError, match="no CPU fallback"):
        PointNet2(22, 8)({"pos": torch.zeros(256, 3), "x": torch.zeros(256, 3)})
    x, sd, lc, lk, ref, _ = R.heads_case(5, (22, 8))
    bag = SimpleNamespace(class_pred=torch.from_numpy(ref["heads"][0]["logits"]), color_pred=torch.from_numpy(ref["heads"][1]["logits"]))
    crit = ClassifierLoss(R.W_CLASS, R.W_COLOR)
    loss = crit(bag, lc, lk)
    assert abs(float(loss) - (R.W_CLASS * ref["loss"][0] + R.W_COLOR * ref["loss"][1])) < 1e-12
    assert np.allclose(crit.last.loss2.numpy(), ref["loss"], rtol=0, atol=1e-12)
    assert crit.last.correct.tolist() == ref["correct"].tolist()


# ---- the dataset -------------------------------------------------------------------------------------------------------------------
def _restated_items(min_points):
    """The dataset's rule restated: distinct (scene, id) in cell order, first occurrence wins; -> kept objects, dropped counts."""
    from text2loc_amd.kitti360pose import load_pickle
    from text2loc_amd.tables import KNOWN_CLASS

    kept, seen, bad_label, small, repeats = [], set(), 0, 0, 0
    for scene in SCENES:
        for cell in load_pickle(osp.join(TINY, "cells", scene + ".pkl")):
            for o in cell.objects:
                if (scene, o.id) in seen:
                    repeats += 1
                    continue
                seen.add((scene, o.id))
                if o.label not in KNOWN_CLASS:
                    bad_label += 1
                elif len(o.xyz) < min_points:
                    small += 1
                else:
                    kept.append((scene, o))
    return kept, bad_label, small, repeats


@pytest.mark.parametrize("min_points", [25, 60, 61])
def test_dataset_items_and_labels(min_points):
    from text2loc_amd.pointnet_pretrain import Kitti360ObjectDataset
    from text2loc_amd.tables import COLORS, KNOWN_CLASS

    ds = Kitti360ObjectDataset(TINY, SCENES, min_points=min_points)
    kept, bad_label, small, repeats = _restated_items(min_points)
    assert repeats > 0  # the fixture's cells overlap: de-duplication is exercised
    if min_points == 61:  # every object of the fixture holds 60 points
        assert len(ds) == len(kept) == 0 and ds.dropped_small == small > 0
        return
    assert len(ds) == len(kept) > 0
    assert ds.keys == [(s, o.id) for s, o in kept] and len(set(ds.keys)) == len(ds.keys)
    assert (ds.dropped_label, ds.dropped_small) == (bad_label, small)
    assert ds.class_labels.dtype == np.int32 and ds.class_labels.tolist() == [KNOWN_CLASS.index(o.label) for _, o in kept]
    # the first occurrence's points are the resident ones
    cs = ds.cell_set
    assert cs.n_objects == len(kept) and all(len(o.xyz) >= min_points for _, o in kept)
    for i in (0, len(kept) // 2, len(kept) - 1):
        xyz, rgb = cs.row_points(i)
        assert np.array_equal(xyz, np.asarray(kept[i][1].xyz, dtype=np.float32)) and np.array_equal(rgb, np.asarray(kept[i][1].rgb, dtype=np.float32))
    # colour labels: nearest of the 8 centres to the mean colour, restated with a plain loop
    want = []
    for _, o in kept:
        mean = np.asarray(o.rgb, dtype=np.float64).mean(axis=0)
        want.append(int(np.argmin([np.sqrt(((mean - c) ** 2).sum()) for c in COLORS])))
    got = ds.color_labels_host()
    assert got.dtype == np.int32 and got.tolist() == want and 0 <= min(want) and max(want) < 8


def test_dataset_drops_unknown_labels_and_small_objects():
    """An object whose label is outside KNOWN_CLASS and one below the point floor are dropped (the fixture holds neither, so they are
    planted in a copy)."""
    from text2loc_amd.kitti360pose import load_pickle
    from text2loc_amd.pointnet_pretrain import Kitti360ObjectDataset

    base = Kitti360ObjectDataset(TINY, SCENES[:1])
    assert base.dropped_label == 0 and base.dropped_small == 0 and len(base) > 2
    cells = load_pickle(osp.join(TINY, "cells", SCENES[0] + ".pkl"))
    first = cells[0].objects[0]
    first.label = "spaceship"
    second = next(o for o in cells[0].objects if o.id != first.id)
    second.xyz, second.rgb = second.xyz[:24], second.rgb[:24]  # one below the default floor of 25
    ds = Kitti360ObjectDataset.from_cells([(SCENES[0], cells)])
    assert (ds.dropped_label, ds.dropped_small) == (1, 1) and len(ds) == len(base) - 2
    assert (SCENES[0], first.id) not in ds.keys and (SCENES[0], second.id) not in ds.keys
    # a later, whole occurrence of a dropped id does not bring it back: the FIRST occurrence decides
    assert sum(o.id == second.id for c in cells for o in c.objects) >= 1


def test_epoch_permutation_depends_on_seed_and_epoch_only():
    from text2loc_amd.pointnet_pretrain import epoch_permutation

    a = epoch_permutation(50, 3, 7)
    assert sorted(a.tolist()) == list(range(50))
    np.random.seed(123)  # the global stream is not read
    torch.manual_seed(5)
    assert np.array_equal(a, epoch_permutation(50, 3, 7))
    assert np.array_equal(a, np.random.default_rng([3, 7]).permutation(50))
    assert not np.array_equal(a, epoch_permutation(50, 3, 8)) and not np.array_equal(a, epoch_permutation(50, 4, 7))


def test_object_batches_refuses_a_dataloader_worker(monkeypatch):
    from text2loc_amd import pointnet_pretrain as PP

    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="object_batches works on the GPU and must run in the process that owns the engine"):
        next(PP.object_batches(None, 4))


def test_short_trajectory_in_float64_strictly_decreases():
    """4 objects as one segment, 3 Adam steps in float64 (OT.adam_step over the backbone's and the heads' gradients): the loss strictly
    decreases for the committed seed. The GPU tier's trajectory test asserts the same of the engine and leans on this."""
    losses = R.trajectory_ref()
    assert len(losses) == R.TRAJ_STEPS + 1 and np.isfinite(losses).all()
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
