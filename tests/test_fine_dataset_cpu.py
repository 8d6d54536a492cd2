"""CPU tier: ``kitti360pose.Kitti360FineDataset`` on tests/golden/k360_fine_tiny — pickles written with the reference's own classes and
the items its ``Kitti360FineDatasetMulti`` returned for them (tools/gen_golden_fine_dataset.py) — read with no reference on sys.path.
Two scenes, cells of 3 to 20 objects (padding and the cut at 16), poses with 0, 1, 3 and 6 matched hints, one matched object from
position 18 of its cell."""
import argparse
import os.path as osp
import sys

import numpy as np
import pytest

from text2loc_amd import kitti360pose as K
from text2loc_amd import packing
from text2loc_amd.cross_matcher import PadObject

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
BASE = osp.join(GOLDEN, "k360_fine_tiny")
KEYS = ["poses", "cells", "objects", "object_points", "hint_descriptions", "texts", "matches", "all_matches", "offsets",
        "offsets_best_center", "object_class_indices", "object_color_indices"]


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "k360_fine_tiny.npz"), allow_pickle=False)


def make_args(setting="all/center", **over):
    cell, learn = setting.split("/")
    a = argparse.Namespace(pad_size=16, num_mentioned=6, regressor_cell=cell, regressor_learn=learn)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def dataset(gold, setting="all/center", **kw):
    return K.Kitti360FineDataset(BASE, [str(s) for s in gold["scenes"]], make_args(setting), **kw)


@pytest.mark.parametrize("k", range(5))
def test_every_item_equals_the_reference(gold, k):
    assert not any("reference" in p for p in sys.path)
    setting = str(gold["settings"][k])
    ds = dataset(gold, setting)
    p = f"r{k}_"
    assert len(ds) == len(gold[p + "texts"]) == 11
    assert sorted(set(gold[p + "matches_n"].tolist())) == [0, 1, 3, 6]
    m_at = np.concatenate([[0], np.cumsum(gold[p + "matches_n"])])
    a_at = np.concatenate([[0], np.cumsum(gold[p + "all_matches_n"])])
    for i in range(len(ds)):
        it = ds[i]
        assert list(it.keys()) == KEYS and it["object_points"] is None
        assert it["poses"].cell_id == it["cells"].id == str(gold[p + "pose_cell_ids"][i])
        assert np.array_equal(it["poses"].pose, gold[p + "pose_in_cell"][i])
        assert [getattr(o, "id", -1) for o in it["objects"]] == gold[p + "object_ids"][i].tolist()
        assert [o.label for o in it["objects"]] == [str(s) for s in gold[p + "object_labels"][i]]
        assert [len(o.xyz) for o in it["objects"]] == gold[p + "object_npts"][i].tolist()
        assert [isinstance(o, PadObject) for o in it["objects"]] == (gold[p + "object_ids"][i] == -1).tolist()
        assert it["texts"] == str(gold[p + "texts"][i])
        assert list(it["hint_descriptions"]) == [str(s) for s in gold[p + "hint_descriptions"][i]]
        assert np.array_equal(np.asarray(it["matches"]).reshape(-1, 2), gold[p + "matches"][m_at[i]:m_at[i + 1]])
        assert np.array_equal(it["all_matches"], gold[p + "all_matches"][a_at[i]:a_at[i + 1]])
        assert it["offsets"].shape == gold[p + "offsets"][i].shape and np.array_equal(it["offsets"], gold[p + "offsets"][i])
        assert np.array_equal(it["offsets_best_center"], gold[p + "offsets_best_center"][i])
        assert it["object_class_indices"] == gold[p + "object_class_indices"][i].tolist()
        assert it["object_color_indices"] == gold[p + "object_color_indices"][i].tolist()


def test_the_fixture_pads_cuts_and_reaches_past_position_16(gold):
    ds = dataset(gold)
    counts = gold["cell_counts"].tolist()
    assert min(counts) == 3 and max(counts) == 20 and [len(c.objects) for c in ds.all_cells] == counts
    assert max(len(o.xyz) for c in ds.all_cells for o in c.objects) <= 60
    late = [i for i in range(len(ds)) for d in ds.all_poses[i].descriptions
            if d.is_matched and [o.id for o in ds[i]["cells"].objects].index(d.object_id) >= 16]
    assert late, "no matched object beyond position 16 of its cell"
    it = ds[late[0]]
    assert it["objects"][0].id in [d.object_id for d in it["poses"].descriptions if d.is_matched] and len(it["objects"]) == 16
    assert any(isinstance(o, PadObject) for i in range(len(ds)) for o in ds[i]["objects"])


def test_collate_and_known_classes(gold):
    ds = dataset(gold)
    batch = K.Kitti360FineDataset.collate_fn([ds[0], ds[3], ds[5]])
    assert list(batch.keys()) == KEYS and all(isinstance(v, list) and len(v) == 3 for v in batch.values())
    assert batch["texts"][1] == ds[3]["texts"] and batch["objects"][2] == ds[5]["objects"]
    assert np.asarray(batch["offsets"]).shape == (3, 2)  # regressor_cell "all": what train_epoch turns into its [B,2] target
    assert ds.get_known_classes() == [str(c) for c in gold["known_classes"]] and "pad" in ds.get_known_classes()


def test_in_memory_records(gold):
    scenes = [str(s) for s in gold["scenes"]]
    records = {s: K.load_scene(BASE, s) for s in scenes}
    ds, ref = K.Kitti360FineDataset(records, scenes, make_args()), dataset(gold)
    assert len(ds) == len(ref) and all(ds[i]["texts"] == ref[i]["texts"] for i in range(len(ds)))
    one = K.Kitti360FineDataset.from_records(*records[scenes[1]], make_args())
    assert len(one) == len(records[scenes[1]][1]) and np.array_equal(one[0]["offsets"], ref[len(records[scenes[0]][1])]["offsets"])


def test_map_cloning_is_refused_and_flip_pose_is_ignored(gold):
    with pytest.raises(NotImplementedError, match="new_matching") as e:
        dataset(gold, pmc_prob=0.3)
    for needle in ("poses.py:427-433", "keyed by obj.id", "add_relation.py:71", "json.dump"):
        assert needle in str(e.value)
    flipped, plain = dataset(gold, flip_pose=True), dataset(gold)
    for i in range(len(plain)):  # load_pose_and_cell never reads its flip arguments: the same items
        a, b = flipped[i], plain[i]
        assert a["texts"] == b["texts"] and np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["all_matches"], b["all_matches"])
        assert [getattr(o, "id", -1) for o in a["objects"]] == [getattr(o, "id", -1) for o in b["objects"]]
        assert all(np.array_equal(x.xyz, y.xyz) for x, y in zip(a["objects"], b["objects"]))  # nothing mirrored
    with pytest.raises(ValueError, match="regressor"):
        K.Kitti360FineDataset(BASE, [str(s) for s in gold["scenes"]], make_args("nearest/center"))


def test_host_sampled_points_are_redrawn_per_epoch(gold):
    ds = dataset(gold, object_points="sample", seed=3)
    a, b = ds[1]["object_points"], ds[1]["object_points"]
    assert a["pos"].shape == a["x"].shape == (16 * 256, 3) and np.array_equal(a["pos"], b["pos"])
    ds.set_epoch(1)
    assert not np.array_equal(ds[1]["object_points"]["pos"], a["pos"])


def test_object_rows_name_the_items_objects(gold):
    ds = dataset(gold, object_points="ids")
    ps = ds.packed()
    assert ps.pad_row == ps.n_objects == int(gold["cell_counts"].sum())
    for i in range(len(ds)):
        it = ds[i]
        assert it["object_points"] is None and it["object_rows"].dtype == np.int32 and it["object_rows"].shape == (16,)
        assert it["draw_salts"].dtype == np.uint32 and it["draw_salts"].shape == (16,)
        for obj, row in zip(it["objects"], it["object_rows"]):
            xyz, rgb = ps.row_points(row)
            assert (row == ps.pad_row) == isinstance(obj, PadObject)
            assert np.array_equal(xyz, np.asarray(obj.xyz, dtype=np.float32)) and np.array_equal(rgb, np.asarray(obj.rgb, dtype=np.float32))
            if row != ps.pad_row:
                assert ps.labels[row] == obj.label
    pad_xyz, pad_rgb = ps.row_points(ps.pad_row)
    assert pad_xyz.shape == (8, 3) and not pad_rgb.any()
    with pytest.raises(IndexError):
        ps.row_points(ps.pad_row + 1)


def test_salts(gold):
    ds = dataset(gold, object_points="ids", seed=5)
    n = len(ds)
    e0 = np.stack([ds[i]["draw_salts"] for i in range(n)])
    assert len(np.unique(e0)) == e0.size  # slots and items
    assert np.array_equal(e0, np.stack([K.draw_salts(0, i, 16) for i in range(n)]))
    ds.set_epoch(1)
    e1 = np.stack([ds[i]["draw_salts"] for i in range(n)])
    assert len(np.unique(np.concatenate([e0, e1]))) == 2 * e0.size  # epochs
    again = dataset(gold, object_points="ids", seed=5)
    again.set_epoch(1)
    assert np.array_equal(e1, np.stack([again[i]["draw_salts"] for i in range(n)]))  # equal (seed, epoch): equal salts
    # the documented hash, restated: mix(mix(mix(epoch + 0x9E3779B9) ^ item) ^ slot), mix = lowbias32
    def mix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    assert int(K.draw_salts(3, 7, 16)[5]) == mix(mix(mix(3 + 0x9E3779B9) ^ 7) ^ 5)


def test_fine_batches_refuses_to_run_in_a_worker(gold, monkeypatch):
    import torch.utils.data

    ds = dataset(gold, object_points="ids")
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="DataLoader worker"):
        next(K.fine_batches(ds, 4, "cuda"))


def test_fine_batches_collates_host_modes_without_a_gpu(gold):
    ds = dataset(gold)
    batches = list(K.fine_batches(ds, 4, "cpu"))
    assert [len(b["texts"]) for b in batches] == [4, 4, 3] and batches[0]["object_points"] == [None] * 4
    assert [len(b["texts"]) for b in K.fine_batches(ds, 4, "cpu", drop_last=True)] == [4, 4]
    a = [t for b in K.fine_batches(ds, 4, "cpu", shuffle=True, seed=2, epoch=1) for t in b["texts"]]
    b = [t for b in K.fine_batches(ds, 4, "cpu", shuffle=True, seed=2, epoch=1) for t in b["texts"]]
    c = [t for b in K.fine_batches(ds, 4, "cpu", shuffle=True, seed=2, epoch=2) for t in b["texts"]]
    assert a == b and a != c and sorted(a) == sorted(c) == sorted(t for bb in batches for t in bb["texts"])


def test_datasets_from_args(gold):
    scenes = [str(s) for s in gold["scenes"]]
    args = make_args(base_path=BASE, no_pc_augment=False, pmc_prob=0.0)
    tr, va, te = K.fine_datasets_from_args(args, scenes=([scenes[0]], [scenes[1]], scenes))
    assert (tr.point_transform, va.point_transform, te.point_transform) == ("rotate_normalize", "normalize", "normalize")
    assert (len(tr), len(va), len(te)) == (6, 5, 11) and tr.point_mode == "sample"
    args.no_pc_augment = True
    assert packing.fine_train_transforms_from_args(args) == ("fixed", "fixed")
    args.pmc_prob = 0.5
    with pytest.raises(NotImplementedError):
        K.fine_datasets_from_args(args, scenes=([scenes[0]], [scenes[1]], scenes))
