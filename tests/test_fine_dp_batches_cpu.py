"""CPU tier: ``fine_batches(..., rank, world)`` — every global batch is the one-process batch and the ranks' contiguous slices
concatenate to it, items, per-epoch point draws and order included (the host point mode runs without a device)."""
import numpy as np
import pytest

from tests.test_fine_dataset_cpu import dataset, gold  # noqa: F401 (the fixture)
from text2loc_amd import kitti360pose as K


def same_batch(a, b):
    assert a["texts"] == b["texts"]
    assert np.array_equal(np.asarray(a["offsets"]), np.asarray(b["offsets"]))
    assert [[getattr(o, "label", None) for o in objs] for objs in a["objects"]] == [[getattr(o, "label", None) for o in objs] for objs in b["objects"]]
    assert len(a["object_points"]) == len(b["object_points"])
    for p, q in zip(a["object_points"], b["object_points"]):
        assert np.array_equal(p["pos"], q["pos"]) and np.array_equal(p["x"], q["x"])


def glue(parts):
    out = {"texts": [t for p in parts for t in p["texts"]], "offsets": np.concatenate([np.asarray(p["offsets"]) for p in parts]),
           "objects": [o for p in parts for o in p["objects"]], "object_points": [o for p in parts for o in p["object_points"]]}
    return out


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("drop_last", [True, False])
def test_the_ranks_slices_concatenate_to_the_one_process_batch(gold, world, drop_last):  # noqa: F811
    kw = dict(shuffle=True, seed=2, epoch=1, drop_last=drop_last)
    whole = list(K.fine_batches(dataset(gold, object_points="sample", seed=3), 4, "cpu", **kw))
    ranks = [list(K.fine_batches(dataset(gold, object_points="sample", seed=3), 4, "cpu", rank=r, world=world, **kw)) for r in range(world)]
    assert [len(b["texts"]) for b in whole] == ([4, 4] if drop_last else [4, 4, 3])
    # the tail of 3: two ranks split it 1 + 2, four ranks cannot all take an item and leave it
    n = 2 if (drop_last or world == 4) else 3
    assert all(len(r) == n for r in ranks)
    for i in range(n):
        assert sum(len(r[i]["texts"]) for r in ranks) == len(whole[i]["texts"])
        if i < 2:
            assert all(len(r[i]["texts"]) == 4 // world for r in ranks)  # equal shards
        same_batch(glue([r[i] for r in ranks]), whole[i])


def test_world_one_is_the_plain_loop_and_bad_splits_are_refused(gold):  # noqa: F811
    ds = dataset(gold, object_points="sample", seed=3)
    for a, b in zip(K.fine_batches(ds, 4, "cpu", rank=0, world=1), list(K.fine_batches(ds, 4, "cpu"))):
        same_batch(a, b)
    for kw in (dict(rank=0, world=3), dict(rank=2, world=2), dict(rank=-1, world=2), dict(rank=0, world=0)):
        with pytest.raises(ValueError, match="world"):
            next(K.fine_batches(ds, 4, "cpu", **kw))
    assert ds._epoch == 0
    with pytest.raises(ValueError, match="world"):
        next(K.fine_batches(ds, 4, "cpu", epoch=5, rank=0, world=3))
    assert ds._epoch == 0  # a refused call leaves the dataset's epoch alone
