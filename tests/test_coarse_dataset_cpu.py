"""CPU tier: ``Kitti360PoseDataset(object_points="ids")`` and ``coarse_batches`` — the coarse training items without a copied cell.

An "ids" item makes the augmentation draws of a "sample" item in the same order (one ``choice`` over the hints, two
``choice((True, False))``), so equal ``RandomState`` seeds give equal texts, cells, flipped poses and flip decisions, item for item;
what it does NOT do is copy and mirror the cell. The flips are a code (bit 0 horizontal, bit 1 vertical) that the device applies as
``float32(1) - x`` to the points it gathers (tests/coarse_batch_ref.py restates it); ``test_restated_mirror_*`` hold that restatement
against the points ``flip_pose_in_cell`` produces.
"""
import os.path as osp

import numpy as np
import pytest

from tests import coarse_batch_ref as R
from tests.conftest import GOLDEN
from text2loc_amd import kitti360pose as K
from text2loc_amd import synth

BASE = osp.join(GOLDEN, "k360_tiny")
AUG = dict(shuffle_hints=True, flip_poses=True)


def _pairs():
    """(name, make(object_points, seed) -> dataset) over the k360_augment golden's inputs and over synthetic records."""
    g = np.load(osp.join(GOLDEN, "k360_augment.npz"), allow_pickle=False)
    scenes = [str(s) for s in g["scenes"]]
    cells, poses = synth.make_k360_records(12, 40, seed=5)
    return [("golden", lambda mode, s: K.Kitti360PoseDataset(BASE, scenes, object_points=mode, aug_rng=np.random.RandomState(s), **AUG),
             [int(s) for s in g["seeds"]]),
            ("synth", lambda mode, s: K.Kitti360PoseDataset.from_records(cells, poses, object_points=mode, aug_rng=np.random.RandomState(s), **AUG),
             [0, 7])]


def _flips(item, plain_pose):
    """The two flip decisions as the pose shows them (a pose-in-cell coordinate of exactly 0.5 would hide one; none is)."""
    p, q = np.asarray(item["poses"].pose, dtype=np.float64), np.asarray(plain_pose.pose, dtype=np.float64)
    return int(p[0] != q[0]) | (int(p[1] != q[1]) << 1)


@pytest.mark.parametrize("which", [0, 1], ids=["golden", "synth"])
def test_ids_items_equal_sample_items_draw_for_draw(which):
    name, make, seeds = _pairs()[which]
    codes = set()
    for s in seeds:
        a, b = make("sample", s), make("ids", s)
        before = [[(id(o), id(o.xyz)) for o in c.objects] for c in b.all_cells]
        for i in range(len(a)):
            x, y = a[i], b[i]
            assert x["texts"] == y["texts"] and x["cell_ids"] == y["cell_ids"] and x["scene_names"] == y["scene_names"]
            assert np.array_equal(np.asarray(x["poses"].pose), np.asarray(y["poses"].pose))
            assert np.array_equal(np.array([d.closest_point for d in x["poses"].descriptions]),
                                  np.array([d.closest_point for d in y["poses"].descriptions]))
            assert list(x["debug_hint_descriptions"]) == list(y["debug_hint_descriptions"])
            assert y["mirror"] == _flips(x, a.all_poses[i]) == _flips(y, b.all_poses[i])
            codes.add(y["mirror"])
            # the resident record itself, its objects untouched; the flipped pose is a copy
            assert y["cells"] is b.cells_dict[y["cell_ids"]] and y["objects"] is y["cells"].objects and y["object_points"] is None
            assert y["cells"] is b.all_cells[y["cell_row"]]
            assert (y["poses"] is b.all_poses[i]) == (y["mirror"] == 0)
            if y["mirror"]:
                assert x["cells"] is not a.cells_dict[x["cell_ids"]]  # ("sample" copied its cell)
        assert [[(id(o), id(o.xyz)) for o in c.objects] for c in b.all_cells] == before
        plain = make(None, s)
        for c, d in zip(b.all_cells, plain.all_cells):
            assert all(np.array_equal(o.xyz, p.xyz) for o, p in zip(c.objects, d.objects))
        assert all(np.array_equal(p.pose, q.pose) for p, q in zip(b.all_poses, plain.all_poses))
    assert codes == {0, 1, 2, 3}, codes


def test_object_rows_index_the_packed_set():
    _, make, _ = _pairs()[1]
    ds = make("ids", 1)
    ps = ds.packed()
    assert ps is ds.get_cell_dataset().packed()  # flattened once, shared with the evaluation side
    for i in range(len(ds)):
        it = ds[i]
        rows = it["object_rows"]
        assert rows.dtype == np.int32 and len(rows) == len(it["objects"]) == len(it["draw_salts"])
        assert it["draw_salts"].dtype == np.uint32
        for r, o in zip(rows, it["objects"]):
            xyz, rgb = ps.row_points(int(r))
            assert np.array_equal(xyz, np.asarray(o.xyz, dtype=np.float32)) and np.array_equal(rgb, np.asarray(o.rgb, dtype=np.float32))
            assert ps.labels[int(r)] == o.label


def test_salts_differ_across_slot_item_and_epoch_and_repeat():
    _, make, _ = _pairs()[1]
    ds = make("ids", 1)
    seen = {}
    for epoch in (0, 1, 2):
        ds.set_epoch(epoch)
        for i in range(len(ds)):
            salts = ds[i]["draw_salts"]
            assert np.array_equal(salts, K.draw_salts(epoch, i, len(salts)))
            assert np.array_equal(salts, ds[i]["draw_salts"])  # equal (epoch, item): the same salts
            for slot, v in enumerate(salts.tolist()):
                seen.setdefault(v, []).append((epoch, i, slot))
    clashes = [v for v in seen.values() if len(set(v)) > 1]
    assert not clashes, clashes[:3]


def _records(dtype, lo, hi, seed):
    """One cell of 5 objects with ``dtype`` points uniform in [lo, hi]^3."""
    rs = np.random.default_rng(seed)
    objs = []
    for n in (1, 2, 37, 300, 4000):
        o = K.ObjectRecord()
        o.__dict__.update(id=len(objs), xyz=rs.uniform(lo, hi, size=(n, 3)).astype(dtype), rgb=rs.uniform(0, 1, size=(n, 3)).astype(np.float32),
                          label="building")
        objs.append(o)
    c = K.CellRecord()
    c.__dict__.update(id="c0", objects=objs, cell_size=30.0, bbox_w=np.array([0, 0, 0, 30, 30, 30.0]))
    return c


@pytest.mark.parametrize("code", [1, 2, 3])
def test_restated_mirror_equals_the_host_flip_on_float32_records(code):
    """float32 points: ``1 - xyz`` in ``flip_pose_in_cell`` is numpy's float32 subtraction — the restatement's, bit for bit."""
    cell = _records(np.float32, -1.0, 2.0, code)
    flipped = R.host_flipped_cell(cell, code)
    for o, f in zip(cell.objects, flipped.objects):
        assert f.xyz.dtype == np.float32 and f.xyz is not o.xyz
        assert np.array_equal(R.mirror_points(o.xyz, code).view(np.uint32), f.xyz.view(np.uint32))


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 2.0)])
def test_restated_mirror_is_within_one_float32_step_on_float64_records(lo, hi):
    """float64 points x in [-1, 2]. The device sees xf = float32(x) and forms a = fl32(u), u = 1 - xf; the host flip forms v = 1 - x in
    float64 and the packer rounds it, b = fl32(v). |u - v| = |xf - x| =: d. The bound |a - b| <= 2^-23:
      x in [0.5, 2]: xf / 2 <= 1 <= 2 xf, so u is exact in float32 (Sterbenz): a = u. d <= 2^-24 (half a float32 step below 2) and
        |v| <= 1, so |b - v| <= 2^-25: |a - b| <= 2^-24 + 2^-25 < 2^-23.
      x in [-1, 0.5): d <= 2^-25 (half a step below 1; 0 at x = -1), and u, v lie in (0.5, 2], where float32 steps are 2^-24 or 2^-23.
        Rounding is monotone and [u, v] is shorter than the steps around it, so it holds at most one rounding boundary: a and b are
        the same float32 value or neighbours, |a - b| <= 2^-23.
    float64's own rounding of 1 - x moves v by 2^-53: the first case keeps its slack, the interval of the second stays shorter than a
    step. Measured over 4e6 draws: 6.0e-8 on [0, 1], 1.19e-7 = 2^-23 on [-1, 2] — the bound is attained."""
    rs = np.random.default_rng(11)
    worst = 0.0
    for code in (1, 2, 3):
        o = K.ObjectRecord()
        o.__dict__.update(id=0, xyz=rs.uniform(lo, hi, size=(200000, 3)), rgb=np.zeros((200000, 3), np.float32), label="building")
        cell = K.CellRecord()
        cell.__dict__.update(id="c", objects=[o])
        f = R.host_flipped_cell(cell, code).objects[0]
        assert f.xyz.dtype == np.float64
        d = np.abs(R.mirror_points(o.xyz, code).astype(np.float64) - f.xyz.astype(np.float32).astype(np.float64))
        for ax in (0, 1, 2):
            if not (ax < 2 and (code >> ax) & 1):
                assert d[:, ax].max() == 0.0  # an axis the code leaves alone is the float32 cast on both sides
        worst = max(worst, float(d.max()))
    print(f"[{lo}, {hi}]: max |restated - host flip| = {worst:.3e} (bound {2.0 ** -23:.3e})")
    assert worst <= 2.0 ** -23


def test_coarse_batches_refusals_and_surface(monkeypatch):
    _, make, _ = _pairs()[1]
    ds = make("ids", 1)
    with pytest.raises(ValueError, match="positive"):
        K.coarse_batches(ds, 0, "cuda")
    with pytest.raises(ValueError, match="positive"):
        K.coarse_batches(ds, -3, "cuda")
    with pytest.raises(ValueError, match="object_points"):
        K.Kitti360PoseDataset.from_records(ds.all_cells, ds.all_poses, object_points="bogus")
    cb = K.coarse_batches(ds, 16, "cuda", drop_last=True)
    assert cb.dataset is ds and len(cb) == len(ds) // 16 and len(K.coarse_batches(ds, 16, "cuda")) == (len(ds) + 15) // 16
    monkeypatch.setattr(K.torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="DataLoader worker"):
        K.coarse_batches(ds, 4, "cuda")
    with pytest.raises(RuntimeError, match="DataLoader worker"):
        iter(cb).__next__()


def test_coarse_batches_without_points_collates_on_the_host():
    """An "ids" dataset built with ``points=False`` (embedding mode reads no points) touches no GPU while batching: the batches carry
    the rows and codes ``plumbing.pack_objects`` gathers by, in a shuffled order that (seed, epoch) fixes."""
    cells, poses = synth.make_k360_records(12, 40, seed=5)

    def batches(seed, epoch):
        ds = K.Kitti360PoseDataset.from_records(cells, poses, object_points="ids", points=False, aug_rng=np.random.RandomState(2), **AUG)
        ds.set_epoch(epoch)
        return ds, list(K.coarse_batches(ds, 16, "cuda", shuffle=True, seed=seed))

    ds, got = batches(3, 1)
    assert not ds.wants_points and [len(b["texts"]) for b in got] == [16, 16, 8]
    b = got[0]
    assert isinstance(b["objects"], list) and b["objects"].cell_set is ds.packed()
    assert b["objects"].mirror.dtype == np.uint8 and b["objects"].mirror.tolist() == b["mirror"]
    assert all(o is c.objects for o, c in zip(b["objects"], b["cells"])) and b["object_points"] == [None] * 16
    assert all(np.array_equal(r, q) for r, q in zip(b["objects"].object_rows, b["object_rows"]))
    _, again = batches(3, 1)
    assert [x["texts"] for x in again] == [x["texts"] for x in got]
    _, other = batches(3, 2)
    assert [x["cell_ids"] for x in other] != [x["cell_ids"] for x in got]
