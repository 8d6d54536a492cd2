"""GPU tier: t2l_sample_object_points_indexed — FixedPoints(256) (+ the transform) for a LIST OF ROWS of resident arrays.

Row r of a call samples object ``ids[r]`` under ``seed ^ salts[r]``; the reference for it is row ``ids[r]`` of the numpy restatement
(oracle/t2l_oracle_pointnet.py: sample_object_points) over the WHOLE set at that seed, held bit for bit under all three transforms
(``test_rows_equal_the_oracle``). The restatement is computed once per (set, seed, transform) and shared.

Bit equality is possible because the transforms' arithmetic is defined operation by operation on both sides (include/t2l.h): every
float32 product / sum / quotient rounded on its own, the mean of the 256 positions a float64 sum rounded once, and the angle's sine and
cosine the float32 Cody-Waite + polynomial routine that numpy's float32 loops run too (csrc/pointnet.hip: sincos_f32).
``test_rows_equal_the_whole_set_call`` holds the other half of the header's statement: row r = row ids[r] of the whole-set ENGINE call at
seed ^ salt, every bit, every transform.
"""
import numpy as np
import pytest
import torch

from oracle import t2l_oracle_pointnet as OP
from tests import guards as G
from tests.test_gpu_memory_safety import dev, engine, same_bits
from text2loc_amd import engine as E
from text2loc_amd import packing

pytestmark = pytest.mark.gpu

TRANSFORMS = ["fixed", "normalize", "rotate_normalize"]
SEED = 0x1234ABCD
SALT_POOL = np.array([0, 1, 0xDEADBEEF, 0xFFFFFFFF], dtype=np.uint32)
SIZES = {1: [257], 5: [1, 8, 255, 256, 5000], 40: [1, 8, 255, 256, 257, 5000, 60, 300] * 5}
ROW_COUNTS = [1, 16, 33, 512]


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


_sets, _oracle = {}, {}


def diff_count(a, b):
    """Elements whose BITS differ. Two NaNs count as equal whatever their sign bit: under NormalizeScale the one-point object is 0 * inf
    in the reference's transform, in the restatement (numpy on the host: the negative quiet NaN) and in the kernel (the positive one)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).sum())


def point_set(n_obj):
    """``n_obj`` objects of SIZES[n_obj] points in the cell frame, then the pad object (8 points, black) as object ``n_obj``."""
    if n_obj not in _sets:
        rs = np.random.default_rng(100 + n_obj)
        n_pts = np.array(SIZES[n_obj], dtype=np.int64)
        total = int(n_pts.sum())
        xyz = (rs.uniform(0.2, 0.8, size=(n_obj, 3)).repeat(n_pts, axis=0) + rs.standard_normal((total, 3)) * 0.05).astype(np.float32)
        rgb = rs.uniform(0, 1, size=(total, 3)).astype(np.float32)
        pad_xyz, pad_rgb = packing.PackedCellSet.pad_points()
        xyz, rgb = np.concatenate([xyz, pad_xyz]), np.concatenate([rgb, pad_rgb])
        poff = np.concatenate([[0], np.cumsum(np.append(n_pts, len(pad_xyz)))]).astype(np.int64)
        _sets[n_obj] = {"xyz": xyz, "rgb": rgb, "poff": poff, "n": n_obj + 1, "pad": n_obj,
                        "dev": (dev(xyz), dev(rgb), dev(poff))}
    return _sets[n_obj]


def oracle_rows(n_obj, ids, salts, transform):
    """Row r = row ids[r] of the restatement over the whole set at seed SEED ^ salts[r]."""
    s = point_set(n_obj)
    salts = np.zeros(len(ids), dtype=np.uint32) if salts is None else salts
    pos, col = np.empty((len(ids), 256, 3), np.float32), np.empty((len(ids), 256, 3), np.float32)
    for salt in np.unique(salts):
        key = (n_obj, int(salt), transform)
        if key not in _oracle:
            _oracle[key] = OP.sample_object_points(s["xyz"], s["rgb"], s["poff"], SEED ^ int(salt), transform=transform)
        sel = salts == salt
        pos[sel], col[sel] = _oracle[key][0][ids[sel]], _oracle[key][1][ids[sel]]
    return pos, col


def row_list(n_obj, n_rows, salted):
    """Reversed order first (so the pad row leads), the pad row again, then random rows: repeats as soon as n_rows > n_obj + 1."""
    s = point_set(n_obj)
    rs = np.random.default_rng([n_obj, n_rows])
    ids = np.concatenate([np.arange(s["n"])[::-1], [s["pad"]], rs.integers(0, s["n"], size=n_rows)])[:n_rows].astype(np.int32)
    salts = SALT_POOL[rs.integers(0, len(SALT_POOL), size=n_rows)] if salted else None
    return ids, salts


@pytest.mark.parametrize("salted", [False, True], ids=["salts-null", "salts-mixed"])
@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("n_rows", ROW_COUNTS)
@pytest.mark.parametrize("n_obj", sorted(SIZES))
def test_rows_equal_the_oracle(eng, n_obj, n_rows, transform, salted):
    s = point_set(n_obj)
    ids, salts = row_list(n_obj, n_rows, salted)
    pos, col = eng.sample_object_points_indexed(*s["dev"], ids, salts, seed=SEED, transform=transform)
    rpos, rcol = oracle_rows(n_obj, ids, salts, transform)
    p, c = pos.cpu().numpy(), col.cpu().numpy()
    print(f"set {n_obj} rows {n_rows} {transform} salted={salted}: colours differ in {diff_count(c, rcol)} elements, positions in "
          f"{diff_count(p, rpos)} of {p.size}, max |diff| {float(np.nanmax(np.abs(p - rpos))):.3e}")
    assert diff_count(c, rcol) == 0
    assert diff_count(p, rpos) == 0


@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("n_obj", sorted(SIZES))
def test_rows_equal_the_whole_set_call(eng, n_obj, transform):
    """include/t2l.h: row r equals row ids[r] of t2l_sample_object_points over the whole set at seed ^ salts[r], bit for bit."""
    s = point_set(n_obj)
    ids, salts = row_list(n_obj, 512, True)
    pos, col = eng.sample_object_points_indexed(*s["dev"], ids, salts, seed=SEED, transform=transform)
    for salt in np.unique(salts):
        wpos, wcol = eng.sample_object_points(*s["dev"], seed=SEED ^ int(salt), transform=transform)
        sel = torch.from_numpy(np.flatnonzero(salts == salt)).cuda()
        g = torch.from_numpy(ids[salts == salt].astype(np.int64)).cuda()
        assert same_bits(pos[sel], wpos[g]) and same_bits(col[sel], wcol[g])


@pytest.mark.parametrize("transform", TRANSFORMS)
def test_two_calls_equal_one(eng, transform):
    s = point_set(40)
    ids, salts = row_list(40, 512, True)
    pos, col = eng.sample_object_points_indexed(*s["dev"], ids, salts, seed=SEED, transform=transform)
    for cut in (1, 200):
        a = eng.sample_object_points_indexed(*s["dev"], ids[:cut], salts[:cut], seed=SEED, transform=transform)
        b = eng.sample_object_points_indexed(*s["dev"], ids[cut:], salts[cut:], seed=SEED, transform=transform)
        assert same_bits(torch.cat([a[0], b[0]]), pos) and same_bits(torch.cat([a[1], b[1]]), col)


def test_salts_change_the_draw_and_null_means_zero(eng):
    s = point_set(5)
    ids = np.array([4, 4, 4], dtype=np.int32)  # 5,000 points: two draws of 256 cannot coincide by chance
    a = eng.sample_object_points_indexed(*s["dev"], ids, np.array([0, 7, 7], dtype=np.uint32), seed=SEED)
    b = eng.sample_object_points_indexed(*s["dev"], ids, None, seed=SEED)
    assert same_bits(a[0][0], b[0][0]) and same_bits(a[0][1], a[0][2]) and not torch.equal(a[0][0], a[0][1])
    assert all(same_bits(b[0][0], b[0][i]) for i in (1, 2))


@pytest.mark.parametrize("bad", [-1, "n_objects + 1"])
def test_out_of_range_ids_are_refused_and_nothing_is_written(eng, bad):
    s = point_set(5)
    ids = np.array([0, 1, s["n"] + 1 if bad != -1 else -1, 2], dtype=np.int32)
    with G.guarded_outputs(E, partly_written=(0, 1)) as g:
        with pytest.raises(E.T2LError, match=r"object_ids\[2\]"):
            eng.sample_object_points_indexed(*s["dev"], ids, None, seed=SEED)
        torch.cuda.synchronize()
        assert g.count == 2
        for guard in g.guards:  # both outputs still hold the 0xA5 pattern in every word
            assert guard.unwritten_words() == guard.nbytes // 4
    # the engine serves the next call as if nothing had happened
    pos, col = eng.sample_object_points_indexed(*s["dev"], ids[:2], None, seed=SEED)
    rpos, rcol = oracle_rows(5, ids[:2], None, "fixed")
    assert np.array_equal(pos.cpu().numpy(), rpos) and np.array_equal(col.cpu().numpy(), rcol)


def test_no_rows_is_accepted(eng):
    s = point_set(1)
    pos, col = eng.sample_object_points_indexed(*s["dev"], np.zeros(0, np.int32), None, seed=SEED)
    assert pos.shape == (0, 256, 3) and col.shape == (0, 256, 3)
    pos, col = eng.sample_object_points_indexed(*s["dev"], np.zeros(0, np.int32), np.zeros(0, np.uint32), seed=SEED)
    assert pos.shape == (0, 256, 3)


def test_packed_cell_set_rows_and_its_pad_row(eng):
    """``PackedCellSet.sample_rows``: rows of the flattened dataset, the pad row behind the last object."""
    from text2loc_amd import synth

    cells, _ = synth.make_k360_records(4, 1, seed=3)
    ps = packing.PackedCellSet(cells)
    rows = np.array([ps.pad_row, 0, ps.n_objects - 1, ps.pad_row, 5], dtype=np.int32)
    salts = np.array([3, 0, 9, 4, 9], dtype=np.uint32)
    pos, col = ps.sample_rows(eng, "cuda", rows, salts, seed=11)
    xyz = np.concatenate([ps.xyz, ps.pad_points()[0]])
    rgb = np.concatenate([ps.rgb, ps.pad_points()[1]])
    poff = np.append(ps.point_offsets, ps.point_offsets[-1] + 8)
    for r, (row, salt) in enumerate(zip(rows, salts)):
        lo, hi = int(poff[row]), int(poff[row + 1])
        # the restatement keys a draw on the object's index in the arrays it is handed: hand it the whole set
        wpos, wcol = _whole(xyz, rgb, poff, 11 ^ int(salt))
        assert np.array_equal(pos[r].cpu().numpy(), wpos[row]) and np.array_equal(col[r].cpu().numpy(), wcol[row])
        assert all((xyz[lo:hi] == q).all(axis=1).any() for q in wpos[row][:8])
    assert np.array_equal(col[0].cpu().numpy(), np.zeros((256, 3), np.float32))  # the pad object is black


_whole_cache = {}


def _whole(xyz, rgb, poff, seed):
    if seed not in _whole_cache:
        _whole_cache[seed] = OP.sample_object_points(xyz, rgb, poff, seed)
    return _whole_cache[seed]
