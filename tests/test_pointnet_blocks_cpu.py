"""CPU tier of the PointNet++ block tests: proves the float64 stage references, their derived tolerances and the
geometry fixtures of tests/pointnet_blocks.py before a GPU sees them (tests/test_gpu_pointnet_blocks.py).

* consistency: the float32 restatement (oracle/t2l_oracle_pointnet.py, run stage by stage) and a numpy model of every arm's operand
  rounding stay inside every stage's tolerance;
* mutants: each fault of the ball query, the sampling order or the self-loop index puts at least one element of the level it touches
  outside that level's tolerance (or breaks that level's centre equality);
* the geometry and magnitude fixtures carry the conditions they were built for."""
import functools

import numpy as np
import pytest

from oracle import t2l_oracle_pointnet as OP
from tests import pointnet_blocks as PB

F32 = np.float32


@functools.lru_cache(maxsize=None)
def sd():
    return PB.weights(0)


@functools.lru_cache(maxsize=None)
def table():
    """the table fixture and the restatement's levels of it, per self-loop option"""
    pos, rgb, off = PB.table_fixture()
    out = {}
    for loops in (True, False):
        f2, levels, f0 = OP.pointnet_features(pos, rgb, off, sd(), pyg_self_loops=loops, return_levels=True)
        lv = {"f0": f0, "f2": f2, "f1": np.maximum(f0 @ sd()[PB.PREFIX + "lin1.weight"].T + sd()[PB.PREFIX + "lin1.bias"], F32(0))}
        for L, (p, x, _) in enumerate(levels):
            lv[f"p{L + 1}"], lv[f"x{L + 1}"] = p, x
        out[loops] = lv
    return pos, rgb, off, out


@pytest.mark.parametrize("loops", [True, False])
def test_the_float32_restatement_stays_inside_every_stage_tolerance(loops):
    pos, rgb, off, lv = table()
    r, _ = PB.hold_all(lv[loops], pos, rgb, off, sd(), loops, "f32")
    assert all(v <= 1.0 for v in r.values()), r
    assert min(r[k] for k in ("x1", "x2", "x3", "f0", "f1", "f2")) > 0.0  # really another computation
    counts = PB.in_radius(pos, lv[loops]["p1"], 0.2).sum(axis=-1)
    assert counts.min() == 1 and counts.max() > 32  # lone and saturated balls both occur


@pytest.mark.parametrize("arm", ["f32", "split", "f16"])
def test_a_model_of_each_arm_stays_inside_its_tolerance(arm):
    """operands rounded as the arm's packing rounds them, float32 BatchNorm fold, sums in float64: inside the arm's bound at every
    MLP stage, and outside the next tighter arm's somewhere (the bounds tell the arms apart)"""
    pos, rgb, off, lv = table()
    lv = lv[True]
    src = [(pos, rgb), (lv["p1"], lv["x1"]), (lv["p2"], lv["x2"])]
    worst = {}
    for L in range(3):
        rows, valid = PB.sa_rows(*src[L], lv[f"p{L + 1}"], off, PB.LEVELS[L][0], True)
        prefix = f"{PB.PREFIX}{PB.LEVELS[L][1]}.point_conv.local_nn"
        st = PB.mlp2_max(rows, valid, sd(), prefix, ("f32", "split", "f16"))
        got = PB.model_mlp2_max(rows, valid, sd(), prefix, arm)
        worst[L] = {a: PB.ratio(got, st.ref, st.tol[a]) for a in PB.ARMS}
    rows = np.concatenate([lv["x3"], lv["p3"]], axis=-1).astype(np.float64)
    st = PB.ga(lv["x3"], lv["p3"], sd(), ("f32", "split", "f16"))
    got = PB.model_mlp2_max(rows, np.ones(rows.shape[:2], bool), sd(), PB.PREFIX + "ga.mlp", arm)
    worst[3] = {a: PB.ratio(got, st.ref, st.tol[a]) for a in PB.ARMS}
    assert all(w[arm] <= 1.0 for w in worst.values()), worst
    if arm == "f16":
        assert any(w["split"] > 1.0 for w in worst.values()), worst  # plain f16 leaves the split bound (worst-case bounds: level 1 shows it)


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def level_sees(mutant, L, src_p, src_x, off, loops=True, arm="split"):
    """Does level L (0..2) notice ``mutant``? The mutated reference (a kernel with that fault, computed exactly) against the
    unmutated one at ``arm``'s tolerance; a mutant of the sampling is seen by the centres."""
    good_p, bad_p = PB.centres(src_p), PB.centres(src_p, mutant)
    if not np.array_equal(good_p, bad_p):
        return True
    good = PB.sa_level(L, src_p, src_x, good_p, off, sd(), loops, (arm,))
    bad = PB.sa_level(L, src_p, src_x, good_p, off, sd(), loops, (arm,), mutant=mutant)
    return PB.ratio(bad.ref, good.ref, good.tol[arm]) > 1.0


# (level, arm) at which every mutant of the table fixture must show: all three levels at the split arm's bound (the default arm; the
# f32 arm's is tighter), level 1 at the plain-f16 arm's too (2^-10 per operand: the deeper levels' f16 bounds are wider than some of
# these faults are large, which is what that arm's precision means). "k31" at level 3 is left out: the fixture's only ball beyond 32
# points there does not have its maximum in the 32nd neighbour, the mutant computes the same numbers.
MUTANT_CASES = [(m, L, "split") for L in (0, 1, 2) for m in PB.MUTANTS if m != "le" and (m, L) != ("k31", 2)]
MUTANT_CASES += [(m, 0, "f16") for m in PB.MUTANTS if m != "le"]


@pytest.mark.parametrize("mutant,L,arm", MUTANT_CASES)
def test_mutants_are_seen_at_their_own_level_on_the_table_fixture(mutant, L, arm):
    pos, rgb, off, lv = table()
    lv = lv[True]
    src = [(pos, rgb), (lv["p1"], lv["x1"]), (lv["p2"], lv["x2"])][L]
    assert level_sees(mutant, L, *src, off, arm=arm)


@functools.lru_cache(maxsize=None)
def geometry():
    pos, rgb, off, info = PB.geometry_fixture()
    return pos, rgb, off, info, PB.reference_levels(pos, rgb, off, sd())


@pytest.mark.parametrize("L,arm", [(0, "split"), (1, "split"), (2, "split"), (0, "f16")])
def test_a_closed_ball_is_seen_at_every_level_on_the_radius_boundary(L, arm):
    """d2 <= r2 instead of <: the probe AT the radius joins centre 0's ball at the level whose radius it sits on"""
    pos, rgb, off, info, lv = geometry()
    src = [(pos, rgb), (lv["p1"], lv["x1"]), (lv["p2"], lv["x2"])][L]
    o = info["boundary"]  # that object alone (a cell of its own): nothing but the probes can make the difference
    assert level_sees("le", L, src[0][o:o + 1], src[1][o:o + 1], np.array([0, 1], np.int32), arm=arm)


def test_no_mutant_is_a_no_op():
    """the controls' control: the unmutated reference against itself is inside (so `level_sees` can say no)"""
    pos, rgb, off, _ = table()
    assert not level_sees(None, 0, pos, rgb, off, arm="f32")


# ---- geometry fixtures: conditions, asserted ----------------------------------------------------------------------------------
def test_radius_boundary_probes():
    pos, rgb, off, info, lv = geometry()
    o = info["boundary"]
    src = [pos[o], lv["p1"][o], lv["p2"][o]]
    for L, r in enumerate(PB.RADII):
        on = np.array([F32(r), 0, 0], dtype=F32)
        under_len = np.nextafter(F32(r), F32(0))
        r2 = F32(F32(r) * F32(r))
        s = src[L]
        assert np.array_equal(s[0], np.zeros(3, F32))  # point 0, the origin, is centre 0 of every level
        i_on = np.flatnonzero((s == on).all(axis=1))
        i_un = np.flatnonzero((np.abs(s).max(axis=1) == under_len) & ((s != 0).sum(axis=1) == 1) & (s[:, 0] == 0))
        assert len(i_on) == 1 and len(i_un) == 1, (L, i_on, i_un)  # both probes survived the sampling down to this level
        d_on, d_un = PB.d2(s[i_on[0]], s[0]), PB.d2(s[i_un[0]], s[0])
        assert d_on == r2 and d_un < r2
        idx, valid = PB.neighbours(s[None], s[None, :1], r)
        nb = set(idx[0, 0][valid[0, 0]].tolist())
        assert i_on[0] not in nb and i_un[0] in nb  # excluded / included, and inside the first 32 of a saturated ball
        assert PB.in_radius(s[None], s[None, :1], r).sum() > 32
        idx, valid = PB.neighbours(s[None], s[None, :1], r, "le")
        assert i_on[0] in set(idx[0, 0][valid[0, 0]].tolist())


def test_saturation_and_chunk_placement():
    pos, rgb, off, info, lv = geometry()
    o = info["saturation"]
    counts = PB.in_radius(pos[o:o + 1], lv["p1"][o:o + 1], 0.2).sum(axis=-1)[0]
    have = set(counts.tolist())
    assert {1, 31, 32, 33} <= have and max(have) >= 64, sorted(have)
    o = info["chunks"]
    inr = PB.in_radius(pos[o:o + 1], lv["p1"][o:o + 1], 0.2)[0]  # [centre, source]
    first, second = inr[:, :64].sum(axis=1), inr[:, 64:128].sum(axis=1)
    assert ((first == 31) & (second > 0) & (first + second > 32)).any()  # the cut falls inside the second chunk
    assert ((inr[:, :192].sum(axis=1) == 0) & (inr[:, 192:].sum(axis=1) > 0)).any()  # a ball that lives in the last chunk only


def test_ties():
    pos, rgb, off, info, lv = geometry()
    assert (pos[info["identical"]] == pos[info["identical"]][0]).all()
    assert np.array_equal(PB.fps(pos[info["identical"]][None])[0], np.zeros(128, np.int64))  # lowest index on every tie
    two = pos[info["two"]]
    assert len(np.unique(two, axis=0)) == 2
    assert PB.fps(two[None])[0].tolist() == [0, 1] + [0] * 126
    assert np.array_equal(PB.fps(pos)[3:5], np.stack([OP.fps(pos[3], 128), OP.fps(pos[4], 128)]))  # as the restatement samples


def test_the_references_sample_as_the_restatement_does():
    pos, rgb, off, lv = table()
    for L, src in enumerate([pos, lv[True]["p1"], lv[True]["p2"]]):
        assert np.array_equal(PB.centres(src), lv[True][f"p{L + 1}"])


def test_magnitude_fixture_margins():
    """every object's largest operand is >= 2 x 3e4 or <= 3e4 / 2 at every stage it reaches unflagged: the expected flags do not
    depend on rounding"""
    pos, rgb, off, msd, expect, first = PB.magnitude_fixture()
    _, op = PB.hold_all(PB.reference_levels(pos, rgb, off, msd), pos, rgb, off, msd, True, "f32")
    for o in range(len(expect)):
        stages = range(4) if first[o] == 0 else range(first[o])
        for s in stages:
            big = op[s, o] >= 2 * PB.WATCH
            assert big or op[s, o] <= PB.WATCH / 2, (o, s, op[s, o])
            assert big == (first[o] == s + 1), (o, s, op[s, o])
    assert expect.tolist() == [int(f > 0) for f in first]


# ---- the dev library's door, without a GPU --------------------------------------------------------------------------------------
def test_the_door_refuses_without_a_launch_and_the_default_library_stays():
    """null context / null pointers are refused with -1 and a message before anything touches the device; a library loaded by path
    is declared like the shipped one, is never cached, and leaves what load_library() hands out alone"""
    from text2loc_amd import engine

    lib = PB.load_blocks()
    nulls = [None] * 9
    assert lib.t2l_blk_pointnet_levels(None, 1, 0, 1, *nulls) == -1 and b"null context" in lib.t2l_blk_last_error()
    assert lib.t2l_blk_pn_fps(None, None, None, 1, 256) == -1 and b"null pointer" in lib.t2l_blk_last_error()
    assert lib.t2l_pointnet_features.argtypes == engine.EXPORTS["t2l_pointnet_features"][1]
    shipped = engine.load_library()
    assert shipped is engine.load_library() and shipped is not lib and PB.load_blocks() is not lib
    assert not hasattr(shipped, "t2l_blk_pointnet_levels")
    with pytest.raises(engine.T2LError, match="missing"):
        engine.load_library(PB.blocks_path() + ".absent")
