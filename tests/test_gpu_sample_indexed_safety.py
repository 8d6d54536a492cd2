"""GPU tier: t2l_sample_object_points_indexed's rows of the two tiers of DESIGN.md 1a. Guard bands (tests/guards.py, ``run_guarded``
of tests/test_gpu_memory_safety.py): the resident points and offsets between poisoned halos, both outputs carved from patterned
buffers — halos intact, outputs written in full, the bits of the plain run, which meets the numpy restatement where the whole-set
entry point's case does (colours and "fixed" positions bit for bit, 4e-6 otherwise). Call history (tests/test_gpu_call_history.py):
the context's staging buffer (ids | salts) is reused from call to call, so a small call must not see what a larger salted one left."""
import numpy as np
import pytest

from oracle import t2l_oracle_pointnet as OP
from tests.test_gpu_call_history import check_history
from tests.test_gpu_memory_safety import dev, engine, other_than, run_guarded

pytestmark = pytest.mark.gpu

TRANSFORMS = ["fixed", "normalize", "rotate_normalize"]


def problem(n_pts, seed, scale=0.08):
    rs = np.random.default_rng(seed)
    poff = np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int64)
    xyz = (rs.uniform(0.2, 0.8, size=(len(n_pts), 3)).repeat(n_pts, axis=0) + rs.standard_normal((int(poff[-1]), 3)) * scale).astype(np.float32)
    rgb = rs.uniform(0, 1, size=(int(poff[-1]), 3)).astype(np.float32)
    return xyz, rgb, poff


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("salted", [False, True], ids=["salts-null", "salts-mixed"])
@pytest.mark.parametrize("transform", TRANSFORMS)
def test_guard_bands(eng, transform, salted):
    """The first and the last object of the arrays among the rows: the reads that sit next to the halos."""
    xyz, rgb, poff = problem(np.array([8, 25, 300, 4000, 61, 2], dtype=np.int64), 4)
    ids = np.array([5, 0, 3, 3, 5, 2, 0, 1, 4] * 4, dtype=np.int32)[:33]
    salts = (np.arange(33, dtype=np.uint32) % 3) * np.uint32(0x9E3779B1) if salted else None
    plain, _ = run_guarded(lambda a: eng.sample_object_points_indexed(a["xyz"], a["rgb"], a["poff"], ids, salts, seed=77, transform=transform),
                           {"xyz": dev(xyz), "rgb": dev(rgb), "poff": dev(poff)}, 2, ints={"poff": other_than(0, int(poff[-1]), 0, poff[-1])})
    pos, col = plain[0].cpu().numpy(), plain[1].cpu().numpy()
    for salt in np.unique(salts) if salted else [0]:
        rpos, rcol = OP.sample_object_points(xyz, rgb, poff, 77 ^ int(salt), transform=transform)
        sel = salts == salt if salted else slice(None)
        assert np.array_equal(col[sel], rcol[ids[sel]])
        if transform == "fixed":
            assert np.array_equal(pos[sel], rpos[ids[sel]])
        else:
            assert np.abs(pos[sel] - rpos[ids[sel]]).max() < 4e-6


def test_small_calls_after_a_larger_salted_call():
    """D: 512 salted rows of objects whose coordinates are x 1e30 (normalisation overflows: non-finite outputs), which sizes and fills
    the staging buffer. S: 5 rows without salts, then 9 with, under each transform."""
    big = tuple(dev(a) for a in problem(np.array([5000, 3, 700] * 7, dtype=np.int64), 5, scale=1e30))
    small = tuple(dev(a) for a in problem(np.array([8, 25, 300, 4000, 61], dtype=np.int64), 4))
    rs = np.random.default_rng(6)
    big_ids, big_salts = rs.integers(0, 21, size=512).astype(np.int32), rs.integers(0, 2 ** 32, size=512, dtype=np.uint64).astype(np.uint32)

    def S(transform, ids, salts):
        def call(e):
            pos, col = e.sample_object_points_indexed(*small, ids, salts, seed=77, transform=transform)
            return {"pos": pos, "rgb": col}
        return call

    smalls = []
    for t in TRANSFORMS:
        smalls.append(S(t, np.array([4, 0, 3, 3, 1], dtype=np.int32), None))
        smalls.append(S(t, np.array([2, 4, 4, 0, 1, 3, 0, 2, 2], dtype=np.int32), np.arange(9, dtype=np.uint32) * np.uint32(2654435761)))
    check_history(lambda: engine(), lambda e: e.sample_object_points_indexed(*big, big_ids, big_salts, seed=1, transform="rotate_normalize"), smalls)
