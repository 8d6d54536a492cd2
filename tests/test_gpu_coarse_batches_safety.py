"""GPU tier: the rows of t2l_sample_object_points_mirrored and t2l_gather_object_rows in the two tiers of DESIGN.md 1a. Guard bands
(tests/guards.py, ``run_guarded`` of tests/test_gpu_memory_safety.py): every resident array between poisoned halos, every output carved
from a patterned buffer — halos intact, outputs written in full, the bits of the plain run, which equals the restatement
(tests/coarse_batch_ref.py). Call history (tests/test_gpu_call_history.py): both entry points stage ids | salts | mirror through the
context's one pinned buffer, so a small call must not see what a larger one left there."""
import numpy as np
import pytest

from tests import coarse_batch_ref as R
from tests.test_gpu_call_history import check_history
from tests.test_gpu_memory_safety import dev, engine, other_than, run_guarded
from tests.test_gpu_sample_indexed_safety import TRANSFORMS, problem

pytestmark = pytest.mark.gpu

TABLE_KEYS = ("class_idx", "color_idx", "rgb", "center", "n_pts")


def table(n, seed):
    rs = np.random.default_rng(seed)
    return {"class_idx": rs.integers(0, 22, size=n).astype(np.int32), "color_idx": rs.integers(0, 8, size=n).astype(np.int32),
            "rgb": rs.uniform(0, 1, size=(n, 3)).astype(np.float32), "center": rs.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32),
            "n_pts": rs.integers(1, 60000, size=n).astype(np.float32)}


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("salted", [False, True], ids=["salts-null", "salts-mixed"])
@pytest.mark.parametrize("transform", TRANSFORMS)
def test_mirrored_sampler_guard_bands(eng, transform, salted):
    """The first and the last object of the arrays among the rows, under every code: the reads that sit next to the halos."""
    xyz, rgb, poff = problem(np.array([8, 25, 300, 4000, 61, 2], dtype=np.int64), 4)
    ids = np.array([5, 0, 3, 3, 5, 2, 0, 1, 4] * 4, dtype=np.int32)[:33]
    mirror = ((np.arange(33) // 2) % 4).astype(np.uint8)
    salts = (np.arange(33, dtype=np.uint32) % 3) * np.uint32(0x9E3779B1) if salted else None
    plain, _ = run_guarded(lambda a: eng.sample_object_points_mirrored(a["xyz"], a["rgb"], a["poff"], ids, salts, mirror, seed=77, transform=transform),
                           {"xyz": dev(xyz), "rgb": dev(rgb), "poff": dev(poff)}, 2, ints={"poff": other_than(0, int(poff[-1]), 0, poff[-1])})
    rpos, rcol = R.sample_rows(xyz, rgb, poff, ids, salts, mirror, 77, transform)
    assert R.diff_count(plain[0].cpu().numpy(), rpos) == 0 and R.diff_count(plain[1].cpu().numpy(), rcol) == 0


@pytest.mark.parametrize("mirrored", [False, True], ids=["mirror-null", "mirror-mixed"])
def test_gather_guard_bands(eng, mirrored):
    """Rows 0 and n - 1 of the tables among the ids; integer halos hold an in-range class / colour row that differs from both ends."""
    t = table(9, 3)
    ids = np.array([8, 0, 3, 3, 8, 2, 0, 1, 4, 7, 6, 5] * 3, dtype=np.int32)[:33]
    mirror = ((np.arange(33) // 2) % 4).astype(np.uint8) if mirrored else None
    ints = {k: other_than(0, 7, t[k][0], t[k][-1]) for k in ("class_idx", "color_idx")}

    def call(a):
        out = eng.gather_object_rows(a, ids, mirror)
        return tuple(out[k] for k in TABLE_KEYS)

    plain, _ = run_guarded(call, {k: dev(t[k]) for k in TABLE_KEYS}, 5, ints=ints)
    for got, (k, ref) in zip(plain, R.gather_rows(t, ids, mirror).items()):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), k


def test_small_calls_after_larger_salted_and_mirrored_calls():
    """D: 1,500 salted and mirrored rows of objects whose coordinates are x 1e30, then 3,000 more: ids | salts take a word per row and
    mirror a byte, so the first fills 3,375 words of the 4,096-word buffer a context starts with and the second (6,750 words) makes it
    regrow; a 1,500-row gather follows. S: 2-row calls of both entry points, with and without salts and codes — the bits of a fresh
    context, before and after the buffer has been replaced."""
    big = tuple(dev(a) for a in problem(np.array([5000, 3, 700] * 7, dtype=np.int64), 5, scale=1e30))
    small = tuple(dev(a) for a in problem(np.array([8, 25, 300, 4000, 61], dtype=np.int64), 4))
    big_t, small_t = {k: dev(v) for k, v in table(21, 7).items()}, {k: dev(v) for k, v in table(5, 8).items()}
    rs = np.random.default_rng(6)
    big_ids, big_salts = rs.integers(0, 21, size=3000).astype(np.int32), rs.integers(0, 2 ** 32, size=3000, dtype=np.uint64).astype(np.uint32)
    big_mirror = rs.integers(0, 4, size=3000).astype(np.uint8)

    def D(e):
        e.sample_object_points_mirrored(*big, big_ids[:1500], big_salts[:1500], big_mirror[:1500], seed=1, transform="rotate_normalize")
        e.sample_object_points_mirrored(*big, big_ids, big_salts, big_mirror, seed=1, transform="rotate_normalize")
        e.gather_object_rows(big_t, big_ids[:1500], big_mirror[:1500])

    def S(transform, ids, salts, mirror):
        def call(e):
            pos, col = e.sample_object_points_mirrored(*small, ids, salts, mirror, seed=77, transform=transform)
            return {"pos": pos, "rgb": col}
        return call

    def Sg(ids, mirror):
        return lambda e: dict(e.gather_object_rows(small_t, ids, mirror))

    two = np.array([4, 0], dtype=np.int32)
    smalls = [Sg(two, None), Sg(two, np.array([3, 1], dtype=np.uint8))]
    for t in TRANSFORMS:
        smalls.append(S(t, two, None, None))
        smalls.append(S(t, two, np.array([7, 2654435761], dtype=np.uint32), np.array([2, 1], dtype=np.uint8)))
    check_history(lambda: engine(), D, smalls)
