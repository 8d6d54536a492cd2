"""GPU tier: the re-rank of merged records under ``search_rerank_form`` = 1 (the default: the merge reduces over the one 16-lane row
that holds a query's records, the twelve early rows travel in one round trip) against = 0 (round 7's form, compiled beside it).
Nothing in the arithmetic differs, so ids, float64 scores and the counters of ``search_counters()`` must be bit-identical between the
arms and repeatable (arms 0, 1, 0, 1 in one process), ids equal to the CPU oracle's and scores within 1e-12 of it.

Shapes: the smallest that reach ``rerank_kernel<8, 16, true, FORM>``. With ``search_auto`` 0 and ``search_merge_lists`` 1 the planner
gives N = 1,100 x Q = 259 the paired scan over 35 tiles in 16 physical splits, i.e. 16 records per query (every lane of the row holds
one), and 8 records under ``search_nsplit`` = 16 (lanes 8..15 of the row hold -inf lists); Q = 259 leaves the last re-rank workgroup
with one dead wave. tests/test_rerank_form_plan.py asserts exactly these plans on the CPU."""
import numpy as np
import pytest

from text2loc_amd import synth

pytestmark = pytest.mark.gpu

N, Q = 1100, 259
# the defaults of the two options the tests move and put back (csrc/search_plan.h: SearchKnobs; tests/rerank_form_plan_check.cpp
# asserts that they still are the defaults)
NSPLIT_DEFAULT, WIDE_REPAIR_DEFAULT = 0, 512


@pytest.fixture(scope="module")
def eng():
    import torch
    from text2loc_amd.engine import Engine

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = Engine(0)
    e.set_option("search_auto", 0)
    e.set_option("search_merge_lists", 1)  # merged records whatever the report cards say
    yield e
    e.close()


def _plane_rows(n):
    """row of plane position p (csrc/search_dev.h: plane_row; one segment): slot j of full tile t holds row j * F + t, F = n // 32."""
    p = np.arange(n)
    full = n // 32
    t, j = p // 32, p % 32
    return np.where(t < full, j * full + t, p)


def _near(rng, v, noise):
    return synth.unit_rows((v.astype(np.float64) + noise * synth.unit_rows(rng.standard_normal((1, 256)))[0])[None])[0]


def _arms(e, db, qs, k, label):
    """arms 0, 1, 0, 1: bit-identical ids, scores and counters, repeatable; the oracle's ids. Returns the counters (of both arms)."""
    import torch
    from oracle import c_oracle

    e.db_set(torch.from_numpy(np.ascontiguousarray(db)).cuda())
    qd = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    got = {}
    try:
        for form in (0, 1, 0, 1):
            e.set_option("search_rerank_form", form)
            idx, sc = e.search(qd, k)
            torch.cuda.synchronize()
            c = e.search_counters()
            if form in got:
                assert torch.equal(idx, got[form][0]) and torch.equal(sc, got[form][1]) and c == got[form][2], (label, form, "not repeatable")
            got[form] = (idx.clone(), sc.clone(), c)
    finally:
        e.set_option("search_rerank_form", 1)
    print(label, "counters:", got[0][2])
    assert torch.equal(got[0][0], got[1][0]), (label, "ids differ between the arms")
    assert torch.equal(got[0][1], got[1][1]), (label, "scores differ between the arms")
    assert got[0][2] == got[1][2], (label, "counters differ between the arms", got[0][2], got[1][2])
    ridx, rsc = c_oracle.retrieve_topk(db, qs, k)
    assert np.array_equal(got[1][0].cpu().numpy().astype(np.int64), ridx), (label, "ids differ from the oracle")
    assert np.abs(got[1][1].cpu().numpy() - rsc).max() < 1e-12, label
    return got[0][2]


def test_option_is_validated(eng):
    with pytest.raises(Exception, match="search_rerank_form"):
        eng.set_option("search_rerank_form", 2)
    eng.set_option("search_rerank_form", 0)
    eng.set_option("search_rerank_form", 1)


@pytest.mark.parametrize("k", [1, 10])
def test_sixteen_records_early_path(eng, k):
    """Unit-Gaussian rows, planted queries: the early certificate settles (nearly) every query."""
    db, qs, _ = synth.make_retrieval_problem(N, Q, seed=81)
    c = _arms(eng, db, qs, k, f"16 records, k={k}")
    assert c["valu_exact_scans"] == 0 and c["rescored"] <= 8, c


def test_eight_records(eng):
    """search_nsplit = 16: 8 physical splits, lanes 8..15 of the record row are empty."""
    db, qs, _ = synth.make_retrieval_problem(N, Q, seed=82)
    eng.set_option("search_nsplit", 16)
    try:
        c = _arms(eng, db, qs, 10, "8 records")
    finally:
        eng.set_option("search_nsplit", NSPLIT_DEFAULT)
    assert c["valu_exact_scans"] == 0 and c["rescored"] <= 8, c


def test_runs_of_sixteen_near_identical_rows(eng):
    """Runs of 16 near-identical rows that are neighbours in the scan's plane (where they meet in one tile, eight of a run in one lane's
    list): records overflow and every certificate fails on a record's bound — the second stage, then the wide repair, which re-scores
    all rows behind the overflowing records (at N = 1,100 a record stands for at most 192 rows, so the default cap of 512 rows holds).
    With the wide repair switched off (``search_wide_repair`` = 0) the same queries go to the exact scan of the shard, where the
    certificate has given up. The parent arm must show each path, so the test cannot pass by never entering them."""
    rng = np.random.default_rng(83)
    base = synth.unit_rows(rng.standard_normal(((N + 15) // 16, 256)))
    tight_plane = synth.unit_rows(3.0 * np.repeat(base, 16, axis=0)[:N] + synth.unit_rows(rng.standard_normal((N, 256)))).astype(np.float32)
    db = np.empty_like(tight_plane)
    db[_plane_rows(N)] = tight_plane
    qs = synth.unit_rows(db[rng.integers(0, N, size=Q)].astype(np.float64) + 0.3 * synth.unit_rows(rng.standard_normal((Q, 256)))).astype(np.float32)
    c = _arms(eng, db, qs, 10, "runs of 16")
    assert c["rescored"] > 0 and c["wide_repairs"] > 0, c
    eng.set_option("search_wide_repair", 0)
    try:
        c = _arms(eng, db, qs, 10, "runs of 16, no wide repair")
    finally:
        eng.set_option("search_wide_repair", WIDE_REPAIR_DEFAULT)
    assert c["rescored"] > 0 and c["valu_exact_scans"] > 0, c


def test_group_repair_and_duplicate_rows(eng):
    """(a) 30 queries have their three best rows in ONE tile-local group (plane slots 0, 1, 2 of a tile: rows t, F + t, 2 F + t): the third
    leaves the scan as the record's B1 by construction, so every planted query fails its first certificate and the re-rank's group
    repair has to re-score B1's group (`rescored` >= 30 by construction; the slack of 4 and "at most 2 wide repairs or exact scans, for a
    second bound in reach" are those of test_gpu_scan_epilogue's planted-triple test).
    (b) 16 bit-identical rows that are every query's best: equal keys across records (lowest part first), ties broken by row."""
    rng = np.random.default_rng(84)
    full = N // 32
    db = synth.unit_rows(rng.standard_normal((N, 256))).astype(np.float32)
    qs = synth.unit_rows(rng.standard_normal((Q, 256))).astype(np.float32)
    planted = 30
    for i, t in enumerate(rng.choice(full, size=planted, replace=False)):
        for j, noise in enumerate((0.35, 0.45, 0.55)):
            db[j * full + t] = _near(rng, qs[i], noise)
    c = _arms(eng, db, qs, 10, "planted triples")
    assert c["rescored"] >= planted - 4 and c["valu_exact_scans"] <= 2 and c["wide_repairs"] <= 2, c
    assert c["rescored"] - c["wide_repairs"] - c["valu_exact_scans"] > 0, c  # repairs settled in the wave: the group repair's path

    db2 = synth.unit_rows(rng.standard_normal((N, 256))).astype(np.float32)
    hot = synth.unit_rows(rng.standard_normal((1, 256)))[0].astype(np.float32)
    db2[rng.choice(N, size=16, replace=False)] = hot
    qs2 = np.stack([_near(rng, hot, 0.5) for _ in range(Q)]).astype(np.float32)
    _arms(eng, db2, qs2, 10, "16 duplicate rows")
    _arms(eng, db2, qs2, 1, "16 duplicate rows, k=1")
