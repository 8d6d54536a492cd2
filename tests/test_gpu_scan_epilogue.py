"""GPU tier: the paired scan's short epilogue and XCD-contiguous record layout (option ``search_epilogue`` = 1, the default) against
round 6's form (= 0) — ids and float64 scores bit-identical between the arms, ids equal to the CPU oracle's outright."""
import numpy as np
import pytest

from text2loc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    from text2loc_amd.engine import Engine

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = Engine(0)
    yield e
    e.close()


def _reset(e):
    for name, v in (("search_auto", 1), ("search_merge_lists", 2), ("search_tile_sel", 1), ("search_xcd_qgroups", 4), ("search_epilogue", 1)):
        e.set_option(name, v)


def _arms(e, db, qs, k=10, label="", force_records=True):
    """search under search_epilogue = 0 and = 1 (twice each, alternating: a stale record layout would show): the arms must agree bit for
    bit, and the ids must be the oracle's. Returns the counters of each arm's last call. force_records: merged records whatever the
    report card of the calls before says (the default, search_merge_lists = 2, moves to plain lists — where the option changes nothing —
    after a batch with many failed certificates, and the engine is shared by the module's tests)."""
    import torch
    from oracle import c_oracle

    if force_records:
        e.set_option("search_auto", 0)
        e.set_option("search_merge_lists", 1)
    e.db_set(torch.from_numpy(np.ascontiguousarray(db)).cuda())
    qd = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    got, counters = {}, {}
    for epi in (0, 1, 0, 1):
        e.set_option("search_epilogue", epi)
        idx, sc = e.search(qd, k)
        torch.cuda.synchronize()
        counters[epi] = e.search_counters()
        if epi in got:
            assert torch.equal(idx, got[epi][0]) and torch.equal(sc, got[epi][1]), (label, epi, "not repeatable")
        got[epi] = (idx.clone(), sc.clone())
    print(label, "counters epilogue 0:", counters[0], "epilogue 1:", counters[1])
    assert torch.equal(got[0][0], got[1][0]), (label, "ids differ between the arms")
    assert torch.equal(got[0][1], got[1][1]), (label, "scores differ between the arms")
    ridx, rsc = c_oracle.retrieve_topk(db, qs, k)
    assert np.array_equal(got[1][0].cpu().numpy().astype(np.int64), ridx), (label, "ids differ from the oracle")
    assert np.abs(got[1][1].cpu().numpy() - rsc).max() < 1e-12, label
    return counters


def test_option_is_validated(eng):
    _reset(eng)
    with pytest.raises(Exception, match="search_epilogue"):
        eng.set_option("search_epilogue", 2)
    eng.set_option("search_epilogue", 0)
    eng.set_option("search_epilogue", 1)


def test_bench_shape(eng):
    _reset(eng)
    db, qs, _ = synth.make_retrieval_problem(11259, 4096, seed=0)
    for force in (False, True):  # the engine's defaults, as bench.py runs it; then records forced
        c = _arms(eng, db, qs, label=f"bench shape (records forced: {force})", force_records=force)
        assert c[0]["valu_exact_scans"] == 0 and c[1]["valu_exact_scans"] == 0, c


@pytest.mark.parametrize("n,q", [(11259, 1000), (5003, 1000), (5000, 512), (4097, 300), (1023, 257), (11233, 256)])
def test_ragged_rows_and_queries(eng, n, q):
    """N not a multiple of 32 (the last tile is masked: 11,259, 5,003, 4,097, 1,023; 11,233 leaves ONE valid row in it), Q = 1000 (not a
    multiple of 256), and tile counts that give the second wave of a pair one tile fewer than the first (5,000 / 5,003 rows = 157 tiles
    over 32 virtual splits: splits 29..31 hold 4 tiles, their partners 13..15 hold 5; 1,023 rows = 32 tiles is the even case)."""
    _reset(eng)
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=300 + n, noise=0.7)
    _arms(eng, db, qs, label=f"n={n} q={q}")


@pytest.mark.parametrize("gq", [1, 2, 4, 8])
@pytest.mark.parametrize("n,q", [(11259, 4096), (5003, 1000)])
def test_every_xcd_rectangle(eng, gq, n, q):
    """The record slot is derived from search_xcd_qgroups (1 and 8: the identity; 2: four interleaved residues; 4: two). Q = 1000 is four
    query blocks: the rectangle of 8 does not divide them and the mapping (and with it the layout) falls back to the identity."""
    _reset(eng)
    eng.set_option("search_xcd_qgroups", gq)
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=17 + gq, noise=0.6)
    try:
        _arms(eng, db, qs, label=f"xcd_qgroups={gq} n={n} q={q}")
    finally:
        eng.set_option("search_xcd_qgroups", 4)


@pytest.mark.parametrize("opt,val", [("search_tile_sel", 0), ("search_merge_lists", 0), ("search_merge_lists", 1)])
def test_other_scan_forms(eng, opt, val):
    """Per-score insertion (the layout applies, the short epilogue does not), plain lists (neither applies), forced merged records."""
    _reset(eng)
    eng.set_option("search_auto", 0)
    eng.set_option("search_merge_lists", 1)
    eng.set_option(opt, val)
    try:
        for n, q in ((11259, 2048), (5003, 1000)):
            db, qs, _ = synth.make_retrieval_problem(n, q, seed=9 + n, noise=0.6)
            _arms(eng, db, qs, label=f"{opt}={val} n={n} q={q}", force_records=False)
    finally:
        _reset(eng)


def _near(rng, v, noise):
    return synth.unit_rows((v.astype(np.float64) + noise * synth.unit_rows(rng.standard_normal((1, 256)))[0])[None])[0]


def test_three_best_rows_in_one_group_of_a_waves_last_tile(eng):
    """The drain's new path feeds a B1 the re-rank must repair. N = 11,259 is 352 tiles over 32 virtual splits, 11 tiles each: tiles
    320..350 are the LAST full tile of their wave. 124 queries get their three best rows into ONE tile-local group of such a tile (plane
    slots j, j + 1, j + 2 with j = 0, 4, 16, 20: the four groups of a tile; plane slot j of full tile t is row j * F + t). Under
    search_epilogue = 0 the last tile is inserted score by score and nothing of it is dropped: no repair. Under = 1 the group keeps
    two keys and the third leaves as B1 by construction, so every planted query's certificate fails on B1 and must be settled by the
    in-wave repair (`rescored`), a wide repair or an exact scan: at least 124 repairs in all, by construction. The in-wave repair is the
    one built for this case; as in test_gpu_search's planted-triple test, at most 2 queries may need each of the other two (a second
    bound in reach on random data)."""
    _reset(eng)
    rng = np.random.default_rng(123)
    n, q = 11259, 320
    full = n // 32
    db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    qs = synth.unit_rows(rng.standard_normal((q, 256))).astype(np.float32)
    planted = 0
    for t in range(320, 351):
        for j0 in (0, 4, 16, 20):
            for d, noise in enumerate((0.35, 0.45, 0.55)):
                db[(j0 + d) * full + t] = _near(rng, qs[planted], noise)
            planted += 1
    assert planted == 124
    c = _arms(eng, db, qs, label="last-tile triples")
    assert c[0]["rescored"] <= 8 and c[0]["valu_exact_scans"] == 0, c
    assert c[1]["valu_exact_scans"] <= 2 and c[1]["wide_repairs"] <= 2, c
    assert c[1]["rescored"] >= planted - 4, c


def test_sixteen_duplicate_rows(eng):
    """16 bit-identical rows that are every query's best (ties: lower row first), at random places and — second database — in the last
    tiles of the plane, masked tile included."""
    _reset(eng)
    rng = np.random.default_rng(5)
    n, q = 11259, 512
    db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    hot = synth.unit_rows(rng.standard_normal((1, 256)))[0].astype(np.float32)
    qs = np.stack([_near(rng, hot, 0.5) for _ in range(q)]).astype(np.float32)
    db1 = db.copy()
    db1[rng.choice(n, size=16, replace=False)] = hot
    _arms(eng, db1, qs, label="16 duplicates, scattered")
    db2 = db.copy()
    db2[n - 16:] = hot  # rows 11,243..11,258: all in the masked last tile (plane positions = rows there)
    _arms(eng, db2, qs, label="16 duplicates, last rows")


@pytest.mark.parametrize("n", [11259, 5003, 11233])
def test_best_rows_are_the_last_valid_rows(eng, n):
    """Every query's best rows are the last valid rows before n_rows: they sit in the masked tile, next to rows the drain must turn
    into -inf before they become keys (a masked row that leaked would out-rank nothing — the plane's tail is zero — but a valid row
    masked by mistake is a wrong id here). The three best sit in ONE tile-local group (11,259: plane slots 24..26 of the masked tile; 5,003:
    slots 8..10), so under search_epilogue = 1 each of the 200 planted queries needs a repair, as in the test above; 11,233 has one row there."""
    _reset(eng)
    rng = np.random.default_rng(n)
    q = 300
    db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    qs = synth.unit_rows(rng.standard_normal((q, 256))).astype(np.float32)
    hot = synth.unit_rows(rng.standard_normal((1, 256)))[0].astype(np.float32)
    qs[:200] = np.stack([_near(rng, hot, 0.4) for _ in range(200)])
    last = min(5, n % 32)
    for d in range(last):
        db[n - 1 - d] = _near(rng, hot, 0.2 + 0.05 * d)
    c = _arms(eng, db, qs, label=f"best rows last, n={n}")
    assert c[0]["rescored"] <= 8 and c[0]["valu_exact_scans"] == 0, c
    if last >= 3:
        assert c[1]["valu_exact_scans"] <= 2 and c[1]["wide_repairs"] <= 2, c
        assert c[1]["rescored"] >= 200 - 4, c
