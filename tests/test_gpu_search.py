"""GPU tier: the fused HIP search (through the C ABI) against the CPU oracle — integer-exact row ids."""
import numpy as np
import pytest

from oracle import t2l_oracle as O
from text2loc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 2], ids=["f16", "bf16x3"])
def eng(request):
    """Both scan arithmetics (the f16 scan and the split-bf16 scan the auto mode escalates to) feed the same float64 re-rank +
    certificate: every test runs against each. (A third, exact-f32 scan existed until round 5: 7x slower, same results by
    construction; removed.)"""
    import torch
    from text2loc_amd.engine import Engine

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = Engine(0)
    e.set_option("search_mode", request.param)
    e.scan_mode = request.param
    yield e
    e.close()


def _search(eng, db, q, k, row_offset=0):
    import torch

    eng.db_set(torch.from_numpy(np.ascontiguousarray(db)).cuda(), row_offset)
    idx, sc = eng.search(torch.from_numpy(np.ascontiguousarray(q)).cuda(), k)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), sc.cpu().numpy()


def test_golden_retrieval_big(eng, golden):
    g = golden("retrieval_big")
    db, q, _ = synth.make_retrieval_problem(int(g["n_cells"]), int(g["n_queries"]), seed=int(g["seed"]),
                                            noise=float(g["noise"]))
    idx, sc = _search(eng, db, q, int(g["k"]))
    assert np.array_equal(idx, g["top_rows"])  # integer-exact vs the reference's own loop
    assert np.abs(sc - g["top_scores"]).max() < 1e-12
    assert eng.search_fallbacks() == 0


def test_golden_e2e_ids(eng, golden):
    g = golden("retrieval_e2e")
    k = int(g["top_k"].max())
    idx, sc = _search(eng, g["cell_encodings"], g["text_encodings"], k)
    assert np.array_equal(idx, g["top_rows"])
    assert np.abs(sc - g["top_scores"]).max() < 1e-12


@pytest.mark.parametrize("n,q,k", [(1, 1, 1), (5, 3, 10), (31, 7, 5), (32, 128, 10), (33, 129, 10), (1000, 257, 26),
                                   (4097, 64, 16), (11259, 300, 10),
                                   # the smallest shape of each scan instance (csrc/search_plan.h: ScanKernel): one wave per SIMD with
                                   # lists of 16 and of 8, the smallest paired launch (32 tiles at 256 queries) and one tile short of it
                                   (33, 17, 10), (11259, 255, 10), (993, 256, 10), (992, 256, 10)])
def test_ragged_shapes_vs_oracle(eng, n, q, k):
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=100 + n, noise=2.0)
    idx, sc = _search(eng, db, qs, k)
    ridx, rsc = O.retrieve_topk(db, qs, k)
    kk = ridx.shape[1]
    assert np.array_equal(idx[:, :kk], ridx)
    assert np.abs(sc[:, :kk] - rsc).max() < 1e-12
    if kk < k:  # K > N: the tail is -1 / -inf
        assert (idx[:, kk:] == -1).all() and np.isneginf(sc[:, kk:]).all()


def test_exact_ties_lower_row_first(eng):
    rng = np.random.default_rng(7)
    base = synth.unit_rows(rng.standard_normal((40, 256))).astype(np.float32)
    db = np.concatenate([base, base, base[:13]], axis=0)  # every row duplicated (some tripled)
    q = synth.unit_rows(rng.standard_normal((50, 256))).astype(np.float32)
    idx, sc = _search(eng, db, q, 10)
    from oracle import c_oracle  # sequential float64 sums: identical rows give bit-identical scores (BLAS may not)
    ridx, rsc = c_oracle.retrieve_topk(db, q, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12


def test_forced_fallback_matches(eng):
    db, qs, _ = synth.make_retrieval_problem(3000, 40, seed=5, noise=2.0)
    ridx, rsc = O.retrieve_topk(db, qs, 10)
    eng.set_option("certify_eps_scale", 1e9)  # every certificate fails -> exact float64 scan kernel
    try:
        idx, sc = _search(eng, db, qs, 10)
        assert eng.search_fallbacks() == 40
    finally:
        eng.set_option("certify_eps_scale", 1.0)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12


def test_near_ties_are_certified_or_fall_back(eng):
    # rows that differ by ~1e-7 in score: f32 cannot order them; the certificate must catch it
    rng = np.random.default_rng(11)
    q = synth.unit_rows(rng.standard_normal((8, 256))).astype(np.float32)
    base = synth.unit_rows(rng.standard_normal((1, 256)))
    db = (base + 1e-7 * rng.standard_normal((600, 256))).astype(np.float32)
    idx, sc = _search(eng, db, q, 10)
    ridx, rsc = O.retrieve_topk(db, q, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12


@pytest.mark.parametrize("db_scale,q_scale", [(1.0, 1.0), (3.0e-6, 1.0), (1.0, 7.0e4), (2.5e5, 1.0e-7), (1.0e-20, 1.0e20)])
def test_scale_invariance(eng, db_scale, q_scale):
    """The f16 scan rescales DB and queries by exact powers of two: ids must not depend on the magnitudes handed in."""
    db, qs, _ = synth.make_retrieval_problem(3000, 200, seed=13, noise=2.0)
    db = (db * np.float32(db_scale)).astype(np.float32)
    qs = (qs * np.float32(q_scale)).astype(np.float32)
    qs[5] *= np.float32(1e-3)  # per-query scales differ inside a batch
    qs[6] *= np.float32(1e3)
    db[17] *= np.float32(1e-4)  # a row far below the largest one
    idx, sc = _search(eng, db, qs, 10)
    ridx, rsc = O.retrieve_topk(db, qs, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() <= 1e-12 * max(1.0, float(np.abs(rsc).max()))
    if eng.scan_mode == 0 or max(abs(np.log10(db_scale)), abs(np.log10(q_scale))) < 11:
        assert eng.search_fallbacks() == 0  # representable: nobody needed the exact scan
    else:  # the split-bf16 scan multiplies the raw values and hand magnitudes beyond 2^+-40 to the exact scan
        assert eng.search_fallbacks() == len(qs)


def test_unrepresentable_inputs_take_the_exact_scan(eng):
    """Zero / denormal-sized queries (and a denormal-sized DB) have no f16 image: those queries are scanned exactly."""
    db, qs, _ = synth.make_retrieval_problem(700, 12, seed=14, noise=2.0)
    qs[3] = 0.0
    qs[4] = (qs[4] * np.float32(1e-30)).astype(np.float32) * np.float32(1e-12)  # denormal magnitudes
    idx, sc = _search(eng, db, qs, 10)
    ridx, rsc = O.retrieve_topk(db, qs, 10)
    keep = np.array([i for i in range(12) if i != 3])  # the zero query ties everywhere: compare it separately
    assert np.array_equal(idx[keep], ridx[keep])
    assert np.array_equal(idx[3], np.arange(10))  # all scores 0: (score desc, row asc)
    assert np.abs(sc - rsc).max() < 1e-12
    tiny = (db * np.float32(1e-30)).astype(np.float32) * np.float32(1e-14)  # every element denormal or zero
    idx, _ = _search(eng, tiny, qs[:3], 10)
    ridx, _ = O.retrieve_topk(tiny, qs[:3], 10)
    from oracle import c_oracle
    ridx, _ = c_oracle.retrieve_topk(tiny, qs[:3], 10)
    assert np.array_equal(idx, ridx)


def test_narrower_embeddings_are_zero_padded(eng):
    """``--coarse_embed_dim 128`` (models/cell_retrieval.py:22-49): the search takes rows narrower than its compiled 256 by zero padding —
    ids and float64 scores are those of the narrow rows (the reference's loop on the same arrays)."""
    rng = np.random.default_rng(128)
    for d in (128, 64, 200):
        db = synth.unit_rows(rng.standard_normal((3000, d))).astype(np.float32)
        q = synth.unit_rows(db[rng.integers(0, 3000, 300)].astype(np.float64) + 0.5 * synth.unit_rows(rng.standard_normal((300, d)))).astype(np.float32)
        idx, sc = _search(eng, db, q, 10)
        ridx, rsc = O.retrieve_topk(db, q, 10)
        assert np.array_equal(idx, ridx), d
        assert np.abs(sc - rsc).max() < 1e-12
    import torch

    with pytest.raises(Exception, match="D <= 256"):
        eng.db_set(torch.zeros(10, 300).cuda())


def test_clustered_scores_use_the_second_stage(eng):
    """Scores packed ~1e-4 apart: more rows than the re-rank re-scores sit inside the scan's error band, so the
    certificate fails and the targeted float64 re-score (or the full one) decides — exactly."""
    rng = np.random.default_rng(23)
    q = synth.unit_rows(rng.standard_normal((40, 256))).astype(np.float32)
    base = synth.unit_rows(rng.standard_normal((1, 256)))
    db = synth.unit_rows(base + 2e-4 * rng.standard_normal((2000, 256))).astype(np.float32)
    db[::7] = synth.unit_rows(rng.standard_normal((len(db[::7]), 256))).astype(np.float32)  # and unrelated rows between
    idx, sc = _search(eng, db, q, 10)
    ridx, rsc = O.retrieve_topk(db, q, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12
    assert eng.search_rescored() >= eng.search_fallbacks()


@pytest.mark.parametrize("alpha,n,clusters", [(5.0, 11259, 64), (4.0, 6000, 24), (6.0, 2500, 40)])
def test_tight_clusters_are_settled_by_the_wide_repair(eng, alpha, n, clusters):
    """DB = normalize(alpha * centroid + unit noise): the top-k of a query all lie in one cluster, a few dozen to a few hundred
    keys reach the threshold and some full lists dropped rows that could. The re-rank wave re-scores exactly those (kept keys of
    the good lists + every row of the bad ones, rerank_kernel's wide repair) instead of sending the query to a float64 scan of
    the whole shard: ids equal the oracle, and (default scan) the wide repair — not the exact scan — served them."""
    from oracle import c_oracle

    rng = np.random.default_rng(int(alpha * 10) + n)
    cent = synth.unit_rows(rng.standard_normal((clusters, 256)))
    member = rng.integers(0, clusters, size=n)
    db = synth.unit_rows(alpha * cent[member] + synth.unit_rows(rng.standard_normal((n, 256)))).astype(np.float32)
    tgt = rng.integers(0, n, size=600)
    spread = 1.0 / np.sqrt(1.0 + alpha * alpha)
    q = synth.unit_rows(db[tgt].astype(np.float64) + 0.25 * spread * synth.unit_rows(rng.standard_normal((600, 256)))).astype(np.float32)
    eng.set_option("search_auto", 0)  # stay on this engine's scan: the test is about the re-rank's repair
    import torch

    ridx, rsc = c_oracle.retrieve_topk(db, q, 10)
    cnts = []
    for call in range(3):  # (the first calls run on merged records — a repair behind one re-scores 4x the rows and the cap sends more of
        idx, sc = _search(eng, db, q, 10) if call == 0 else tuple(t.cpu().numpy() for t in eng.search(torch.from_numpy(q).cuda(), 10))
        cnts.append(eng.search_counters())  # them to exact scans — until the report card of the first call moves the engine to plain lists)
        assert np.array_equal(idx, ridx), call
        assert np.abs(sc - rsc).max() < 1e-12
    eng.set_option("search_auto", 1)
    if eng.scan_mode == 0:
        assert cnts[0]["wide_repairs"] > 0, cnts
        assert cnts[0]["valu_exact_scans"] <= cnts[0]["wide_repairs"], cnts
        assert cnts[-1]["wide_repairs"] > 0 and cnts[-1]["valu_exact_scans"] <= cnts[-1]["wide_repairs"] // 4, cnts


def test_auto_mode_leaves_the_f16_scan_on_packed_scores_and_returns(eng):
    """Scores packed ~1e-4 apart: the f16 error band cannot separate anything, every query is flagged; the engine
    reads that count back (no synchronisation of its own) and serves the next batches with the split-bf16 scan, then goes
    back to the f16 scan once ordinary data would certify again. Results are exact throughout."""
    import torch

    if eng.scan_mode != 0:
        pytest.skip("auto mode belongs to the default scan")
    eng.set_option("search_auto", 0)  # forget what earlier tests on this engine left behind
    eng.set_option("search_auto", 1)
    rng = np.random.default_rng(29)
    q = synth.unit_rows(rng.standard_normal((64, 256))).astype(np.float32)
    base = synth.unit_rows(rng.standard_normal((1, 256)))
    packed = synth.unit_rows(base + 1e-3 * rng.standard_normal((3000, 256))).astype(np.float32)
    ridx, rsc = O.retrieve_topk(packed, q, 10)

    def again(qq):  # (the database stays resident: t2l_db_set voids the report cards, a new database starts on the f16 scan)
        i, s = eng.search(torch.from_numpy(np.ascontiguousarray(qq)).cuda(), 10)
        torch.cuda.synchronize()
        return i.cpu().numpy().astype(np.int64), s.cpu().numpy()

    # t2l_db_set's prior (round 5): rows this parallel (mean pairwise cosine > 0.9 over a sample) start on the stand-in scan at once
    idx, sc = _search(eng, packed, q, 10)
    assert np.array_equal(idx, ridx) and np.abs(sc - rsc).max() < 1e-12
    assert eng.search_counters()["probe"] > len(q) // 8 and eng.search_fallbacks() == 0
    # ... and WITHOUT the prior (forgotten: the report-card mechanism by itself, from the f16 scan)
    eng.set_option("search_auto", 0)
    eng.set_option("search_auto", 1)
    idx, sc = again(q)
    assert np.array_equal(idx, ridx) and np.abs(sc - rsc).max() < 1e-12
    first = eng.search_rescored()
    assert first > len(q) // 8
    # the report card of a call is published by the NEXT call's re-rank (no extra launch, no synchronisation), so the
    # stand-in scan takes over from the third call on: its certificate holds
    for _ in range(3):
        idx, sc = again(q)
        assert np.array_equal(idx, ridx) and np.abs(sc - rsc).max() < 1e-12
    assert eng.search_rescored() < first
    assert eng.search_counters()["probe"] > len(q) // 8  # the stand-in is counting what the f16 band would still flag
    # friendly QUERIES against the same rows (far from the packed direction's fine structure? no: any query sees packed scores here),
    # so release is exercised on a friendly database below; a new database starts on the f16 scan at once
    db, qs, _ = synth.make_retrieval_problem(3000, 64, seed=31, noise=2.0)
    r2, _ = O.retrieve_topk(db, qs, 10)
    idx, _ = _search(eng, db, qs, 10)
    assert np.array_equal(idx, r2)
    assert eng.search_counters()["probe"] == 0  # t2l_db_set voided the old database's report cards and the new rows are not parallel: the f16 scan is back
    for _ in range(3):
        idx, _ = again(qs)
        assert np.array_equal(idx, r2)
    assert eng.search_fallbacks() == 0


def test_randomized_shapes_and_data_kinds(eng):
    """24 random (N, Q, K, row offset) draws over plain / tightly clustered / rescaled / duplicated data: ids equal the oracle
    (swaps only between float64-equal scores, where BLAS and the kernel may sum in different orders), scores to 1e-12."""
    from oracle import c_oracle

    rng = np.random.default_rng(2024 + eng.scan_mode)
    for _ in range(24):
        n = int(rng.choice([1, 7, 31, 32, 33, 100, 257, 511, 1000, 2049, 5000, 11259]))
        q = int(rng.choice([1, 2, 31, 64, 65, 255, 256, 257, 700]))
        k = int(rng.choice([1, 3, 5, 10, 11, 26]))
        kind = int(rng.integers(0, 4))
        db, qs, _ = synth.make_retrieval_problem(n, q, seed=int(rng.integers(1 << 30)), noise=float(rng.choice([0.1, 0.5, 2.0])))
        if kind == 1:
            base = synth.unit_rows(rng.standard_normal((1, 256)))
            db = synth.unit_rows(base + 10 ** rng.uniform(-4, -2) * rng.standard_normal((n, 256))).astype(np.float32)
        elif kind == 2:
            db = (db * np.float32(10 ** rng.uniform(-8, 8))).astype(np.float32)
            qs = (qs * np.float32(10 ** rng.uniform(-8, 8))).astype(np.float32)
        elif kind == 3 and n > 40:
            db[n // 2:n // 2 + min(20, n // 4)] = db[:min(20, n // 4)]
        off = int(rng.integers(0, 1000))
        idx, sc = _search(eng, db, qs, k, row_offset=off)
        ridx, rsc = (c_oracle if kind == 3 else O).retrieve_topk(db, qs, k)
        kk = ridx.shape[1]
        scale = max(1.0, float(np.abs(rsc).max()))
        assert np.abs(sc[:, :kk] - rsc).max() <= 1e-12 * scale, (n, q, k, kind)
        for a, b in np.argwhere(idx[:, :kk] != ridx + off):
            assert abs(sc[a, b] - rsc[a, b]) <= 1e-13 * scale, (n, q, k, kind)


@pytest.mark.parametrize("nsplit", [1, 3, 8, 32])
def test_nsplit_invariance(eng, nsplit):
    db, qs, _ = synth.make_retrieval_problem(2500, 130, seed=9, noise=2.0)
    ridx, _ = O.retrieve_topk(db, qs, 10)
    eng.set_option("search_nsplit", nsplit)
    try:
        idx, _ = _search(eng, db, qs, 10)
    finally:
        eng.set_option("search_nsplit", 0)
    assert np.array_equal(idx, ridx)


def test_row_offset_and_logical_shards_merge(eng):
    """8 logical shards on one GPU: per-shard top-k then the merge == unsharded result."""
    from text2loc_amd.sharded import merge_topk, shard_bounds

    db, qs, _ = synth.make_retrieval_problem(3001, 96, seed=3, noise=2.0)
    ridx, rsc = O.retrieve_topk(db, qs, 10)
    parts_i, parts_s = [], []
    for r in range(8):
        lo, hi = shard_bounds(len(db), 8, r)
        i, s = _search(eng, db[lo:hi], qs, 10, row_offset=lo)
        parts_i.append(i)
        parts_s.append(s)
    idx, sc = merge_topk(np.stack(parts_i), np.stack(parts_s), 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12


def test_full_size_properties(eng):
    """BASELINE config 2 size (N=11,259, Q=4,096): planted positives are retrieved, scores are sorted,
    ids unique and in range, and EVERY one of the 4,096 x 10 (id, score) pairs equals the float64 C oracle."""
    from oracle import c_oracle

    db, qs, target = synth.make_retrieval_problem(11259, 4096, seed=1, noise=0.5)
    idx, sc = _search(eng, db, qs, 10)
    assert (idx[:, 0] == target).all()
    assert (np.diff(sc, axis=1) <= 0).all()
    assert ((idx >= 0) & (idx < 11259)).all()
    assert all(len(set(r)) == 10 for r in idx[::64])
    ridx, rsc = c_oracle.retrieve_topk(db, qs, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12


def test_shard_of_two_scan_segments(eng):
    """A shard beyond one scan launch's 524,288 rows is searched segment by segment and merged; the f16 plane deals rows to tiles strided
    INSIDE each segment (plane_row: the second segment here has 156 full tiles and a partial one). Batched (paired scan) and streaming
    (few queries) paths against the float64 ranking."""
    rng = np.random.default_rng(19)
    n = 524_288 + 5_000
    db = rng.standard_normal((n, 256)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    tgt = np.concatenate([rng.integers(0, n, 200), rng.integers(524_288, n, 56)])  # (some answers in the short second segment)
    q = db[tgt].astype(np.float64) + 0.6 * rng.standard_normal((256, 256)) / 16.0
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    s = q.astype(np.float64) @ db.astype(np.float64).T
    ridx = np.argsort(-s, axis=1, kind="stable")[:, :10]
    rsc = np.take_along_axis(s, ridx, axis=1)
    idx, sc = _search(eng, db, q, 10)
    assert np.array_equal(idx, ridx)
    assert np.abs(sc - rsc).max() < 1e-12
    idx, sc = _search(eng, db, q[:8], 10)  # the streaming scan walks the whole plane in one launch
    assert np.array_equal(idx, ridx[:8])
    assert (ridx[200:, 0] >= 524_288).all()


def test_hip_merge_kernel_vs_host_merge(eng):
    import torch
    from text2loc_amd.sharded import merge_topk_host

    rng = np.random.default_rng(21)
    P, Q, K = 8, 77, 10
    idx = np.stack([np.sort(np.stack([rng.permutation(1000)[:K] for _ in range(Q)]) + 1000 * p, axis=1)
                    for p in range(P)]).astype(np.int32)  # unique row ids, as shards are disjoint
    sc = -np.sort(-rng.standard_normal((P, Q, K)), axis=2)
    sc[3, :, 5:] = sc[3, :, 4:5]  # ties inside a shard
    idx[5, :, 7:] = -1            # short shard
    sc[5, :, 7:] = -np.inf
    gi, gs = eng.merge_topk(torch.from_numpy(idx).cuda(), torch.from_numpy(sc).cuda())
    torch.cuda.synchronize()
    hi, hs = merge_topk_host(idx, sc, K)
    assert np.array_equal(gi.cpu().numpy().astype(np.int64), hi)
    assert np.array_equal(gs.cpu().numpy(), hs)
    # the packed single-collective form: pack per shard, stack (= all_gather), merge
    pairs = torch.stack([eng.pack_pairs(torch.from_numpy(idx[p]).cuda(), torch.from_numpy(sc[p]).cuda()) for p in range(P)])
    pi, ps = eng.merge_pairs(pairs)
    assert np.array_equal(pi.cpu().numpy().astype(np.int64), hi)
    assert np.array_equal(ps.cpu().numpy(), hs)
    # the block form (no pack launch): every rank's {ids | scores} block back to back, as t2l_search fills and all_gather delivers
    buf, _, _, bb, so = eng.result_block(Q, K, "cuda", parts=P)
    for p_ in range(P):
        buf[p_, :Q * K * 4].view(torch.int32).view(Q, K).copy_(torch.from_numpy(idx[p_]))
        buf[p_, so:so + Q * K * 8].view(torch.float64).view(Q, K).copy_(torch.from_numpy(sc[p_]))
    bi, bs = eng.merge_gathered(buf.view(-1), bb, so, P, Q, K)
    assert np.array_equal(bi.cpu().numpy().astype(np.int64), hi) and np.array_equal(bs.cpu().numpy(), hs)
    # wider lists than one lane per candidate (26 x 9 = 234 candidates), odd query counts, K = 1
    for P2, Q2, K2 in ((9, 5, 26), (2, 131, 1), (25, 3, 10)):
        idx2 = np.stack([np.stack([rng.permutation(5000)[:K2] for _ in range(Q2)]) + 5000 * p_ for p_ in range(P2)]).astype(np.int32)
        sc2 = -np.sort(-rng.standard_normal((P2, Q2, K2)), axis=2)
        g2i, g2s = eng.merge_topk(torch.from_numpy(idx2).cuda(), torch.from_numpy(sc2).cuda())
        h2i, h2s = merge_topk_host(idx2, sc2, K2)
        assert np.array_equal(g2i.cpu().numpy().astype(np.int64), h2i) and np.array_equal(g2s.cpu().numpy(), h2s)


@pytest.mark.parametrize("n,q,k", [(1, 1, 1), (33, 5, 10), (1000, 64, 10), (4097, 17, 26), (70001, 33, 10)])
def test_streaming_small_batch_path_vs_oracle(n, q, k):
    """The HBM-streaming scan for small query batches (forced on for small shards too): same contract."""
    import torch
    from text2loc_amd.engine import Engine

    e = Engine(0)
    e.set_option("stream_min_rows", 1)
    try:
        db, qs, _ = synth.make_retrieval_problem(n, q, seed=300 + n, noise=2.0)
        e.db_set(torch.from_numpy(db).cuda(), 7)
        idx, sc = e.search(torch.from_numpy(qs).cuda(), k)
        torch.cuda.synchronize()
        idx, sc = idx.cpu().numpy().astype(np.int64), sc.cpu().numpy()
        ridx, rsc = O.retrieve_topk(db, qs, k)
        kk = ridx.shape[1]
        assert np.array_equal(idx[:, :kk], ridx + 7)
        assert np.abs(sc[:, :kk] - rsc).max() < 1e-12
        if kk < k:
            assert (idx[:, kk:] == -1).all() and np.isneginf(sc[:, kk:]).all()
        # duplicated rows: exact ties -> lower row first, through the fallback if the certificate cannot decide
        db2 = np.concatenate([db[: min(n, 50)], db[: min(n, 50)]], axis=0)
        e.db_set(torch.from_numpy(db2).cuda(), 0)
        idx2, _ = e.search(torch.from_numpy(qs).cuda(), min(k, 10))
        from oracle import c_oracle  # sequential float64 sums: identical rows give identical scores (BLAS may not)
        r2, _ = c_oracle.retrieve_topk(db2, qs, min(k, 10))
        assert np.array_equal(idx2.cpu().numpy().astype(np.int64)[:, : r2.shape[1]], r2)
    finally:
        e.close()


@pytest.mark.parametrize("n,q,k", [(1, 1, 1), (5, 3, 10), (31, 1, 26), (257, 4, 10), (700, 5, 10), (4097, 16, 26), (11259, 1, 10), (11259, 2, 10),
                                   (11259, 13, 5), (65535, 1, 10), (60001, 7, 3)])
def test_one_launch_exact_search_for_a_handful_of_queries(n, q, k):
    """Q <= 16 against <= 65,536 rows (search_small.hip): ONE launch, float64 scores of every row, per-workgroup top-k published
    write-through, merged by the last workgroup to arrive. Ids equal the oracle's float64 ranking, scores to 1e-12 — and they are
    BIT-identical to what the batched two-launch path (option search_small = 0) reports for the same rows; exact ties go to the
    lower row; a shard offset is applied; K > N leaves -1 / -inf; repeated calls with other query counts reuse the ticket counters."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    e = Engine(0)
    try:
        e.set_option("profile_events", 1)
        db, qs, _ = synth.make_retrieval_problem(n, q, seed=900 + n + q, noise=1.5)
        e.db_set(torch.from_numpy(db).cuda(), 11)
        dq = torch.from_numpy(qs).cuda()
        e.kernel_stats("search_small")
        idx, sc = e.search(dq, k)
        torch.cuda.synchronize()
        assert e.kernel_stats("search_small")[1] == 1 and e.search_fallbacks() == 0
        ridx, rsc = c_oracle.retrieve_topk(db, qs, k)
        kk = ridx.shape[1]
        got_i, got_s = idx.cpu().numpy().astype(np.int64), sc.cpu().numpy()
        assert np.array_equal(got_i[:, :kk], ridx + 11)
        assert np.abs(got_s[:, :kk] - rsc).max() <= 1e-12 * max(1.0, float(np.abs(rsc).max()))
        if kk < k:
            assert (got_i[:, kk:] == -1).all() and np.isneginf(got_s[:, kk:]).all()
        # the batched path on the same call: same ids, the SAME float64 bits
        e.set_option("search_small", 0)
        idx0, sc0 = e.search(dq, k)
        torch.cuda.synchronize()
        assert e.kernel_stats("search_small")[1] == 0
        e.set_option("search_small", 1)
        assert torch.equal(idx0, idx) and torch.equal(sc0, sc)
        # other query counts right behind it (1, then 16, then 3: the slices' ticket bases diverge and are levelled again), every result checked
        for q2 in (1, 16, 3, 16):
            qs2 = synth.make_queries_for(db, q2, seed=q2 + n, noise=1.0)[0] if n > 1 else qs[:1].repeat(q2, axis=0)
            i2, s2 = e.search(torch.from_numpy(np.ascontiguousarray(qs2)).cuda(), min(k, 10))
            r2, _ = c_oracle.retrieve_topk(db, qs2, min(k, 10))
            assert np.array_equal(i2.cpu().numpy().astype(np.int64)[:, : r2.shape[1]], r2 + 11), (n, q2)
        # fewer workgroups per slice (option): same result
        e.set_option("search_small_wgs", 8)
        i3, s3 = e.search(dq, k)
        e.set_option("search_small_wgs", 0)
        assert torch.equal(i3, idx) and torch.equal(s3, sc)
        # exact ties: every row twice (some three times) -> lower row first
        m = min(n, 300)
        db2 = np.concatenate([db[:m], db[:m], db[: m // 3]], axis=0)
        e.db_set(torch.from_numpy(db2).cuda(), 0)
        i4, s4 = e.search(dq, min(k, 10))
        r4, rs4 = c_oracle.retrieve_topk(db2, qs, min(k, 10))
        assert np.array_equal(i4.cpu().numpy().astype(np.int64)[:, : r4.shape[1]], r4)
        # a zero query: all scores 0 (also -0.0 x row products): (score desc, row asc) = rows 0, 1, 2, ...
        z = np.zeros((1, 256), dtype=np.float32)
        i5, s5 = e.search(torch.from_numpy(z).cuda(), min(k, 10))
        kk5 = min(min(k, 10), len(db2))
        assert np.array_equal(i5.cpu().numpy()[0, :kk5], np.arange(kk5)) and (s5.cpu().numpy()[0, :kk5] == 0).all()
    finally:
        e.close()


def _clustered_problem(n, q, spread, seed):
    """rows = one direction + `spread`-sized perturbations (score gaps far below every scan's error band), queries = rows +
    a quarter of that spread"""
    rs = np.random.default_rng(seed)
    base = synth.unit_rows(rs.standard_normal((1, 256)))
    db = synth.unit_rows(base + spread * rs.standard_normal((n, 256))).astype(np.float32)
    tgt = rs.integers(0, n, size=q)
    qs = synth.unit_rows(db[tgt].astype(np.float64) + 0.25 * spread * rs.standard_normal((q, 256))).astype(np.float32)
    return db, qs


@pytest.mark.parametrize("n,q,k,spread", [(11259, 700, 10, 1e-3), (3000, 130, 5, 1e-4), (40, 33, 10, 1e-3), (5000, 64, 26, 1e-3)])
def test_float64_mfma_exact_stage_on_clustered_database(n, q, k, spread):
    """heavy mode (search_exact.hip): queries the certificates cannot settle are ranked by the float64 MFMA scan — ids and
    scores must still be exactly the float64 ranking."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    db, qs = _clustered_problem(n, q, spread, seed=n + q)
    e = Engine(0)
    try:
        e.set_option("search_auto", 0)
        e.set_option("search_heavy", 1)
        e.set_option("search_wide_repair", 0)  # this test is about the exact stages behind the re-rank's repairs
        e.set_option("profile_events", 1)
        e.db_set(torch.from_numpy(db).cuda(), 3)
        idx, sc = e.search(torch.from_numpy(qs).cuda(), k)
        torch.cuda.synchronize()
        ridx, rsc = c_oracle.retrieve_topk(db, qs, k)
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx + 3)
        assert np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
        assert e.search_fallbacks() > q // 2  # the exact stage really served them
        assert e.kernel_stats("search_exact")[1] >= 1
        # exact duplicates: more ties than the stage re-scores -> its certificate fails -> the VALU scan decides, lower row first
        db2 = np.concatenate([db[:20]] * 3, axis=0)
        e.db_set(torch.from_numpy(db2).cuda(), 0)
        idx2, _ = e.search(torch.from_numpy(qs[:9]).cuda(), min(k, 10))
        r2, _ = c_oracle.retrieve_topk(db2, qs[:9], min(k, 10))
        assert np.array_equal(idx2.cpu().numpy().astype(np.int64), r2)
    finally:
        e.close()


def test_auto_mode_moves_a_clustered_database_to_the_exact_stage():
    """no option set: the report card of earlier calls switches the engine to the float64 MFMA stage, and back on friendly data"""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    db, qs = _clustered_problem(4000, 512, 1e-3, seed=9)
    e = Engine(0)
    try:
        e.set_option("profile_events", 1)
        e.db_set(torch.from_numpy(db).cuda())
        dq = torch.from_numpy(qs).cuda()
        ridx, _ = c_oracle.retrieve_topk(db, qs, 10)
        for _ in range(8):
            idx, _ = e.search(dq, 10)
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx)
        assert e.kernel_stats("search_exact")[1] >= 1  # engaged within a few calls
        db3, qs3, _ = synth.make_retrieval_problem(4000, 512, seed=3, noise=0.5)
        e.db_set(torch.from_numpy(db3).cuda())
        r3, _ = c_oracle.retrieve_topk(db3, qs3, 10)
        for _ in range(8):
            idx, _ = e.search(torch.from_numpy(qs3).cuda(), 10)
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy().astype(np.int64), r3)
        e.kernel_stats("search_exact")
        for _ in range(3):
            e.search(torch.from_numpy(qs3).cuda(), 10)
        torch.cuda.synchronize()
        assert e.kernel_stats("search_exact")[1] == 0  # released again
    finally:
        e.close()


@pytest.mark.parametrize("lanes", [2, 4])  # (3, the bench's side measurement, is checked there: results_equal_stream_ordered)
def test_pipelined_searches_equal_stream_ordered_ones(lanes):
    """t2l_set_option("search_lanes", n) + t2l_search_join: consecutive calls run on internal streams and overlap; every call's
    (ids, scores) are those of the stream-ordered call, whatever mix of batch sizes (small batches and the streaming scan
    join and run in the caller's stream), and the database may be replaced while calls are in flight."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    eng = Engine(0)
    db, q0, _ = synth.make_retrieval_problem(11259, 4096, seed=3, noise=0.5)
    batches = [q0, synth.make_queries_for(db, 1000, seed=5, noise=0.5)[0], synth.make_queries_for(db, 257, seed=6, noise=2.0)[0],
               synth.make_queries_for(db, 31, seed=7, noise=0.5)[0], synth.make_queries_for(db, 4096, seed=8, noise=0.5)[0]]
    d_db = torch.from_numpy(db).cuda()
    d_q = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in batches]
    eng.db_set(d_db)
    ref = [tuple(t.clone() for t in eng.search(q, 10)) for q in d_q]
    torch.cuda.synchronize()
    ridx, rsc = c_oracle.retrieve_topk(db, batches[1], 10)
    assert np.array_equal(ref[1][0].cpu().numpy(), ridx)
    eng.set_option("search_lanes", lanes)
    n_calls = 37
    outs = [eng.search(d_q[i % len(d_q)], 10, join=False) for i in range(n_calls)]
    eng.search_join()
    torch.cuda.synchronize()
    for i, (idx, sc) in enumerate(outs):
        assert torch.equal(idx, ref[i % len(d_q)][0]) and torch.equal(sc, ref[i % len(d_q)][1]), i
    # join=True (the default) keeps the stream-ordered contract call by call
    idx, sc = eng.search(d_q[0], 10)
    assert torch.equal(idx.cpu(), ref[0][0].cpu())
    # a new database while calls are in flight: db_set orders itself behind them
    db2 = np.ascontiguousarray(db[::-1])
    pending = [eng.search(d_q[0], 10, join=False) for _ in range(5)]
    eng.db_set(torch.from_numpy(db2).cuda())
    after = [eng.search(d_q[4], 10, join=False) for _ in range(3)]
    eng.search_join()
    torch.cuda.synchronize()
    for idx, sc in pending:
        assert torch.equal(idx, ref[0][0])
    r2, _ = c_oracle.retrieve_topk(db2, batches[4], 10)
    for idx, sc in after:
        assert np.array_equal(idx.cpu().numpy(), r2)
    c = eng.search_counters()
    assert c["valu_exact_scans"] == 0
    eng.set_option("search_lanes", 1)
    idx, sc = eng.search(d_q[4], 10)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), r2)
    eng.close()


def test_scan_mapping_option_is_result_neutral():
    """search_xcd_qgroups (which workgroups share an XCD) changes speed only: ids AND float64 scores are bit-identical,
    stream-ordered and pipelined, including a query count that is not a multiple of 256 and rows that are not a multiple of 32."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    e = Engine(0)
    try:
        for n, q in ((11259, 4096), (5000, 1000), (11259, 257)):
            db, qs, _ = synth.make_retrieval_problem(n, q, seed=77 + q, noise=0.7)
            e.db_set(torch.from_numpy(db).cuda())
            dq = torch.from_numpy(qs).cuda()
            e.set_option("search_xcd_qgroups", 1)
            ref_i, ref_s = (t.clone() for t in e.search(dq, 10))
            if q <= 1000:
                ridx, rsc = c_oracle.retrieve_topk(db, qs, 10)
                assert np.array_equal(ref_i.cpu().numpy().astype(np.int64), ridx) and np.abs(ref_s.cpu().numpy() - rsc).max() < 1e-12
            for gq in (1, 2, 4, 8):
                e.set_option("search_xcd_qgroups", gq)
                i1, s1 = e.search(dq, 10)
                assert torch.equal(i1, ref_i) and torch.equal(s1, ref_s), (n, q, gq)
            e.set_option("search_lanes", 3)
            outs = [e.search(dq, 10, join=False) for _ in range(5)]
            e.search_join()
            e.set_option("search_lanes", 1)
            assert all(torch.equal(o[0], ref_i) and torch.equal(o[1], ref_s) for o in outs)
        e.set_option("search_xcd_qgroups", 4)
        with pytest.raises(Exception, match="1, 2, 4 or 8"):
            e.set_option("search_xcd_qgroups", 3)
        for gone in ("search_fused", "search_prep"):  # round 5: measured slower, removed from the product
            with pytest.raises(Exception, match="unknown option"):
                e.set_option(gone, 1)
    finally:
        e.close()


def test_merge_kernel_randomised_against_the_host_merge():
    """tools/fuzz_merge.py (60 draws here): random part counts, k, query counts, short lists, empty parts, exact ties across parts,
    scores over sixty decades, scores packed tighter than float32 resolves (the merge's float32 bound must stay a LOWER bound)
    and negative scores — t2l_merge_gathered and t2l_merge_topk equal the host merge bit for bit."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("fuzz_merge", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "tools", "fuzz_merge.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(60, 17) == 0


def _cluster_db(rng, n, clusters, alpha):
    cent = synth.unit_rows(rng.standard_normal((clusters, 256)))
    return synth.unit_rows(alpha * cent[rng.integers(0, clusters, size=n)] + synth.unit_rows(rng.standard_normal((n, 256)))).astype(np.float32)


@pytest.mark.parametrize("kind,n,q,k", [("gauss", 11259, 4096, 10), ("gauss", 11259, 1000, 10), ("gauss", 1023, 257, 10), ("gauss", 4097, 300, 5),
                                        ("clusters3", 11259, 2048, 10), ("clusters6", 6000, 700, 10), ("runs16", 11259, 1024, 10),
                                        ("dups", 3000, 512, 10)])
def test_merged_candidate_records_equal_the_plain_lists(kind, n, q, k):
    """``search_merge_lists``: the paired scan hands the re-rank ONE 32-byte record per (query, workgroup) — the best 7 of the workgroup's
    24 kept keys, the source list in two extra code bits, + a bound on everything else — instead of four 24-byte lists. Same ids, same
    float64 scores bit for bit, on benign data, on clusters (where records overflow and the bound sends queries to the repairs), on runs
    of 16 near-identical neighbouring rows (one lane's list overflows) and on exact duplicates (ties: lower row first)."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    rng = np.random.default_rng(n + q)
    if kind == "gauss":
        db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    elif kind.startswith("clusters"):
        db = _cluster_db(rng, n, 64, float(kind[8:]))
    elif kind == "runs16":
        base = synth.unit_rows(rng.standard_normal(((n + 15) // 16, 256)))
        db = synth.unit_rows(3.0 * np.repeat(base, 16, axis=0)[:n] + synth.unit_rows(rng.standard_normal((n, 256)))).astype(np.float32)
    else:
        db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
        db[rng.integers(0, n, size=n // 3)] = db[rng.integers(0, n, size=n // 3)]
    qs = synth.unit_rows(db[rng.integers(0, n, size=q)].astype(np.float64) + 0.3 * synth.unit_rows(rng.standard_normal((q, 256)))).astype(np.float32)
    ridx, rsc = c_oracle.retrieve_topk(db, qs, k)
    e = Engine(0)
    try:
        e.set_option("search_auto", 0)
        e.db_set(torch.from_numpy(db).cuda())
        qd = torch.from_numpy(qs).cuda()
        got = {}
        for merge in (0, 1, "lists of 5"):  # (the third arm: plain lists of 5 keys per lane, option search_pair_ll)
            e.set_option("search_merge_lists", 0 if merge == "lists of 5" else merge)
            e.set_option("search_pair_ll", 5 if merge == "lists of 5" else 6)
            idx, sc = e.search(qd, k)
            torch.cuda.synchronize()
            got[merge] = (idx.cpu().numpy().astype(np.int64), sc.cpu().numpy(), e.search_counters())
            assert np.array_equal(got[merge][0], ridx), (merge, got[merge][2])
            assert np.abs(got[merge][1] - rsc).max() < 1e-12
        assert np.array_equal(got[0][1], got[1][1])
        if kind == "gauss":  # benign data: neither format needs a repair worth the name
            assert got[0][2]["valu_exact_scans"] == 0 and got[1][2]["valu_exact_scans"] == 0 and got[1][2]["rescored"] <= 8, (got[0][2], got[1][2])
    finally:
        e.close()


def _plane_rows(n):
    """row of plane position p (csrc/search_dev.h: plane_row; one segment): slot j of full tile t holds row j * F + t, F = n // 32."""
    p = np.arange(n)
    full = n // 32
    t, j = p // 32, p % 32
    return np.where(t < full, j * full + t, p)


def test_three_best_rows_in_one_tile_local_group_are_repaired_in_the_wave():
    """The paired scan keeps the best TWO keys of every group of 8 accumulator registers (search_dev.h: TileSelLists) and hands the third
    to the re-rank as the record's B1. Here every query's three best rows sit in ONE such group — plane slots 0, 1, 2 of one tile, i.e.
    rows t, F + t, 2 F + t of the strided plane — so the third is dropped by construction: the re-rank must find it again by re-scoring
    the 8 rows of B1's group (the 'group repair', counted as `rescored`), not by an exact scan of the shard and not by a wide repair;
    ids and float64 scores equal the oracle's. The same database under the per-score insertion (search_tile_sel = 0) needs no repair."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    rng = np.random.default_rng(77)
    n, q = 11259, 320  # (>= 256 queries: the paired scan; one tile per query out of the 351 full tiles)
    full = n // 32
    db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    qs = synth.unit_rows(rng.standard_normal((q, 256))).astype(np.float32)
    tiles = rng.choice(full, size=q, replace=False)
    for i, t in enumerate(tiles):  # three near-copies of query i at plane slots 0, 1, 2 of tile t
        for j, noise in enumerate((0.35, 0.45, 0.55)):
            db[j * full + t] = synth.unit_rows((qs[i].astype(np.float64) + noise * synth.unit_rows(rng.standard_normal((1, 256)))[0])[None])[0]
    # ... and for the last 40 queries a SECOND such triple in the neighbouring tile (another workgroup's record): two B1 keys in reach —
    # the anticipated one-trip repair steps aside and the general in-wave path re-scores both groups (compacted through LDS)
    two = np.arange(q - 40, q)
    free = np.setdiff1d(np.arange(full), np.concatenate([tiles, tiles + 1, tiles - 1]))
    second = {int(i): int(t) for i, t in zip(two, free[:len(two)])}
    for i, t in second.items():
        for j, noise in enumerate((0.4, 0.5, 0.6)):
            db[j * full + t] = synth.unit_rows((qs[i].astype(np.float64) + noise * synth.unit_rows(rng.standard_normal((1, 256)))[0])[None])[0]
    rows = _plane_rows(n)
    assert all(rows[32 * t + j] == j * full + t for t in tiles[:8] for j in range(3))
    ridx, rsc = c_oracle.retrieve_topk(db, qs, 10)
    assert all({tiles[i], full + tiles[i], 2 * full + tiles[i]} <= set(ridx[i][:6]) for i in range(q))
    assert all({t, full + t, 2 * full + t} <= set(ridx[i][:6]) for i, t in second.items())
    e = Engine(0)
    try:
        e.set_option("search_auto", 0)
        e.set_option("search_merge_lists", 1)  # merged records whatever the report card says: the selection under test needs them
        e.db_set(torch.from_numpy(db).cuda())
        qd = torch.from_numpy(qs).cuda()
        out = {}
        for sel in (1, 0):
            e.set_option("search_tile_sel", sel)
            idx, sc = e.search(qd, 10)
            torch.cuda.synchronize()
            out[sel] = e.search_counters()
            assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx), sel
            assert np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
        # (measured: 294 of the 320 queries repaired in the wave, 1 in an exact scan, 25 certified without: a wave's LAST tile — one in
        # eleven — is inserted score by score in the scan's epilogue, nothing of it is dropped)
        assert out[1]["valu_exact_scans"] <= 2 and out[1]["wide_repairs"] <= 2, out
        assert out[1]["rescored"] >= q * 8 // 10, out
        assert out[0]["rescored"] <= 8 and out[0]["valu_exact_scans"] == 0, out
    finally:
        e.close()


def test_merged_records_follow_the_report_card():
    """Default (``search_merge_lists = 2``): merged records while next to no query fails its first certificate; a clustered database moves
    the engine to plain lists within a few calls (a repair behind a merged record re-scores 4x the rows: the wide repair's cap sends those
    queries to exact scans), and a benign database brings the records back. Results are the oracle's throughout."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    rng = np.random.default_rng(5)
    n, q = 11259, 2048
    benign = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
    # runs of 16 near-identical rows that are neighbours IN THE SCAN'S PLANE (the plane deals rows to tiles strided, so that runs of
    # neighbouring database rows — overlapping cells — never meet in a tile: here they are placed where they do): eight of a run sit
    # in ONE lane's list of six
    base = synth.unit_rows(rng.standard_normal(((n + 15) // 16, 256)))
    tight_plane = synth.unit_rows(3.0 * np.repeat(base, 16, axis=0)[:n] + synth.unit_rows(rng.standard_normal((n, 256)))).astype(np.float32)
    tight = np.empty_like(tight_plane)
    tight[_plane_rows(n)] = tight_plane
    e = Engine(0)
    try:
        def calls(db, times):
            qs = synth.unit_rows(db[rng.integers(0, n, size=q)].astype(np.float64) + 0.3 * synth.unit_rows(rng.standard_normal((q, 256)))).astype(np.float32)
            ridx, _ = c_oracle.retrieve_topk(db, qs, 10)
            e.db_set(torch.from_numpy(db).cuda())
            qd = torch.from_numpy(qs).cuda()
            out = []
            for _ in range(times):
                idx, _ = e.search(qd, 10)
                torch.cuda.synchronize()
                assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx)
                out.append(e.search_counters())
            return out

        c = calls(benign, 3)
        assert all(x["valu_exact_scans"] == 0 and x["wide_repairs"] == 0 for x in c), c
        c = calls(tight, 6)
        # the first calls run on merged records (overflowing records -> exact scans); once the report card is in, plain lists and
        # their wide repairs take over
        assert c[0]["valu_exact_scans"] > 100, [(x["valu_exact_scans"], x["wide_repairs"]) for x in c]
        assert c[-1]["wide_repairs"] > 0 and c[-1]["valu_exact_scans"] < c[0]["valu_exact_scans"] // 2, [(x["valu_exact_scans"], x["wide_repairs"]) for x in c]
        c = calls(benign, 4)
        assert all(x["valu_exact_scans"] == 0 for x in c), c
    finally:
        e.close()


def test_merged_records_with_the_exact_stage_and_pipelined_lanes():
    """Forced combinations the report card never picks by itself: merged records + heavy mode (flagged queries deferred to the float64
    MFMA stage) on a database that defeats the certificates, and merged records under three pipelined lanes."""
    import torch
    from oracle import c_oracle
    from text2loc_amd.engine import Engine

    rng = np.random.default_rng(91)
    n, q = 11259, 1024
    e = Engine(0)
    try:
        e.set_option("search_auto", 0)
        e.set_option("search_merge_lists", 1)
        db = _cluster_db(rng, n, 64, 30.0)
        qs = synth.unit_rows(db[rng.integers(0, n, size=q)].astype(np.float64) + 0.01 * synth.unit_rows(rng.standard_normal((q, 256)))).astype(np.float32)
        ridx, rsc = c_oracle.retrieve_topk(db, qs, 10)
        e.set_option("search_heavy", 1)
        e.db_set(torch.from_numpy(db).cuda())
        idx, sc = e.search(torch.from_numpy(qs).cuda(), 10)
        torch.cuda.synchronize()
        cnt = e.search_counters()
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx) and np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
        assert cnt["deferred_to_mfma_exact"] > 0, cnt
        e.set_option("search_heavy", 0)
        db = synth.unit_rows(rng.standard_normal((n, 256))).astype(np.float32)
        e.db_set(torch.from_numpy(db).cuda())
        e.set_option("search_lanes", 3)
        batches = [synth.unit_rows(rng.standard_normal((777, 256))).astype(np.float32) for _ in range(7)]
        outs = [e.search(torch.from_numpy(b).cuda(), 10, join=False) for b in batches]
        e.search_join()
        torch.cuda.synchronize()
        for b, (idx, sc) in zip(batches, outs):
            ridx, rsc = c_oracle.retrieve_topk(db, b, 10)
            assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx) and np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
    finally:
        e.close()
