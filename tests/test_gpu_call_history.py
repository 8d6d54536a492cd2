"""GPU tier: no entry point may depend on what an earlier call left in the context's workspaces (reduce_ws, loss_ws, the text head's
W->ws, small_part and its ticket counters, the scan's record buffers, the PointNet++ and fine-stage scratch).

Per case: the small call S on a FRESH engine gives the reference bits, flags and counters. A second engine first runs a dirtying
call D — larger, differently ragged, and through inputs the API accepts full of huge or non-finite values — and then S: the same
bits, flags and counters. Then D and S once more on that engine (S, D, S on one context agrees with itself). S is taken from
tests/test_gpu_memory_safety.py, where it is held to its oracle.

The one exemption is that file's: reduce_objects on objects over 4096 points adds float64 partial sums with atomicAdd
(reduce_partial_kernel), so those objects are held to the 3e-5 bar of tests/test_gpu_reduce.py instead of to the same bits.
"""
import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from tests.test_gpu_memory_safety import COLOR_ROWS, REDUCE_SIZES, cells_with_counts, dev, engine, reduce_problem, same_bits
from text2loc_amd import packing, synth

pytestmark = pytest.mark.gpu


def snapshot(values):
    """Tensors are copied (the next call may reuse their memory); everything else is kept as it is."""
    torch.cuda.synchronize()
    return {k: v.clone() if torch.is_tensor(v) else v for k, v in values.items()}


def assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        if torch.is_tensor(ref[k]):
            assert same_bits(got[k], ref[k]), f"{what}: {k} differs from the fresh engine's bits"
        else:
            assert got[k] == ref[k], f"{what}: {k} = {got[k]}, the fresh engine gave {ref[k]}"


def check_history(make, dirty, smalls):
    """``make() -> Engine``; ``dirty(e)``; ``smalls``: calls ``S(e) -> dict`` run in this order behind the dirtying call."""
    refs = []
    for S in smalls:
        e = make()
        try:
            refs.append(snapshot(S(e)))
        finally:
            e.close()
    e = make()
    try:
        for visit in ("after the dirtying call", "after the second dirtying call"):
            dirty(e)
            for i, (S, ref) in enumerate(zip(smalls, refs)):
                assert_same(snapshot(S(e)), ref, f"small call {i} {visit}")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ search
def search_small_call(db, qs, k, many=False):
    d_db, d_q = dev(db), dev(qs)

    def S(e):
        e.db_set(d_db)
        idx, sc = (e.search_many if many else e.search)(d_q, k)
        return {"idx": idx, "score": sc, "fallbacks": e.search_fallbacks(), "counters": e.search_counters()}

    return S


def search_dirty():
    """11,259 rows x 1e30 against 300 queries x 1e-7 (magnitudes tests/test_gpu_search.py: test_scale_invariance shows are served):
    squares of the rows overflow float32, so whatever the scan and the re-rank park in their scratch is huge or non-finite."""
    db, qs, _ = synth.make_retrieval_problem(11259, 300, seed=13, noise=2.0)
    d_db, d_q = dev((db * np.float32(1e30)).astype(np.float32)), dev((qs * np.float32(1e-7)).astype(np.float32))

    def D(e):
        e.db_set(d_db)
        e.search(d_q, 26)

    return D


SEARCH_PATHS = {
    "paired-f16": (dict(search_mode=0, search_small=0), (33, 129, 10)),
    "paired-bf16x3": (dict(search_mode=2, search_small=0), (33, 129, 10)),
    "one-launch": (dict(), (33, 4, 10)),
    "streaming": (dict(stream_min_rows=1), (33, 5, 10)),
    "forced-fallback": (dict(certify_eps_scale=1e9, search_small=0), (33, 40, 10)),
}


@pytest.mark.parametrize("path", list(SEARCH_PATHS))
def test_search_after_a_huge_database(path):
    options, (n, q, k) = SEARCH_PATHS[path]
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=100 + n, noise=2.0)
    smalls = [search_small_call(db, qs, k)]
    if path == "paired-f16":
        db2, qs2, _ = synth.make_retrieval_problem(1000, 3 * 129, seed=41, noise=2.0)
        smalls.append(search_small_call(db2, qs2.reshape(3, 129, 256), 10, many=True))
    check_history(lambda: engine(**options), search_dirty(), smalls)


def test_exact_stage_after_a_huge_database():
    from tests.test_gpu_search import _clustered_problem

    db, qs = _clustered_problem(33, 33, 1e-3, seed=66)
    S = search_small_call(db, qs, 10)

    def checked(e):
        out = S(e)
        assert out["fallbacks"] > 33 // 2  # the float64 MFMA stage served them, fresh or not
        return out

    check_history(lambda: engine(search_auto=0, search_heavy=1, search_wide_repair=0), search_dirty(), [checked])


def test_one_launch_path_from_16_queries_to_1_to_13():
    """The slices' ticket counters and published lists are reused across query counts (search_small.hip)."""
    db, qs, _ = synth.make_retrieval_problem(700, 16, seed=905, noise=1.5)
    d_db, d_q = dev(db), dev((qs * np.float32(3e4)).astype(np.float32))

    def D(e):
        e.db_set(d_db, 11)
        e.search(d_q, 26)

    def S(q):
        dq = dev(synth.make_queries_for(db, q, seed=q, noise=1.0)[0])

        def call(e):
            e.db_set(d_db, 11)
            idx, sc = e.search(dq, 10)
            return {"idx": idx, "score": sc, "fallbacks": e.search_fallbacks(), "counters": e.search_counters()}

        return call

    check_history(lambda: engine(), D, [S(1), S(13)])


# ------------------------------------------------------------------------------------------------------------------ merge
def test_merge_after_a_larger_merge(P=3, Q=5, K=10):
    rng = np.random.default_rng(5)

    def parts(P, Q, K, scale):
        idx = np.stack([np.stack([rng.permutation(1000)[:K] for _ in range(Q)]) + 1000 * p for p in range(P)]).astype(np.int32)
        return dev(idx), dev(-np.sort(-rng.standard_normal((P, Q, K)), axis=2) * scale)

    big_i, big_s = parts(8, 129, 26, 1e300)
    big_s[3, :, 5:] = float("inf")
    i, s = parts(P, Q, K, 1.0)

    def D(e):
        e.merge_topk(big_i, big_s)
        e.merge_pairs(torch.stack([e.pack_pairs(big_i[p], big_s[p]) for p in range(8)]))

    def S(e):
        mi, ms = e.merge_topk(i, s)
        pi, ps = e.merge_pairs(torch.stack([e.pack_pairs(i[p], s[p]) for p in range(P)]))
        return {"idx": mi, "score": ms, "pair_idx": pi, "pair_score": ps}

    check_history(lambda: engine(), D, [S])


# ------------------------------------------------------------------------------------------------------------------ reduce_objects
def test_reduce_objects_after_a_huge_object():
    rs = np.random.default_rng(1)
    big_xyz = dev((rs.uniform(0, 1, (60000, 3)) * 1e6).astype(np.float32))
    big_rgb = dev((rs.uniform(0, 1, (60000, 3)) * 1e6).astype(np.float32))
    sizes = list(REDUCE_SIZES)
    xyz, rgb, poff = reduce_problem(sizes, seed=9)
    d_xyz, d_rgb = dev(xyz), dev(rgb)
    small = torch.from_numpy(np.array([n <= 4096 for n in sizes])).cuda()

    def D(e):
        e.reduce_objects(big_xyz, big_rgb, np.array([0, 60000], dtype=np.int64), packing.COLORS, COLOR_ROWS)

    def S(e):
        out = e.reduce_objects(d_xyz, d_rgb, poff, packing.COLORS, COLOR_ROWS)
        for i in (j for j, n in enumerate(sizes) if n > 4096):  # (float64 atomics: tests/test_gpu_reduce.py's bar instead of the bits)
            crgb, cidx, center, cnt = O.object_reductions(xyz[poff[i]:poff[i + 1]], rgb[poff[i]:poff[i + 1]], synth.COLORS)
            assert np.abs(out["rgb"][i].cpu().numpy() - crgb).max() < 3e-5 and np.abs(out["center"][i].cpu().numpy() - center).max() < 3e-5
            assert out["n_pts"][i].item() == cnt and out["color_idx"][i].item() == synth.color_name_to_embed_index(cidx)
        return {k: v[small] for k, v in out.items()}

    check_history(lambda: engine(), D, [S])


# ------------------------------------------------------------------------------------------------------------------ PointNet++ side
def test_sample_object_points_after_a_larger_batch():
    rs = np.random.default_rng(4)

    def batch(n_pts, scale):
        poff = np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int64)
        return dev((rs.standard_normal((int(poff[-1]), 3)) * scale).astype(np.float32)), dev(rs.uniform(0, 1, (int(poff[-1]), 3)).astype(np.float32)), dev(poff)

    big, small = batch([5000, 3, 700] * 7, 1e30), batch([8, 25, 300, 4000, 61], 0.08)

    def S(transform):
        def call(e):
            pos, col = e.sample_object_points(*small, seed=77, transform=transform)
            return {"pos": pos, "rgb": col}
        return call

    check_history(lambda: engine(), lambda e: e.sample_object_points(*big, seed=1, transform="rotate_normalize"),
                  [S("fixed"), S("normalize"), S("rotate_normalize")])


@pytest.mark.parametrize("f32", [0, 1], ids=["split-f16", "f32"])
def test_pointnet_features_after_the_magnitude_watch_fired(f32):
    """D: tests/test_gpu_pointnet.py's batch of thousands of objects with one object's colours x 2e5 (the magnitude watch hands it to the
    f32 kernels, its split-f16 intermediates are non-finite)."""
    sd = synth.make_object_branch_weights(0)
    sd.update(synth.make_pointnet_weights(0))

    def make():
        e = engine(encoder_f32=f32)
        e.load_weights(sd, class_embed=False, color_embed=False)
        return e

    big = synth.make_cells(150, seed=21)
    bpos, brgb = synth.make_sampled_points(big, 21)
    brgb = brgb.copy()
    brgb[int(big["offsets"][75])] *= np.float32(2.0e5)
    d_bpos, d_brgb = dev(bpos), dev(brgb)
    cells = synth.make_cells(3, seed=1, min_obj=1, max_obj=5)
    pos, rgb = (dev(a) for a in synth.make_sampled_points(cells, 1))
    check_history(make, lambda e: e.pointnet_features(d_bpos, d_brgb, big["offsets"]),
                  [lambda e: {"features2": e.pointnet_features(pos, rgb, cells["offsets"])}])


# ------------------------------------------------------------------------------------------------------------------ encode_cells
@pytest.mark.parametrize("two_cells", [1, 0], ids=["two-cells", "one-cell"])
def test_encode_cells_after_features_beyond_the_f16_range(two_cells):
    """D: 300 cells of 6..35 objects (an even count, other raggedness) with one object's pn_feat and mean colour x 1e6: beyond the range
    the split-f16 form is safe for, so the guarded cells are redone by the f32 kernel and the flag lists are in use."""
    sd = synth.make_object_branch_weights(3)

    def make():
        e = engine(encoder_two_cells=two_cells)
        e.load_weights(sd, class_embed=False, color_embed=False)
        return e

    big = synth.make_cells(300, seed=4, with_pn_feat=True)
    o = int(big["offsets"][150]) + 2
    big["pn_feat"][o] *= np.float32(1e6)
    big["rgb"][o] *= np.float32(1e6)
    d_big = {k: dev(v) for k, v in big.items() if k != "counts"}
    smalls = []
    for counts in ((1, 29, 40), (40,)):
        d_cells = {k: dev(v) for k, v in cells_with_counts(counts, seed=12).items() if k != "counts"}
        smalls.append(lambda e, c=d_cells: {"emb": e.encode_cells(c)})
    check_history(make, lambda e: e.encode_cells(d_big), smalls)


# ------------------------------------------------------------------------------------------------------------------ text head
HEAD_SD = {}


def head_engine():
    if not HEAD_SD:
        HEAD_SD.update(synth.make_language_head_weights(3))
    e = engine()
    e.text_head_load_weights(HEAD_SD)
    return e


def test_text_head_after_an_overflowing_batch():
    hidden = synth.make_t5_hidden(40, 13, seed=4013)
    hidden[2, 3, 100] = np.nan
    hidden[31, 12, 7] = 4.0e4
    d_big = dev(hidden)

    def D(e):
        _, bad = e.text_head(d_big)
        assert bad  # the flag is raised ...

    def S(n_sent, L):
        d = dev(synth.make_t5_hidden(n_sent, L, seed=n_sent * 100 + L))

        def call(e):
            out, bad = e.text_head(d)
            return {"out": out, "overflow": bad}  # ... and is per call
        return call

    check_history(head_engine, D, [S(2, 17), S(1, 1)])


def test_text_inter_after_an_overflowing_batch():
    sent = np.random.default_rng(7).standard_normal((40 * 13, 256)).astype(np.float32)
    sent[17, 3] = np.nan
    sent[400, 200] = 4.0e4
    d_big = dev(sent)

    def D(e):
        _, bad = e.text_inter(d_big, 40)
        assert bad

    def S(n_desc, n_sent):
        d = dev(np.random.default_rng(n_desc * 100 + n_sent).standard_normal((n_desc * n_sent, 256)).astype(np.float32))

        def call(e):
            out, bad = e.text_inter(d, n_desc)
            return {"out": out, "overflow": bad}
        return call

    check_history(head_engine, D, [S(2, 17), S(1, 1)])


# ------------------------------------------------------------------------------------------------------------------ fine stage
@pytest.mark.parametrize("f32", [0, 1], ids=["split-f16", "f32"])
def test_fine_stage_after_the_norm_guard_fired(f32):
    """D: tests/test_gpu_fine.py's largest case (37 cells, 530 pairs by index) with hint rows x 40 and x 3e3 — its norm-guard case — and
    cells whose centres and point counts are x 1e6."""
    sd = synth.make_fine_weights(3)

    def make():
        e = engine(encoder_f32=f32)
        e.fine_load_weights(sd, class_embed=True, color_embed=True)
        return e

    keys = ("offsets", "class_idx", "color_idx", "rgb", "center", "n_pts")
    big = synth.make_cells(37, seed=77, min_obj=16, max_obj=16)
    big["center"][5::7] *= np.float32(1e6)
    big["n_pts"][3::5] *= np.float32(1e6)
    d_big = {k: dev(big[k]) for k in keys}
    rng = np.random.default_rng(5)
    hints = rng.standard_normal((53, 6, 128)).astype(np.float32)
    hints[2] *= 40.0
    hints[7] *= 3.0e3
    d_hints, ci = dev(hints), dev(rng.integers(0, 37, size=530).astype(np.int32))
    hi = torch.arange(53, dtype=torch.int32, device="cuda").repeat_interleave(10)

    def D(e):
        e.fine_match(e.fine_encode_objects(d_big), d_hints, ci, hi)

    cells = synth.make_cells(5, seed=2, min_obj=16, max_obj=16)
    d_cells = {k: dev(cells[k]) for k in keys}
    d_h = dev(rng.standard_normal((5, 6, 128)).astype(np.float32))
    d_h1 = dev(rng.standard_normal((1, 8, 128)).astype(np.float32))

    def S(e):
        desc = e.fine_encode_objects(d_cells)
        return {"desc": desc, "offsets": e.fine_match(desc, d_h), "one_pair": e.fine_match(desc[:1].contiguous(), d_h1)}

    check_history(make, D, [S])


# ------------------------------------------------------------------------------------------------------------------ contrastive loss
def loss_call(B, scale, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, 256)).astype(np.float32)
    p = (a + 0.8 * rng.standard_normal((B, 256))).astype(np.float32)
    d_a, d_p = dev(a * np.float32(scale)), dev(p * np.float32(scale))

    def call(e):
        loss, ga, gp = e.contrastive_loss(d_a, d_p, 0.1)
        forward_only = e.contrastive_loss(d_a, d_p, 0.1, need_grad=False)[0]
        return {"loss": loss, "grad_anchor": ga, "grad_positive": gp, "forward_only": forward_only}

    return call


def test_chained_loss_after_1024_huge_rows():
    """129 and 200 rows lay the [B][B] matrix out at other strides in the workspace 1024 rows x 1e18 filled."""
    check_history(lambda: engine(), loss_call(1024, 1e18, 0), [loss_call(129, 1.0, 129), loss_call(200, 1.0, 200)])


def test_fused_loss_after_128_huge_rows():
    check_history(lambda: engine(), loss_call(128, 1e18, 1), [loss_call(33, 1.0, 33)])
