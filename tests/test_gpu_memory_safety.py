"""GPU tier: guard bands around every tensor an ``Engine`` entry point is handed or allocates (tests/guards.py).

Each case runs once with ordinary tensors and once per float fill (quiet NaN, +3e38) with every device input copied between two
poisoned halos and every output the wrapper allocates carved out of a 0xA5-filled buffer. Asserted: the halos are intact, the
outputs are written in full, the guarded runs return the SAME BITS as the ordinary run (a stray read would have picked the poison
up), and the ordinary run meets its oracle at the bar of the entry point's own test file (cited at each case). Integer halos hold
in-range values (a valid class / colour row / offset / row id), so a stray read changes a result and never an address.

Bit identity is replaced by the oracle bar, for all runs, where floats are accumulated through atomics:
  reduce_objects, objects over 4096 points     reduce_partial_kernel: atomicAdd of float64 partial sums into acc[obj][6]
  encode_cells_train / encode_cells_backward   train_kernels.h: BatchNorm statistics and parameter gradients through atomicAdd /
                                               unsafeAtomicAdd (include/t2l.h: "float atomics: summation order ... varies")
  text_head_train / text_head_backward         text_head.hip: column sums and split-k partial tiles added with float atomics
  pointnet_features_train / pointnet_backward  pointnet_train.h: per-cell BatchNorm sums and gradients through atomicAdd
  fine_train_forward / fine_train_backward     fine_train.hip: BatchNorm sums and gradients through atomicAdd (t2l.h: "the last
                                               bits vary between runs")

Engine methods that take or return a device tensor and have no case here:
  train_bind, fine_train_bind, text_train_bind   bound parameter / gradient storage lives as long as the binding, not a call
  adam_state, set_adam_state, text_adam_state,   optimizer storage of the same bound tensors (copies of library-owned moments)
  set_text_adam_state
  train_sync_bn                                  a caller-owned float64 exchange buffer driven by torch.distributed, same lifetime
  fine_train_forward_points                      t2l_pointnet_features_train's kernels feeding t2l_fine_train_forward's, both covered;
                                                 its own per-call tensors are the two point arrays the backbone case guards
  result_block                                   allocates and slices, launches nothing
Library-internal workspaces cannot be guarded from here: tests/test_gpu_call_history.py covers them through dirty contexts.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import t2l_oracle as O
from oracle import t2l_oracle_fine as OF
from oracle import t2l_oracle_pointnet as OP
from tests import guards as G
from text2loc_amd import engine as E
from text2loc_amd import packing, synth

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def other_than(lo, hi, *avoid):
    """An integer in [lo, hi] that none of ``avoid`` equals: a halo value that is in range and differs from the payload's ends."""
    return next(v for v in range(lo, hi + 1) if v not in [int(a) for a in avoid])


def guard_inputs(args, fill, ints, skew=None):
    """Every CUDA tensor of ``args`` guarded: floats with ``fill``, integers with ``ints[name]`` (an int, or a function of the fill)."""
    out = {}
    for k, v in args.items():
        if not (torch.is_tensor(v) and v.is_cuda):
            out[k] = v
            continue
        f = fill if v.is_floating_point() else ints[k]
        out[k] = G.guarded(v, f(fill) if callable(f) else f, skew_bytes=(skew or {}).get(k, 0))
    return out


def run_guarded(call, args, n_alloc, ints=None, exact=True, skew=None):
    """``call(args) -> tuple of tensors``: once on ordinary tensors, once per fill guarded (each run on its own copies of ``args``, so a
    tensor the call writes into starts alike). ``exact``: the guarded outputs equal the ordinary ones bit for bit.
    Returns (ordinary outputs, [guarded outputs per fill])."""
    plain = tuple(t.clone() for t in call({k: v.clone() if torch.is_tensor(v) else v for k, v in args.items()}))
    torch.cuda.synchronize()
    runs = []
    for fill in G.FLOAT_FILLS:
        g_in = guard_inputs(args, fill, ints or {}, skew)
        with G.guarded_outputs(E) as g:
            out = tuple(call(g_in))
        assert g.count == n_alloc, (g.count, n_alloc)
        G.check_halos(*[v for v in g_in.values() if torch.is_tensor(v) and v.is_cuda])
        for i, (a, b) in enumerate(zip(out, plain)):
            assert not exact or same_bits(a, b), f"output {i} differs from the unguarded run under the {G.fill_id(fill)} fill"
        runs.append(out)
    return plain, runs


def engine(**options):
    e = E.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    return e


# ------------------------------------------------------------------------------------------------------------------ db_set + search
def check_search(got, db, qs, k, row_offset=0):
    """tests/test_gpu_search.py: ids integer-exact against c_oracle.retrieve_topk, scores to 1e-12."""
    ridx, rsc = c_oracle.retrieve_topk(db, qs.reshape(-1, 256), k)
    idx, sc = got[0].cpu().numpy().astype(np.int64).reshape(-1, k), got[1].cpu().numpy().reshape(-1, k)
    assert np.array_equal(idx, ridx + row_offset)
    assert np.abs(sc - rsc).max() < 1e-12


def search_case(e, db, qs, k, row_offset=0, many=False, skew=None):
    def call(a):
        e.db_set(a["db"], row_offset)
        return (e.search_many if many else e.search)(a["q"], k)

    plain, _ = run_guarded(call, {"db": dev(db), "q": dev(qs)}, 2, skew=skew)
    check_search(plain, db, qs, k, row_offset)


@pytest.mark.parametrize("mode", [0, 2], ids=["f16", "bf16x3"])
@pytest.mark.parametrize("n,q,k", [(33, 129, 10), (1000, 257, 26), (4097, 64, 16)])
def test_paired_scan(mode, n, q, k):
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=100 + n, noise=2.0)
    e = engine(search_mode=mode, search_small=0)
    try:
        search_case(e, db, qs, k)
    finally:
        e.close()


@pytest.mark.parametrize("n,q,k", [(31, 1, 26), (257, 4, 10), (700, 5, 10)])
def test_one_launch_search(n, q, k):
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=900 + n + q, noise=1.5)
    e = engine(profile_events=1)
    try:
        e.kernel_stats("search_small")
        search_case(e, db, qs, k, row_offset=11)
        assert e.kernel_stats("search_small")[1] == 3  # the ordinary run and both guarded ones took the one-launch path
    finally:
        e.close()


@pytest.mark.parametrize("n,q,k", [(33, 5, 10), (4097, 17, 26)])
def test_streaming_search(n, q, k):
    db, qs, _ = synth.make_retrieval_problem(n, q, seed=300 + n, noise=2.0)
    e = engine(stream_min_rows=1)
    try:
        search_case(e, db, qs, k, row_offset=7)
    finally:
        e.close()


def test_float64_mfma_exact_stage():
    from tests.test_gpu_search import _clustered_problem

    n, q, k = 40, 33, 10
    db, qs = _clustered_problem(n, q, 1e-3, seed=n + q)
    e = engine(search_auto=0, search_heavy=1, search_wide_repair=0, profile_events=1)
    try:
        search_case(e, db, qs, k, row_offset=3)
        assert e.search_fallbacks() > q // 2 and e.kernel_stats("search_exact")[1] >= 3  # the exact stage served every run
    finally:
        e.close()


def test_forced_fallback_search():
    db, qs, _ = synth.make_retrieval_problem(3000, 40, seed=5, noise=2.0)
    e = engine(certify_eps_scale=1e9)
    try:
        search_case(e, db, qs, 10)
        assert e.search_fallbacks() == 40
    finally:
        e.close()


def test_search_many():
    db, qs, _ = synth.make_retrieval_problem(1000, 3 * 129, seed=41, noise=2.0)
    e = engine()
    try:
        search_case(e, db, qs.reshape(3, 129, 256), 10, many=True)
    finally:
        e.close()


def test_search_on_row_slices():
    """A caller's row slice: ``db[5:]`` and ``queries[3:]`` start 5 and 3 rows of 1 KiB into their buffers (rows of 256 floats keep the
    16-byte alignment of the kernels' float4 loads, DESIGN.md: alignment contract). Paired scan and one-launch path."""
    for q, options in ((257, {"search_small": 0}), (5, {})):
        db, qs, _ = synth.make_retrieval_problem(700, q, seed=77, noise=2.0)
        e = engine(**options)
        try:
            search_case(e, db, qs, 10, skew={"db": 5 * 1024, "q": 3 * 1024})
        finally:
            e.close()


# ------------------------------------------------------------------------------------------------------------------ merge and pack
def byte_fill(fill):
    """The float fills as bytes of a block buffer: 0xFF.. is a float64 NaN and row id -1, 0x7F7F.. is 1.4e306 and a large positive id."""
    return 0xFF if fill != fill else 0x7F


@pytest.mark.parametrize("P,Q,K", [(3, 5, 10), (8, 129, 26)])
def test_merge_and_pack_kernels(P, Q, K):
    """(tests/test_gpu_search.py: test_hip_merge_kernel_vs_host_merge — equal to the host merge bit for bit)"""
    from text2loc_amd.sharded import merge_topk_host

    rng = np.random.default_rng(21 + P)
    idx = np.stack([np.sort(np.stack([rng.permutation(1000)[:K] for _ in range(Q)]) + 1000 * p, axis=1) for p in range(P)]).astype(np.int32)
    sc = -np.sort(-rng.standard_normal((P, Q, K)), axis=2)
    sc[1, :, 5:] = sc[1, :, 4:5]  # ties inside a part
    idx[2, :, 7:] = -1            # a short part
    sc[2, :, 7:] = -np.inf
    hi, hs = merge_topk_host(idx, sc, K)
    halo_id = other_than(0, 999, idx[0, 0, 0], idx[-1, -1, -1])
    e = engine()
    try:
        def check(got):
            assert np.array_equal(got[0].cpu().numpy().astype(np.int64), hi) and np.array_equal(got[1].cpu().numpy(), hs)

        plain, _ = run_guarded(lambda a: e.merge_topk(a["idx"], a["score"]), {"idx": dev(idx), "score": dev(sc)}, 2, ints={"idx": halo_id})
        check(plain)
        packed = []
        for p in range(P):
            one, _ = run_guarded(lambda a: (e.pack_pairs(a["idx"], a["score"]),), {"idx": dev(idx[p]), "score": dev(sc[p])}, 1,
                                 ints={"idx": halo_id})
            packed.append(one[0])
        assert np.array_equal(torch.stack(packed).cpu().numpy(), np.stack([sc, idx.astype(np.float64)], axis=-1))
        plain, _ = run_guarded(lambda a: e.merge_pairs(a["pairs"]), {"pairs": torch.stack(packed)}, 2)
        check(plain)
        buf, _, _, bb, so = e.result_block(Q, K, "cuda", parts=P)
        buf.zero_()
        for p in range(P):
            buf[p, :Q * K * 4].view(torch.int32).view(Q, K).copy_(torch.from_numpy(idx[p]))
            buf[p, so:so + Q * K * 8].view(torch.float64).view(Q, K).copy_(torch.from_numpy(sc[p]))
        plain, _ = run_guarded(lambda a: e.merge_gathered(a["blocks"], bb, so, P, Q, K), {"blocks": buf.view(-1)}, 2, ints={"blocks": byte_fill})
        check(plain)
        # the alignment contract's one refusal (include/t2l.h): a byte buffer that does not start on an 8-byte boundary is turned away
        # by the wrapper and by the C entry point, before either launches anything
        odd = torch.zeros(buf.numel() + 8, dtype=torch.uint8, device="cuda")[4:4 + buf.numel()]
        with pytest.raises(E.T2LError, match="8-byte boundary"):
            e.merge_gathered(odd, bb, so, P, Q, K)
        assert e.lib.t2l_merge_gathered(e._h, odd.data_ptr(), bb, so, P, Q, K, plain[0].data_ptr(), plain[1].data_ptr(), None) == -1
        assert b"8-byte boundary" in e.lib.t2l_last_error(e._h)
        check(plain)  # ... and the outputs it was handed are untouched
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ reduce_objects
REDUCE_SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
COLOR_ROWS = np.array([packing.color_table()[c] for c in packing.COLOR_NAMES], dtype=np.int32)


def reduce_problem(sizes, seed):
    rs = np.random.default_rng(seed)
    xyz = np.concatenate([rs.uniform(0, 1, (1, 3)) + 0.05 * rs.standard_normal((n, 3)) for n in sizes]).astype(np.float32)
    rgb = np.concatenate([np.clip(rs.uniform(0.1, 0.9, (1, 3)) + 0.05 * rs.standard_normal((n, 3)), 0, 1) for n in sizes]).astype(np.float32)
    return xyz, rgb, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def reduce_case(e, sizes, seed, skew_rows=0):
    xyz, rgb, poff = reduce_problem(sizes, seed)
    keys = ("rgb", "center", "n_pts", "color_idx")

    def call(a):
        out = e.reduce_objects(a["xyz"], a["rgb"], poff, packing.COLORS, COLOR_ROWS)
        return tuple(out[k] for k in keys)

    small = np.array([n <= 4096 for n in sizes])
    plain, runs = run_guarded(call, {"xyz": dev(xyz), "rgb": dev(rgb)}, 4, exact=False, skew={"xyz": 12 * skew_rows, "rgb": 12 * skew_rows})
    for out in [plain] + runs:
        for a, b in zip(out, plain):  # one wave, one atomicAdd into a zeroed slot: the same bits; several runs per object: the bar below
            assert same_bits(a[torch.from_numpy(small).cuda()], b[torch.from_numpy(small).cuda()])
        got = {k: v.cpu().numpy() for k, v in zip(keys, out)}
        for i, n in enumerate(sizes):  # tests/test_gpu_reduce.py: test_edge_objects (3e-5 on means of values in [0, 1]; counts and colours exact)
            crgb, cidx, center, cnt = O.object_reductions(xyz[poff[i]:poff[i + 1]], rgb[poff[i]:poff[i + 1]], synth.COLORS)
            assert np.abs(got["rgb"][i] - crgb).max() < 3e-5 and np.abs(got["center"][i] - center).max() < 3e-5, (n, i)
            assert got["n_pts"][i] == cnt and got["color_idx"][i] == synth.color_name_to_embed_index(cidx), (n, i)


@pytest.fixture(scope="module")
def plain_eng():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_reduce_objects(plain_eng, order):
    sizes = REDUCE_SIZES if order == "ascending" else tuple(np.random.default_rng(3).permutation(REDUCE_SIZES))
    reduce_case(plain_eng, [int(s) for s in sizes], seed=len(order))


def test_reduce_objects_on_row_slices(plain_eng):
    """``xyz[5:]`` / ``rgb[5:]``: the payload starts 60 bytes into its buffer, aligned to 4 bytes only (alignment contract —
    reduce.hip reads its points with scalar float loads)."""
    reduce_case(plain_eng, [1, 63, 65, 257, 4097], seed=9, skew_rows=5)


# ------------------------------------------------------------------------------------------------------------------ PointNet++ side
@pytest.fixture(scope="module", params=[0, 1], ids=["split-f16", "f32"])
def pn_eng(request):
    e = engine(encoder_f32=request.param)
    sd = synth.make_object_branch_weights(0)
    sd.update(synth.make_pointnet_weights(0))
    e.load_weights(sd, class_embed=False, color_embed=False)
    e._sd = sd
    yield e
    e.close()


@pytest.mark.parametrize("transform", ["fixed", "normalize", "rotate_normalize"])
def test_sample_object_points(plain_eng, transform):
    """(tests/test_gpu_pointnet.py: test_point_batches_sampled_on_the_gpu — colours and "fixed" positions bit for bit, 4e-6 otherwise)"""
    rs = np.random.default_rng(4)
    n_pts = np.array([8, 25, 300, 4000, 61], dtype=np.int64)
    poff = np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int64)
    xyz = (rs.uniform(0.2, 0.8, size=(5, 3)).repeat(n_pts, axis=0) + rs.standard_normal((int(poff[-1]), 3)) * 0.08).astype(np.float32)
    rgb = rs.uniform(0, 1, size=(int(poff[-1]), 3)).astype(np.float32)
    plain, _ = run_guarded(lambda a: plain_eng.sample_object_points(a["xyz"], a["rgb"], a["poff"], seed=77, transform=transform),
                           {"xyz": dev(xyz), "rgb": dev(rgb), "poff": dev(poff)}, 2, ints={"poff": other_than(0, int(poff[-1]), 0, poff[-1])})
    rpos, rcol = OP.sample_object_points(xyz, rgb, poff, 77, transform=transform)
    assert np.array_equal(plain[1].cpu().numpy(), rcol)
    if transform == "fixed":
        assert np.array_equal(plain[0].cpu().numpy(), rpos)
    else:
        assert np.abs(plain[0].cpu().numpy() - rpos).max() < 4e-6


@pytest.mark.parametrize("n_cells,min_obj,max_obj", [(1, 1, 1), (3, 1, 5)])
def test_pointnet_features(pn_eng, n_cells, min_obj, max_obj):
    """(tests/test_gpu_pointnet.py: 2e-4 of the feature scale against the build's restatement)"""
    cells = synth.make_cells(n_cells, seed=1, min_obj=min_obj, max_obj=max_obj)
    pos, rgb = synth.make_sampled_points(cells, 1)
    plain, _ = run_guarded(lambda a: (pn_eng.pointnet_features(a["pos"], a["rgb"], cells["offsets"]),), {"pos": dev(pos), "rgb": dev(rgb)}, 1)
    ref = OP.pointnet_features(pos, rgb, cells["offsets"], pn_eng._sd)
    assert np.abs(plain[0].cpu().numpy() - ref).max() < 2e-4 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------------------------ encode_cells
ENC_TOL = 2e-5  # tests/test_gpu_encoder.py, tests/test_gpu_shapes.py: TOL
OBJ_KEYS = ("class_idx", "color_idx", "rgb", "center", "n_pts", "pn_feat")


def cells_with_counts(counts, seed):
    total = int(sum(counts))
    cells = synth.make_cells(1, seed=seed, min_obj=total, max_obj=total, with_pn_feat=True)
    cells["counts"] = np.array(counts, dtype=np.int32)
    cells["offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return cells


def cell_int_fills(cells):
    """In-range halo values that differ from the payload's first and last entries: an object offset, a class row, a colour row."""
    return {"offsets": other_than(0, int(cells["offsets"][-1]), cells["offsets"][0], cells["offsets"][-1]),
            "class_idx": other_than(1, len(synth.KNOWN_CLASS), cells["class_idx"][0], cells["class_idx"][-1]),
            "color_idx": other_than(0, 7, cells["color_idx"][0], cells["color_idx"][-1])}


def encode_case(e, cells, ref, skew=None):
    args = {k: dev(v) for k, v in cells.items() if k != "counts"}
    plain, _ = run_guarded(lambda a: (e.encode_cells(a),), args, 1, ints=cell_int_fills(cells), skew=skew)
    assert np.abs(plain[0].cpu().numpy() - ref).max() < ENC_TOL


@pytest.fixture(scope="module", params=[1, 0], ids=["two-cells", "one-cell"])
def enc_eng(request):
    e = engine(encoder_two_cells=request.param)
    yield e
    e.close()


@pytest.mark.parametrize("mode", ["embed", "pn", "mixed"])
@pytest.mark.parametrize("counts", [(40,), (28, 40), (1, 29, 40), (0, 27, 40)], ids=lambda c: "-".join(map(str, c)))
def test_encode_cells_published_shape(enc_eng, mode, counts):
    """1, 2 and 3 cells (3: the odd tail workgroup of the two-cell form), object counts around object_size = 28, the over-full cell last."""
    ce, co = {"embed": (True, True), "pn": (False, False), "mixed": (True, False)}[mode]
    sd = synth.make_object_branch_weights(3)
    cells = cells_with_counts(counts, seed=12)
    enc_eng.load_weights(sd, class_embed=ce, color_embed=co)
    encode_case(enc_eng, cells, O.encode_cells(cells, sd, ce, co))


def test_encode_cells_other_shape(enc_eng):
    from tests.test_gpu_shapes import SHAPES

    D, heads, layers, osz = SHAPES[1]
    sd = synth.make_object_branch_weights(3, embed_dim=D, num_layers=layers)
    cells = cells_with_counts((1, osz + 1, 40), seed=12)
    enc_eng.load_weights(sd, class_embed=True, color_embed=False, num_layers=layers, num_heads=heads, embed_dim=D, object_size=osz)
    encode_case(enc_eng, cells, O.encode_cells(cells, sd, True, False, object_size=osz, n_heads=heads, n_layers=layers))


def test_encode_cells_on_arrays_sliced_at_an_odd_object(enc_eng):
    """Per-object arrays as ``arr[3:]`` of a larger batch: rgb / center start 36 bytes, n_pts / class_idx / color_idx 12 bytes into their
    buffers (element-wide loads), pn_feat 3 KiB (rows of 1 KiB keep its float4 alignment): DESIGN.md, alignment contract."""
    sd = synth.make_object_branch_weights(3)
    cells = cells_with_counts((1, 29, 40), seed=13)
    enc_eng.load_weights(sd, class_embed=False, color_embed=False)
    skew = {"rgb": 36, "center": 36, "n_pts": 12, "class_idx": 12, "color_idx": 12, "pn_feat": 3 * 1024, "offsets": 4}
    encode_case(enc_eng, cells, O.encode_cells(cells, sd, False, False), skew=skew)


# ------------------------------------------------------------------------------------------------------------------ text head
@pytest.fixture(scope="module")
def head_eng():
    e = engine()
    e._sd = synth.make_language_head_weights(3)
    e.text_head_load_weights(e._sd)
    yield e
    e.close()


@pytest.mark.parametrize("n_sent,L", [(1, 1), (7, 16), (2, 17), (33, 32)])
def test_text_head(head_eng, n_sent, L):
    """(tests/test_gpu_text.py: 2e-5 of the output scale, flag clear)"""
    from tests.test_gpu_text import _first_half_oracle

    hidden = synth.make_t5_hidden(n_sent, L, seed=n_sent * 100 + L)
    plain, runs = run_guarded(lambda a: head_eng.text_head(a["hidden"], check=False), {"hidden": dev(hidden)}, 2)
    ref = _first_half_oracle(hidden, head_eng._sd)
    assert all(int(r[1].item()) == 0 for r in [plain] + runs)
    assert np.abs(plain[0].cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n_desc,S", [(1, 1), (7, 5), (2, 17)])
def test_text_inter(head_eng, n_desc, S):
    from tests.test_gpu_text import _inter_oracle

    sent = np.random.default_rng(n_desc * 100 + S).standard_normal((n_desc * S, 256)).astype(np.float32)
    plain, runs = run_guarded(lambda a: head_eng.text_inter(a["sent"], n_desc, check=False), {"sent": dev(sent)}, 2)
    ref = _inter_oracle(sent, head_eng._sd, n_desc)
    assert all(int(r[1].item()) == 0 for r in [plain] + runs)
    assert np.abs(plain[0].cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------------------------ fine stage
@pytest.fixture(scope="module", params=[0, 1], ids=["split-f16", "f32"])
def fine_eng(request):
    e = engine(encoder_f32=request.param)
    e._sd = synth.make_fine_weights(3)
    e.fine_load_weights(e._sd, class_embed=True, color_embed=True)
    yield e
    e.close()


@pytest.mark.parametrize("n_pairs", [1, 5])
def test_fine_encode_objects_and_match(fine_eng, n_pairs):
    """1 and 5 pairs (the last four-pair workgroup partly empty), 1, 6 and 8 hints, pairs by position and by index
    (tests/test_gpu_fine.py: descriptors to 5e-6, offsets to 5e-5)."""
    sd = fine_eng._sd
    cells = synth.make_cells(n_pairs, seed=2, min_obj=16, max_obj=16)
    keys = ("offsets", "class_idx", "color_idx", "rgb", "center", "n_pts")
    plain, _ = run_guarded(lambda a: (fine_eng.fine_encode_objects(a),), {k: dev(cells[k]) for k in keys}, 1, ints=cell_int_fills(cells))
    ref_desc = OF.fine_object_encodings(cells, sd, True, True)
    assert np.abs(plain[0].cpu().numpy() - ref_desc).max() < 5e-6
    desc = plain[0]
    rng = np.random.default_rng(n_pairs)
    for n_hints in (1, 6, 8):
        hints = rng.standard_normal((n_pairs, n_hints, 128)).astype(np.float32)
        plain, _ = run_guarded(lambda a: (fine_eng.fine_match(a["desc"], a["hints"]),), {"desc": desc, "hints": dev(hints)}, 1)
        assert np.abs(plain[0].cpu().numpy() - OF.cross_match(ref_desc, hints, sd)).max() < 5e-5
        ci = rng.integers(0, n_pairs, size=n_pairs + 2).astype(np.int32)
        hi = rng.integers(0, n_pairs, size=n_pairs + 2).astype(np.int32)
        ints = {"ci": other_than(0, max(n_pairs - 1, 0), ci[0], ci[-1]) if n_pairs > 1 else 0,
                "hi": other_than(0, max(n_pairs - 1, 0), hi[0], hi[-1]) if n_pairs > 1 else 0}
        plain, _ = run_guarded(lambda a: (fine_eng.fine_match(a["desc"], a["hints"], a["ci"], a["hi"]),),
                               {"desc": desc, "hints": dev(hints), "ci": dev(ci), "hi": dev(hi)}, 1, ints=ints)
        assert np.abs(plain[0].cpu().numpy() - OF.cross_match(ref_desc[ci], hints[hi], sd)).max() < 5e-5


# ------------------------------------------------------------------------------------------------------------------ contrastive loss
@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "forward"])
@pytest.mark.parametrize("B", [1, 31, 33, 100, 129, 200])
def test_contrastive_loss(plain_eng, B, need_grad):
    """(tests/test_gpu_loss.py: 3e-5 relative on the loss, 3e-6 absolute on the gradients; no atomics in loss.hip)"""
    rng = np.random.default_rng(B)
    a = rng.standard_normal((B, 256)).astype(np.float32)
    p = (a + 0.8 * rng.standard_normal((B, 256))).astype(np.float32)

    def call(x):
        out = plain_eng.contrastive_loss(x["a"], x["p"], 0.1, need_grad=need_grad)
        return tuple(t for t in out if t is not None)

    plain, _ = run_guarded(call, {"a": dev(a), "p": dev(p)}, 3 if need_grad else 1)
    rl, rga, rgp = O.contrastive_loss(a, p, 0.1, dtype=np.float64)
    assert abs(float(plain[0].item()) - rl) < 3e-5 * max(1.0, abs(rl))
    if need_grad:
        assert np.abs(plain[1].cpu().numpy() - rga).max() < 3e-6 and np.abs(plain[2].cpu().numpy() - rgp).max() < 3e-6


# ------------------------------------------------------------------------------------------------------------------ training steps
# Per-call tensors only (bound parameter and gradient storage is out of scope); every run re-binds, so that running statistics and
# accumulated gradients start alike. Float atomics: the oracle bar of each entry point's own file is asserted for ALL three runs.
def test_encode_cells_train_and_backward():
    """tests/test_gpu_train.py: test_forward_backward_match_the_float64_oracle at (5 cells, 3..33 objects), PointNet mode, p = 0.1."""
    from oracle import t2l_oracle_train as OT
    from tests.test_gpu_train import bind

    n_cells, seed = 5, 0xC0FFEE + 5
    cells = synth.make_cells(n_cells, seed=21 + n_cells, with_pn_feat=True, min_obj=3, max_obj=33)
    sd = synth.make_object_branch_weights(3)
    gout = np.random.default_rng(n_cells).standard_normal((n_cells, 256)).astype(np.float32) * 0.05
    ref_out, info = OT.encode_cells_train(cells, sd, False, False, grad_out=gout, p_drop=float(np.float32(0.1)), seed=seed)
    exp = info["grad_pn_feat"]
    rms = np.sqrt((exp ** 2).mean())
    e = engine()
    try:
        def call(a):
            bind(e, sd, False)
            out = e.encode_cells_train({k: a[k] for k in ("offsets",) + OBJ_KEYS}, dropout_p=0.1, seed=seed)
            e.encode_cells_backward(a["grad_emb"], a["grad_pn_feat"])
            return out, a["grad_pn_feat"]

        args = {k: dev(cells[k]) for k in ("offsets",) + OBJ_KEYS}
        args.update(grad_emb=dev(gout), grad_pn_feat=torch.zeros((int(cells["offsets"][-1]), 256), device="cuda"))
        plain, runs = run_guarded(call, args, 1, ints=cell_int_fills(cells), exact=False)
        for out, gpn in [plain] + runs:
            assert np.abs(out.cpu().numpy() - ref_out).max() < 2e-5
            err = np.abs(gpn.cpu().numpy() - exp)
            assert np.median(err) < 2e-3 * rms + 1e-9 and np.quantile(err, 0.9) < 2e-2 * rms + 1e-8
    finally:
        e.close()


def test_text_head_train_and_backward():
    """tests/test_gpu_text_train.py: test_engine_text_train_matches_the_float64_oracle at (9 descriptions, 1 sentence, 1 token), split-bf16."""
    from oracle import t2l_oracle_text_train as OTT
    from tests.test_gpu_text_train import _bind

    n_desc, S, L, p, seed = 9, 1, 1, 0.1, 1235
    sd = synth.make_language_head_weights(6)
    hidden = synth.make_t5_hidden(n_desc * S, L, seed=n_desc * 10 + L)
    gout = np.random.default_rng(L).standard_normal((n_desc, 256)).astype(np.float32)
    ref, _ = OTT.text_head_train(hidden, sd, n_desc, grad_out=gout, p_drop=float(np.float32(p)), seed=seed)
    e = engine()
    try:
        def call(a):
            _bind(e, sd)
            out = e.text_head_train(a["hidden"], n_desc, dropout_p=p, seed=seed)
            e.text_head_backward(a["grad_out"])
            return (out,)

        plain, runs = run_guarded(call, {"hidden": dev(hidden), "grad_out": dev(gout)}, 1, exact=False)
        for (out,) in [plain] + runs:
            assert np.abs(out.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    finally:
        e.close()


def test_pointnet_features_train_and_backward():
    """tests/test_gpu_pointnet_train.py: test_pointnet_train_forward_backward_match_the_float64_oracle at (2 cells of 2 objects)."""
    from oracle import t2l_oracle_pointnet_train as OPT
    from tests.test_gpu_pointnet_train import bind_all

    cells = synth.make_cells(2, seed=5, min_obj=2, max_obj=2)
    pos, rgb = synth.make_sampled_points(cells, 3)
    sd_pn, sd_obj = synth.make_pointnet_weights(1), synth.make_object_branch_weights(2)
    offs = np.asarray(cells["offsets"], dtype=np.int32)
    R = np.random.default_rng(0).standard_normal((pos.shape[0], 256))
    f2_ref, _ = OPT.forward_backward(pos, rgb, offs, sd_pn, grad_f2=R, pyg_self_loops=True)
    e = engine()
    try:
        def call(a):
            bind_all(e, sd_obj, sd_pn)
            f2 = e.pointnet_features_train(a["pos"], a["rgb"], offs)
            e.pointnet_backward(a["grad_f2"])
            return (f2,)

        plain, runs = run_guarded(call, {"pos": dev(pos), "rgb": dev(rgb), "grad_f2": dev(R.astype(np.float32))}, 1, exact=False)
        for (f2,) in [plain] + runs:
            assert np.abs(f2.cpu().numpy().astype(np.float64) - f2_ref).max() < 2e-4 * np.abs(f2_ref).max()
    finally:
        e.close()


def test_fine_train_forward_and_backward():
    """tests/test_gpu_fine_train.py: GRID's (5 pairs, 6 hints, 1 layer, PointNet mode) — its smallest case with a features2 gradient —
    without dropout, against the float64 twin: offsets to 1e-4, the two returned gradients to 2e-3 of their rms."""
    from tests.fine_train_twin import Twin
    from tests.test_gpu_fine_train import ALL, bind, rel
    from tests.test_oracle_fine_train import problem

    B, H, L = 5, 6, 1
    sd, cells, hints, pn, gout = problem(False, L, P=B, H=H, seed=B + H, use=ALL)
    off_t, _, gh_t, gp_t = Twin(sd, False, False, ALL, L).step(cells, hints, gout, pn)
    e = engine()
    try:
        def call(a):
            bind(e, sd, False, ALL, L)
            off = e.fine_train_forward({k: v for k, v in a.items() if k in cells and k != "counts"}, a["pn"], a["hints"], dropout_p=0.0, seed=0)
            e.fine_train_backward(a["gout"], a["gh"], a["gp"])
            return off, a["gh"], a["gp"]

        args = {k: dev(v) for k, v in cells.items() if k != "counts"}
        args.update(pn=dev(pn), hints=dev(hints), gout=dev(gout), gh=torch.zeros(hints.shape, device="cuda"), gp=torch.zeros(pn.shape, device="cuda"))
        plain, runs = run_guarded(call, args, 1, ints=cell_int_fills(cells), exact=False)
        for off, gh, gp in [plain] + runs:
            assert np.abs(off.cpu().numpy() - off_t).max() < 1e-4
            assert rel(gh.cpu().numpy(), gh_t) < 2e-3 and rel(gp.cpu().numpy(), gp_t) < 2e-3
    finally:
        e.close()
