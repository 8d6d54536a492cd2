"""GPU tier: t2l_text_inter at the compiled shapes other than the published (256, 4 heads) — (128, 4) = what --coarse_embed_dim 128
builds, (128, 2), (256, 8) — from the kernel up to LanguageEncoder.head, the sentence cache and the search behind it.
The references: the float32 numpy restatement (oracle/t2l_oracle.py: encoder_layer) for the engine call, the reference's own goldens
(tools/gen_golden_text_shapes.py) and the PyTorch modules for the module."""
import os.path as osp

import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from text2loc_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
SHAPES = [(128, 4), (128, 2), (256, 8)]
SHAPE_IDS = ["d128_h4", "d128_h2", "d256_h8"]
W_SEED = 3
COMPILED_MSG = "width 128 with 2 or 4 heads or 256 with 4 or 8 heads"


def inter_oracle(sent, sd, n_desc, D, heads):
    """x = sent.view(B, S, D).permute(1, 0, 2); x += inter_module[0](x); max over the sentences (tests/test_gpu_text.py: _inter_oracle)."""
    x = np.ascontiguousarray(sent.reshape(n_desc, -1, D).transpose(1, 0, 2))
    x = x + O.encoder_layer(np.ascontiguousarray(x), sd, "language_encoder.inter_module.0", heads)
    return x.max(axis=0)


_SD = {}


def head_sd(D):
    if D not in _SD:
        _SD[D] = synth.make_language_head_weights(W_SEED, embed_dim=D)
    return _SD[D]


@pytest.fixture(scope="module", params=SHAPES, ids=SHAPE_IDS)
def shaped(request):
    from text2loc_amd.engine import Engine

    D, heads = request.param
    e = Engine(0)
    e.text_head_load_weights(head_sd(D), inter_num_heads=heads)
    e._sd, e._D, e._heads = head_sd(D), D, heads
    yield e
    e.close()


# (n_desc, S): a single row; dead rows in a tile (5, 6, 11, 17); a half-filled second tile (13 x 6 = 2 tiles of 5 + 3 descriptions);
# one description per tile (17, 32); a full tile with no dead row (32); an odd tile count (33 x 11: 17 tiles); 300 x 6 = 30 workgroups:
# fewer than the 256 CUs, so no shape here runs a second round of workgroups on a CU (nor is it made to: the tiling has no state
# that a second round could meet).
CASES = [(1, 1), (7, 5), (13, 6), (2, 17), (3, 32), (33, 11), (300, 6)]


@pytest.mark.parametrize("n_desc,S", CASES)
def test_text_inter_matches_the_restatement(shaped, n_desc, S):
    D, heads = shaped._D, shaped._heads
    sent = np.random.default_rng(n_desc * 100 + S).standard_normal((n_desc * S, D)).astype(np.float32)
    out, bad = shaped.text_inter(torch.from_numpy(sent).cuda(), n_desc)
    ref = inter_oracle(sent, shaped._sd, n_desc, D, heads)
    assert not bad and out.shape == ref.shape == (n_desc, D)
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"({D}, {heads}) n_desc {n_desc} S {S}: err {err:.2e}, |ref|max {np.abs(ref).max():.2f}")
    assert err < 2e-5 * max(1.0, np.abs(ref).max()), err


def test_plain_f16_flag_and_argument_checks(shaped):
    from text2loc_amd.engine import T2LError

    D, heads = shaped._D, shaped._heads
    sent = np.random.default_rng(4).standard_normal((60, D)).astype(np.float32)
    ref = inter_oracle(sent, shaped._sd, 10, D, heads)
    scale = max(1.0, np.abs(ref).max())
    split, bad = shaped.text_inter(torch.from_numpy(sent).cuda(), 10)
    assert not bad
    shaped.set_option("encoder_f16", 1)
    try:
        fast, bad = shaped.text_inter(torch.from_numpy(sent).cuda(), 10)
    finally:
        shaped.set_option("encoder_f16", 0)
    e16 = np.abs(fast.cpu().numpy() - ref).max()
    print(f"({D}, {heads}) plain f16 err {e16:.2e}, scale {scale:.2f}")
    assert not bad and 1e-6 < e16 < 1e-3 * scale, e16
    assert not torch.equal(fast, split)
    for poison in (5.0e4, np.nan):
        hot = sent.copy()
        hot[7, 3] = poison
        _, bad = shaped.text_inter(torch.from_numpy(hot).cuda(), 10)
        assert bad
        again, bad = shaped.text_inter(torch.from_numpy(sent).cuda(), 10)  # the flag is per call
        assert not bad and torch.equal(again, split)
    with pytest.raises(T2LError):
        shaped.text_inter(torch.from_numpy(sent[:59]).cuda(), 10)  # rows do not split over the descriptions
    with pytest.raises(T2LError, match=f"{D} wide"):
        shaped.text_inter(torch.zeros((60, 384 - D), device="cuda"), 10)  # the other compiled width


def test_a_description_does_not_depend_on_its_batch(shaped):
    """What tools/text_inter_probe.py probes and encode_text_batches relies on: a description's output is bit-identical whether it is
    computed alone, in a prefix of the batch or in the full batch of 96 x 6 — wherever its rows sit at the same place of a 32-row tile
    (S = 6: five descriptions per tile, so description d sits at place d % 5). The key sums of the softmax and of P V group their
    terms by tile row, so a description MOVED to another place of a tile agrees to rounding only — at every width, the published one
    included (tests/test_gpu_e2e.py: "<= 2e-6 from the inter-sentence kernel's tile placement" on unit embeddings); here that case is
    held to the restatement's bound, 2e-5 of the output scale, and printed."""
    D = shaped._D
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((96 * 6, D)).astype(np.float32)).cuda()
    full, _ = shaped.text_inter(x, 96, check=False)
    for n in (1, 7, 10, 11):
        part, _ = shaped.text_inter(x[: n * 6].contiguous(), n, check=False)
        assert torch.equal(part, full[:n]), n
    for d in (0, 5, 15, 95):  # alone, from the second tile of a workgroup and from later workgroups: place 0 of a tile in both runs
        alone, _ = shaped.text_inter(x[d * 6: d * 6 + 6].contiguous(), 1, check=False)
        assert torch.equal(alone[0], full[d]), d
    for lo, hi in ((5, 16), (10, 17), (85, 96)):  # slices that start on a tile: every description keeps its place
        part, _ = shaped.text_inter(x[lo * 6: hi * 6].contiguous(), hi - lo, check=False)
        assert torch.equal(part, full[lo:hi]), (lo, hi)
    scale = max(1.0, float(full.abs().max()))
    part, _ = shaped.text_inter(x[7 * 6: 14 * 6].contiguous(), 7, check=False)  # moved places: 2 -> 0, 3 -> 1, ...
    alone, _ = shaped.text_inter(x[17 * 6: 18 * 6].contiguous(), 1, check=False)
    moved = max(float((part - full[7:14]).abs().max()), float((alone[0] - full[17]).abs().max()))
    print(f"D {D}: moved within the tile: {moved:.2e} (scale {scale:.2f})")
    assert moved < 2e-5 * scale


# ---- through the product: LanguageEncoder.head ---------------------------------------------------------------------------------
def _encoder(D, heads, weight_seed, layers=1):
    from text2loc_amd.cell_retrieval import LanguageEncoder

    enc = LanguageEncoder(D, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=layers, inter_module_num_heads=heads,
                          llm_model=object(), tokenizer=None, input_dim=1024)
    sd = {k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(weight_seed, embed_dim=D).items()}
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("inter_module.1.") for k in missing), (missing, unexpected)
    return enc.to("cuda").eval()


@pytest.mark.parametrize("D,heads", SHAPES, ids=SHAPE_IDS)
def test_the_references_golden_through_the_language_encoder(golden, D, heads):
    """The reference's encode_text at (D, heads) to 2e-5 with BOTH halves of the head in the engine; then the overflow fallback, the
    deferred mode and a weight update."""
    from text2loc_amd.cell_retrieval import LanguageEncoder as LE

    g = golden(f"text_head_d{D}_h{heads}")
    B, L = int(g["batch"]), int(g["n_tokens"])
    hidden = torch.from_numpy(synth.make_t5_hidden(6 * B, L, seed=int(g["hidden_seed"]))).cuda()
    enc = _encoder(D, heads, int(g["weight_seed"]))
    n0, i0, t0 = LE.head_engine_calls, LE.inter_engine_calls, LE.inter_torch_calls
    with torch.no_grad():
        out = torch.nn.functional.normalize(enc.head(hidden, B))
    assert LE.head_engine_calls == n0 + 1 and LE.inter_engine_calls == i0 + 1
    assert LE.inter_torch_calls == t0
    err = np.abs(out.cpu().numpy() - g["text_embeddings"]).max()
    print(f"({D}, {heads}) head vs the reference's golden: {err:.2e}")
    assert err < 2e-5
    # an overflowing batch (its first half overflows) runs on the PyTorch modules, bit for bit
    big = hidden.clone()
    big[0, 0, 0] = 5.0e4
    with torch.no_grad():
        a = enc.head(big, B)
        enc.use_engine_head = False
        b = enc.head(big, B)
        enc.use_engine_head = True
    assert torch.equal(a, b)
    # one whose first half is fine and whose inter layer overflows: the second half alone falls back, bit for bit
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((6 * B, D)).astype(np.float32)).cuda()
    x[7, 3] = 5.0e4
    i1, t1 = LE.inter_engine_calls, LE.inter_torch_calls
    with torch.no_grad():
        a = enc._head_second_half(x, B, True)
        b = enc._head_second_half(x, B, False)
    assert LE.inter_engine_calls == i1 and LE.inter_torch_calls == t1 + 2 and torch.equal(a, b)
    # deferred mode names the ordinal
    enc.begin_deferred()
    with torch.no_grad():
        a = enc.head(hidden, B)
        b = enc.head(big, B)
        c = enc.head(hidden, B)
    assert enc.end_deferred() == [1]
    assert torch.isnan(b).all() and torch.equal(a, c) and not torch.isnan(a).any()
    assert enc.end_deferred() == []
    # a weight update re-packs
    with torch.no_grad():
        enc.inter_module[0].linear1.bias.add_(0.25)
        i2 = LE.inter_engine_calls
        new = enc.head(hidden, B)
        assert LE.inter_engine_calls == i2 + 1
        enc.use_engine_head = False
        new_t = enc.head(hidden, B)
        enc.use_engine_head = True
    assert float((new - a).abs().max()) > 1e-3
    assert float((new - new_t).abs().max()) < 5e-5


@pytest.mark.parametrize("D,heads,layers", [(128, 8, 1), (128, 4, 2)], ids=["d128_h8", "two_layers"])
def test_unsupported_shapes_stay_on_the_pytorch_modules(D, heads, layers):
    from text2loc_amd.cell_retrieval import LanguageEncoder as LE
    from text2loc_amd.engine import Engine, T2LError

    B = 4
    enc = _encoder(D, heads, 1, layers=layers)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((6 * B, D)).astype(np.float32)).cuda()
    i0, t0 = LE.inter_engine_calls, LE.inter_torch_calls
    with torch.no_grad():
        a = enc._head_second_half(x, B, True)
        assert LE.inter_engine_calls == i0 and LE.inter_torch_calls == t0 + 1
        enc.use_engine_head = False
        b = enc._head_second_half(x, B, False)
        enc.use_engine_head = True
        assert torch.equal(a, b)
        hidden = torch.from_numpy(synth.make_t5_hidden(6 * B, 9, seed=4)).cuda()
        n0, t1 = LE.head_engine_calls, LE.inter_torch_calls
        enc.head(hidden, B)  # the first half in the engine, the inter half on the modules: nothing raises
        assert LE.head_engine_calls == n0 + 1 and LE.inter_torch_calls == t1 + 1 and LE.inter_engine_calls == i0
    e = Engine(0)
    try:
        sd = {"language_encoder." + k: v for k, v in enc.state_dict().items() if not k.endswith("num_batches_tracked")}
        e.text_head_load_weights(sd, inter_num_heads=heads)  # the load does not fail ...
        with pytest.raises(T2LError, match=COMPILED_MSG):  # ... the call names the compiled set
            e.text_inter(x, B)
    finally:
        e.close()


# ---- behind the sentence cache, and into the search ---------------------------------------------------------------------------
def test_text_cache_at_d128():
    """tests/test_gpu_text_cache.py at --coarse_embed_dim 128: encode_text with the cache (gather + t2l_text_inter with the memo)
    equals the uncached run to 2e-5 on k360_tiny's descriptions."""
    from tests.test_gpu_text_cache import _tiny_t5
    from tests.test_gpu_train_loop import _args
    from text2loc_amd import kitti360pose as K
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork, LanguageEncoder
    from text2loc_amd.text_cache import TextCache

    g = np.load(osp.join(GOLDEN, "k360_tiny.npz"), allow_pickle=False)
    ds = K.Kitti360PoseDataset(osp.join(GOLDEN, "k360_tiny"), [str(s) for s in g["scenes"]])
    sentences = TextCache.sentences_of(ds)
    tok, t5 = _tiny_t5(sentences)
    le = LanguageEncoder(128, fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4, inter_module_num_layers=1,
                         inter_module_num_heads=4, llm_model=t5, tokenizer=tok)
    model = CellRetrievalNetwork(ds.get_known_classes(), synth.COLOR_NAMES, _args(coarse_embed_dim=128, batch_size=5), language_encoder=le)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_object_branch_weights(4, embed_dim=128).items()}
    sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_language_head_weights(2, embed_dim=128).items()})
    model.load_state_dict(sd, strict=False)
    model = model.to("cuda").eval()
    dl = torch.utils.data.DataLoader(ds, batch_size=5, collate_fn=K.Kitti360PoseDataset.collate_fn, shuffle=False)
    texts = next(iter(dl))["texts"]
    i0, t0 = LanguageEncoder.inter_engine_calls, LanguageEncoder.inter_torch_calls
    with torch.no_grad():
        plain = model.encode_text(texts)
    assert plain.shape == (len(texts), 128) and LanguageEncoder.inter_engine_calls == i0 + 1
    le.text_cache = TextCache.build(le, ds)
    for memo in (True, False):
        le.memoise_sentence_vectors = memo
        t5_0, c_0, i1 = LanguageEncoder.t5_calls, LanguageEncoder.cache_calls, LanguageEncoder.inter_engine_calls
        with torch.no_grad():
            cached = model.encode_text(texts)
        assert LanguageEncoder.t5_calls == t5_0 and LanguageEncoder.cache_calls == c_0 + 1
        assert LanguageEncoder.inter_engine_calls == i1 + 1
        assert float((cached - plain).abs().max()) < 2e-5
    assert LanguageEncoder.inter_torch_calls == t0


def test_queries_at_d128_feed_the_search_unchanged(golden):
    """LanguageEncoder(128).head -> t2l_search over a 1,000-row 128-wide database on the device: the ids are the float64 ranking of
    exactly those embeddings (tests/test_gpu_text.py: test_text_head_feeds_the_search_unchanged)."""
    from oracle import c_oracle
    from text2loc_amd.cell_retrieval import LanguageEncoder as LE
    from text2loc_amd.engine import Engine

    g = golden("text_head_d128_h4")
    B, L = int(g["batch"]), int(g["n_tokens"])
    hidden = torch.from_numpy(synth.make_t5_hidden(6 * B, L, seed=int(g["hidden_seed"]))).cuda()
    enc = _encoder(128, 4, int(g["weight_seed"]))
    i0 = LE.inter_engine_calls
    with torch.no_grad():
        q = torch.nn.functional.normalize(enc.head(hidden, B)).contiguous()
    assert LE.inter_engine_calls == i0 + 1 and q.shape == (B, 128)
    db, _, _ = synth.make_retrieval_problem(1000, 4, dim=128, seed=2, noise=1.0)
    eng = Engine(0)
    try:
        eng.db_set(torch.from_numpy(db).cuda())
        idx, sc = eng.search(q, 5)
        ridx, rsc = c_oracle.retrieve_topk(db, q.cpu().numpy(), 5)
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx) and np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
    finally:
        eng.close()
