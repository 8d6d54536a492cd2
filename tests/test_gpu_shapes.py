"""GPU tier: the cell encoder at the compiled shapes other than the published one (coarse_embed_dim 128 / 256, head_dim 32 / 64,
object_size 1..32, 1..4 layers) through the C ABI and through the Python surface, against the reference goldens of
tools/gen_golden_shapes.py and the numpy oracle. TOL is test_gpu_encoder.py's bar for this kernel family."""
import argparse

import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from text2loc_amd import synth
from tests.test_host_logic import StubCell, StubPose, make_objects
from tests.test_oracle_shapes import ENCODER_GOLDENS, golden_cases, golden_cells, golden_shape

pytestmark = pytest.mark.gpu
TOL = 2e-5
OBJ_KEYS = ("class_idx", "color_idx", "rgb", "center", "n_pts", "pn_feat")
TRAIN_MSG = "published shape only"


def to_gpu(cells):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}


def take(cells, n_cells=None, n_objects=None):
    """First n_cells cells, or one cell made of the first n_objects objects."""
    out = {}
    if n_objects is not None:
        out["counts"] = np.array([n_objects], dtype=np.int32)
        out["offsets"] = np.array([0, n_objects], dtype=np.int32)
        hi = n_objects
    else:
        out["counts"] = cells["counts"][:n_cells]
        out["offsets"] = cells["offsets"][: n_cells + 1]
        hi = int(cells["offsets"][n_cells])
    for k in OBJ_KEYS:
        if k in cells:
            out[k] = cells[k][:hi]
    return out


@pytest.fixture(scope="module", params=[(0, 1), (0, 0), (1, 0)], ids=["split-f16-two-cells", "split-f16-one-cell", "f32"])
def eng(request):
    """The three engine settings of test_gpu_encoder.py. encoder_two_cells acts on the published shape only: at the other shapes
    the first two settings run the same split-f16 instance, the third the all-f32 one."""
    from text2loc_amd.engine import Engine

    e = Engine(0)
    e.set_option("encoder_f32", request.param[0])
    e.set_option("encoder_two_cells", request.param[1])
    e.encoder_f32 = request.param[0]
    yield e
    e.close()


def load(eng, sd, embed, D, heads, layers, osz, color_embed=None, **kw):
    eng.load_weights(sd, class_embed=embed, color_embed=embed if color_embed is None else color_embed, num_layers=layers,
                     num_heads=heads, embed_dim=D, object_size=osz, **kw)


@pytest.mark.parametrize("name", ENCODER_GOLDENS)
def test_shape_goldens(eng, golden, name):
    g = golden(name)
    D, heads, layers, osz = golden_shape(g)
    sd = synth.make_object_branch_weights(int(g["weight_seed"]), embed_dim=D, num_layers=layers)
    for mode, sfx in golden_cases(g):
        embed = mode == "embed"
        load(eng, sd, embed, D, heads, layers, osz)
        assert eng.embed_dim == D
        out = eng.encode_cells(to_gpu(golden_cells(g, with_pn=not embed))).cpu().numpy()
        assert out.shape == (int(g["n_cells"]), D)
        err = np.abs(out - g["cell_embeddings" + sfx]).max()
        print(f"{name} {mode}: max err {err:.2e}")
        assert err < TOL, err
        assert np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-5


SHAPES = [(128, 4, 2, 28), (128, 2, 2, 32), (256, 8, 2, 32), (128, 4, 3, 32)]


@pytest.mark.parametrize("D,heads,layers,osz", SHAPES[:3])
@pytest.mark.parametrize("mode", ["embed", "pn", "mixed"])
@pytest.mark.parametrize("feats", [("class", "color", "position", "num"), ("class", "position"), ("num",)])
def test_feature_subsets_vs_oracle(eng, mode, feats, D, heads, layers, osz):
    ce, co = {"embed": (True, True), "pn": (False, False), "mixed": (True, False)}[mode]
    sd = synth.make_object_branch_weights(3, use_features=feats, embed_dim=D, num_layers=layers)
    cells = synth.make_cells(25, seed=12, min_obj=1, max_obj=40, with_pn_feat=True)
    ref = O.encode_cells(cells, sd, ce, co, object_size=osz, n_heads=heads, n_layers=layers, use_features=feats)
    load(eng, sd, ce, D, heads, layers, osz, color_embed=co, use_features=feats)
    out = eng.encode_cells(to_gpu(cells)).cpu().numpy()
    assert out.shape == ref.shape == (25, D)
    assert np.abs(out - ref).max() < TOL


@pytest.mark.parametrize("D,heads,layers,osz", SHAPES)
def test_counts_edge_cases(eng, D, heads, layers, osz):
    """1 object, exactly object_size, object_size + 1 (first truncation), 60 objects; unit rows; truncation beyond object_size."""
    sd = synth.make_object_branch_weights(0, embed_dim=D, num_layers=layers)
    load(eng, sd, True, D, heads, layers, osz)
    big = synth.make_cells(1, seed=2, min_obj=60, max_obj=60)
    for n in (1, osz, osz + 1, 60):
        cells = take(big, n_objects=n)
        ref = O.encode_cells(cells, sd, True, True, object_size=osz, n_heads=heads, n_layers=layers)
        out = eng.encode_cells(to_gpu(cells)).cpu().numpy()
        assert np.abs(out - ref).max() < TOL
        assert abs(np.linalg.norm(out[0]) - 1.0) < 1e-5
    a = eng.encode_cells(to_gpu(take(big, n_objects=osz))).cpu().numpy()
    b = eng.encode_cells(to_gpu(take(big, n_objects=45))).cpu().numpy()
    assert np.array_equal(a, b)
    if osz < 32:  # a slot below object_size is a real (zero) token, a row at or above it is dead: the two cut-offs differ
        load(eng, sd, True, D, heads, layers, osz + 1)
        c = eng.encode_cells(to_gpu(take(big, n_objects=osz))).cpu().numpy()
        assert np.abs(c - a).max() > 1e-4


def test_full_size_batch_d128(eng):
    """11,259 cells in one launch at D = 128: unit norms; a sample equals the oracle (batch independence)."""
    sd = synth.make_object_branch_weights(0, embed_dim=128)
    load(eng, sd, True, 128, 4, 2, 28)
    cells = synth.make_cells(11259, seed=4)
    out = eng.encode_cells(to_gpu(cells)).cpu().numpy()
    assert out.shape == (11259, 128)
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-5
    ref = O.encode_cells(take(cells, n_cells=40), sd, True, True)
    assert np.abs(out[:40] - ref).max() < TOL


def test_shapes_interleave_on_one_context_and_side_by_side(eng, golden):
    from text2loc_amd.engine import Engine

    g128, g256 = golden("shapes_d128_h4"), golden("encoder_embed")
    sd128 = synth.make_object_branch_weights(int(g128["weight_seed"]), embed_dim=128)
    sd256 = synth.make_object_branch_weights(int(g256["weight_seed"]))
    c128, c256 = to_gpu(golden_cells(g128)), to_gpu(golden_cells(g256))
    load(eng, sd128, True, 128, 4, 2, 28)
    a = eng.encode_cells(c128).cpu().numpy()
    assert a.shape[1] == 128 and np.abs(a - g128["cell_embeddings"]).max() < TOL
    eng.load_weights(sd256, class_embed=True, color_embed=True)  # the published model, through the unchanged call
    assert eng.embed_dim == 256
    b = eng.encode_cells(c256).cpu().numpy()
    assert b.shape[1] == 256 and np.abs(b - g256["cell_embeddings"]).max() < TOL
    other = Engine(0)
    other.set_option("encoder_f32", eng.encoder_f32)  # the same instance as `eng`: equal bit for bit
    try:
        load(other, sd128, True, 128, 4, 2, 28)
        a2 = other.encode_cells(c128).cpu().numpy()
        b2 = eng.encode_cells(c256).cpu().numpy()
        assert other.embed_dim == 128 and eng.embed_dim == 256
        assert np.array_equal(a2, a) and np.array_equal(b2, b)
    finally:
        other.close()


@pytest.mark.parametrize("f32", [0, 1], ids=["split-f16", "f32"])
def test_published_one_cell_is_the_shaped_instance(f32):
    """The published shape with encoder_two_cells = 0 runs the <256, 64> instance of the one-cell kernel with object_size 28, the
    instance the same state_dict gets when the shape is spelled out: equal bits on cells of 0, 1, 27, 28 and 29 objects."""
    from text2loc_amd.engine import Engine

    sd = synth.make_object_branch_weights(0)
    src = synth.make_cells(1, seed=2, min_obj=86, max_obj=86)
    counts = np.array([0, 1, 27, 28, 29], dtype=np.int32)
    cells = {"counts": counts, "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}
    cells.update({k: src[k][: counts.sum()] for k in OBJ_KEYS if k in src})
    a, b = Engine(0), Engine(0)
    try:
        for e in (a, b):
            e.set_option("encoder_f32", f32)
            e.set_option("encoder_two_cells", 0)
        a.load_weights(sd, class_embed=True, color_embed=True)
        b.load_weights(sd, class_embed=True, color_embed=True, embed_dim=256, num_heads=4, object_size=28)
        out_a = a.encode_cells(to_gpu(cells)).cpu().numpy()
        out_b = b.encode_cells(to_gpu(cells)).cpu().numpy()
        assert out_a.shape == (5, 256) and np.isfinite(out_a).all()
        assert np.array_equal(out_a, out_b)
        assert np.abs(out_a - O.encode_cells(cells, sd, True, True)).max() < TOL
    finally:
        a.close()
        b.close()


def test_c_entry_point_refuses_what_is_not_compiled(eng):
    """T2L_EINVAL from t2l_load_weights_shaped itself (the binding's own check is bypassed), the message names the compiled set."""
    import ctypes as C

    from text2loc_amd.engine import T2LError, _ModelConfig, _ModelShape, _WeightDesc

    sd = synth.make_object_branch_weights(0, embed_dim=128)
    w = np.ascontiguousarray(sd["obj_inter_module.0.norm1.weight"], dtype=np.float32)
    descs = (_WeightDesc * 1)(_WeightDesc(b"obj_inter_module.0.norm1.weight", w.ctypes.data, w.size))
    for D, heads, osz in [(192, 4, 28), (256, 3, 28), (128, 4, 33), (128, 8, 28), (128, 4, 0), (64, 2, 28)]:
        cfg, shape = _ModelConfig(1, 1, 1, 1, 1, 1, 2, heads), _ModelShape(D, osz)
        assert eng.lib.t2l_load_weights_shaped(eng._h, descs, 1, C.byref(cfg), C.byref(shape)) == -1  # T2L_EINVAL
        msg = eng.lib.t2l_last_error(eng._h).decode()
        assert "compiled shapes" in msg and "head_dim 32 or 64" in msg and "object_size 1..32" in msg, msg
    cfg = _ModelConfig(1, 1, 1, 1, 1, 1, 2, 3)
    assert eng.lib.t2l_load_weights(eng._h, descs, 1, C.byref(cfg)) == -1  # the unchanged entry point: 4 or 8 heads at D = 256
    with pytest.raises(T2LError, match="wrong size|missing/odd"):  # a D = 128 checkpoint declared as D = 256
        eng.load_weights(sd, class_embed=True, color_embed=True, embed_dim=256)
    with pytest.raises(T2LError, match="wrong size"):
        eng.load_weights(sd, class_embed=False, color_embed=False, embed_dim=256)
    sd8 = synth.make_object_branch_weights(0)
    eng.load_weights(sd8, class_embed=True, color_embed=True, num_heads=8)  # t2l_load_weights' shape now takes 8 heads
    cells = synth.make_cells(6, seed=1)
    out = eng.encode_cells(to_gpu(cells)).cpu().numpy()
    assert np.abs(out - O.encode_cells(cells, sd8, True, True, n_heads=8)).max() < TOL


# ---- the Python surface at D = 128 -------------------------------------------------------------------------------------------------
class PresetText(torch.nn.Module):
    """Text branch stand-in: returns precomputed (golden) text embeddings; 'descriptions' are row indices."""

    def __init__(self, table):
        super().__init__()
        self.table = torch.nn.Parameter(torch.from_numpy(table), requires_grad=False)

    def forward(self, idx):
        return self.table[torch.as_tensor(idx, device=self.table.device)]

    @property
    def device(self):
        return self.table.device


def make_args(g, **kw):
    a = argparse.Namespace(coarse_embed_dim=int(g["embed_dim"]), object_size=int(g["object_size"]),
                           object_inter_module_num_heads=int(g["num_heads"]), object_inter_module_num_layers=int(g["num_layers"]),
                           hungging_model=None, fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4,
                           inter_module_num_layers=1, inter_module_num_heads=4, class_embed=True, color_embed=True,
                           use_features=["class", "color", "position", "num"], ranking_loss="contrastive",
                           top_k=[int(k) for k in g["top_k"]], threshs=[int(t) for t in g["threshs"]], batch_size=16)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def d128_model(g):
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    args = make_args(g)
    model = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=PresetText(g["text_encodings"]))
    sd = synth.make_object_branch_weights(int(g["weight_seed"]), embed_dim=int(g["embed_dim"]), num_layers=int(g["num_layers"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    objects = make_objects(synth.make_cells(int(g["n_cells"]), seed=int(g["cell_seed"])), int(g["cell_seed"]))
    cells = [StubCell(c, b, g["cell_size"]) for c, b in zip(g["db_cell_ids"], g["cell_bbox_w"])]
    return model.to("cuda").eval(), args, objects, cells


class CellDs:
    def __init__(self, cells, objects):
        self.cells, self.objects = cells, objects

    def __len__(self):
        return len(self.cells)

    def __getitem__(self, i):
        return {"cells": self.cells[i], "cell_ids": self.cells[i].id, "objects": self.objects[i], "object_points": None}


def test_run_coarse_at_d128_matches_the_reference_run(golden):
    """The pattern of test_gpu_pipeline.py::test_run_coarse_matches_the_reference_run at --coarse_embed_dim 128: cell encodings
    within 2e-6 of the reference's; for EVERY query the ids are the float64 ranking of the engine's own embeddings; the
    reference's ids for every query whose top-6 reference score gaps exceed 2 delta, delta from the measured row error; at least
    56 of the 64 queries decided that way (the reference's own gaps allow a worst row error of 6e-6 in the L2 norm)."""
    from oracle import c_oracle
    from text2loc_amd import packing
    from text2loc_amd.coarse import collate_fn, eval_epoch, run_coarse

    g = golden("retrieval_e2e_d128")
    model, args, objects, cells = d128_model(g)
    poses = [StubPose(c, p) for c, p in zip(g["query_cell_ids"], g["query_pose_w"])]

    class Ds:
        all_cells, all_poses = cells, poses

        def __len__(self):
            return len(poses)

        def __getitem__(self, i):
            return {"texts": i, "cell_ids": poses[i].cell_id}

        def get_cell_dataset(self):
            return CellDs(cells, objects)

    for objs in objects:  # the host packer: the reference's own arithmetic for the per-object means
        for o in objs:
            packing.object_features(o)
    dl = torch.utils.data.DataLoader(Ds(), batch_size=16, collate_fn=collate_fn, shuffle=False)
    acc, close, retr, ce, te = eval_epoch(model, dl, args, return_encodings=True)
    assert ce.shape == (64, 128) and te.shape == (64, 128)
    ref_ce = g["cell_encodings"].astype(np.float64)
    print("cell encodings: max element error", np.abs(ce - ref_ce).max())
    assert np.abs(ce - ref_ce).max() < 2e-6
    assert np.abs(te - g["text_encodings"].astype(np.float64)).max() < 1e-6
    ids = g["db_cell_ids"]
    k = max(args.top_k)
    ridx, _ = c_oracle.retrieve_topk(ce.astype(np.float32), te.astype(np.float32), k)
    for q in range(len(retr)):
        assert np.array_equal(retr[q], ids[ridx[q]])
    delta = np.linalg.norm(ce - ref_ce, axis=1).max() * np.linalg.norm(te, axis=1).max()
    full = np.sort(ref_ce @ te.T, axis=0)[::-1]
    decided = np.abs(np.diff(full[: k + 1], axis=0)).min(axis=0) > 2 * delta
    print("delta", delta, "decided", int(decided.sum()))
    assert decided.sum() >= 56, (decided.sum(), delta)
    for q in np.nonzero(decided)[0]:
        assert np.array_equal(retr[q], ids[g["top_rows"][q]])
    undecided = int((~decided).sum())
    assert np.abs(np.array([acc[kk] for kk in args.top_k]) - g["acc"]).max() <= undecided / 64 + 1e-12
    retrievals, at = run_coarse(model, dl, args)
    got = np.array([[at[kk][t] for t in args.threshs] for kk in args.top_k])
    assert np.abs(got - g["acc_thresh"]).max() <= undecided / 64 + 1e-12
    assert len(retrievals) == 64 and retrievals[0].dtype.kind == "U"


def test_cell_database_round_trip_at_d128(golden, tmp_path):
    from text2loc_amd.db import CellDatabase

    g = golden("retrieval_e2e_d128")
    model, args, objects, cells = d128_model(g)
    db = CellDatabase.build(model, CellDs(cells, objects), batch_size=20)
    assert len(db) == 64 and db.embeddings.shape == (64, 128)
    assert np.abs(db.embeddings - g["cell_encodings"]).max() < 1e-4
    t = torch.from_numpy(g["text_encodings"]).cuda()
    idx0, sc0 = db.search(model.engine(), t, 5)
    path = str(tmp_path / "cells_d128.t2ldb.npz")
    db.save(path)
    db2 = CellDatabase.load(path)
    assert np.array_equal(db2.cell_ids, db.cell_ids) and np.array_equal(db2.embeddings, db.embeddings)
    idx, sc = db2.search(model.engine(), t, 5)
    assert torch.equal(idx, idx0) and torch.equal(sc, sc0)
    ridx, rsc = O.retrieve_topk(db2.embeddings, g["text_encodings"], 5)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx) and np.abs(sc.cpu().numpy() - rsc).max() < 1e-12
    empty = CellDatabase.build(model, CellDs([], []), batch_size=20)
    assert empty.embeddings.shape == (0, 128)


def test_encode_cell_set_at_d128(golden):
    from text2loc_amd import packing

    g = golden("retrieval_e2e_d128")
    model, args, objects, cells = d128_model(g)
    cs = packing.PackedCellSet([argparse.Namespace(id=c.id, objects=o) for c, o in zip(cells, objects)])
    out = model.encode_cell_set(cs, chunk_cells=24)
    assert out.shape == (64, 128) and np.abs(out.cpu().numpy() - g["cell_encodings"]).max() < 1e-4


def test_language_encoder_at_d128_first_half_in_the_engine():
    """LanguageEncoder(128) in eval mode: t2l_text_head serves the first half (inter_mlp width 128 <= 256), the 128-wide inter layer
    runs on the PyTorch modules; equal to the same modules run entirely on PyTorch within 2e-5 on the normalised output."""
    from text2loc_amd.cell_retrieval import LanguageEncoder

    B, L = 12, 9
    enc = LanguageEncoder(128, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1, llm_model=object(),
                          tokenizer=None, input_dim=1024)
    sd = {k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(1, embed_dim=128).items()}
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    enc = enc.to("cuda").eval()
    hidden = torch.from_numpy(synth.make_t5_hidden(6 * B, L, seed=4)).cuda()
    n0, t0 = LanguageEncoder.head_engine_calls, LanguageEncoder.head_torch_calls
    with torch.no_grad():
        out = torch.nn.functional.normalize(enc.head(hidden, B))
    assert out.shape == (B, 128)
    assert LanguageEncoder.head_engine_calls == n0 + 1 and LanguageEncoder.head_torch_calls == t0
    enc.use_engine_head = False
    with torch.no_grad():
        out_t = torch.nn.functional.normalize(enc.head(hidden, B))
    enc.use_engine_head = True
    assert LanguageEncoder.head_torch_calls == t0 + 1
    assert float((out - out_t).abs().max()) < 2e-5


def test_training_is_refused_at_other_shapes_and_eval_keeps_working(golden):
    from text2loc_amd import optim
    from text2loc_amd.engine import Engine, T2LError

    g = golden("retrieval_e2e_d128")
    model, args, objects, cells = d128_model(g)
    before = model.encode_objects(objects[:5], [None] * 5).cpu().numpy()
    assert before.shape == (5, 128) and np.abs(before - g["cell_encodings"][:5]).max() < 1e-4
    model.train()
    with pytest.raises(T2LError, match=TRAIN_MSG):
        model.encode_objects(objects[:5], [None] * 5)
    with pytest.raises(T2LError, match=TRAIN_MSG):
        model.train_engine()
    with pytest.raises(T2LError, match=TRAIN_MSG):
        optim.Adam(model, lr=1e-3)
    with torch.no_grad():  # train mode without gradients is the eval path, as at the published shape
        assert model.encode_objects(objects[:5], [None] * 5).shape == (5, 128)
    e = Engine(0)
    try:
        tens = {}
        for k, v in synth.make_object_branch_weights(0, embed_dim=128).items():
            if k.endswith("num_batches_tracked") or ".color_encoder." in k or ".mlp_pointnet." in k or ".pointnet." in k:
                continue
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
        with pytest.raises(T2LError, match=TRAIN_MSG):
            e.train_bind(tens, class_embed=True, color_embed=True)
    finally:
        e.close()
    model.eval()
    after = model.encode_objects(objects[:5], [None] * 5).cpu().numpy()
    assert np.array_equal(after, before)
