"""Seeded synthetic inputs and weights for the coarse-retrieval hot path.

No KITTI360Pose data, checkpoints or T5 weights exist in this environment, so tests, the bench,
``smoke()`` and the golden-fixture generator all draw from the generators below (numpy PCG64
streams, stable across platforms). The distributions follow SURVEY.md §8(d):

* cells: n_i ~ U{6..35} objects (exercises the >28 truncation), per object a class index 1..22,
  mean rgb U[0,1]^3, centre U[0,1]^3, point count ~ clipped log-normal matched to the statistics the
  reference hard-codes in ``models/object_encoder.py:43-44`` (mean 1826.68, std 2516.89);
* weights: one array per ``state_dict`` key of the reference's coarse model (key names and shapes
  per SURVEY.md §8(b)), BatchNorm running statistics perturbed so that BN folding is exercised;
* retrieval embeddings: unit-normalised N(0,1)^256 rows with one planted positive per query.

Nothing here is on the product compute path.
"""
from __future__ import annotations

import numpy as np

from .tables import COLOR_NAMES, COLORS, KNOWN_CLASS  # noqa: F401  (dataset constants live with the product)

NUM_MEAN = 1826.6844940968194  # models/object_encoder.py:43
NUM_STD = 2516.8905096993817  # models/object_encoder.py:44


# ----------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------
def _linear(rng, out_f, in_f, prefix, sd):
    b = 1.0 / np.sqrt(in_f)
    sd[prefix + ".weight"] = rng.uniform(-b, b, size=(out_f, in_f)).astype(np.float32)
    sd[prefix + ".bias"] = rng.uniform(-b, b, size=(out_f,)).astype(np.float32)


def _bn(rng, c, prefix, sd):
    sd[prefix + ".weight"] = rng.uniform(0.5, 1.5, size=(c,)).astype(np.float32)
    sd[prefix + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
    sd[prefix + ".running_mean"] = (0.3 * rng.standard_normal(c)).astype(np.float32)
    sd[prefix + ".running_var"] = rng.uniform(0.5, 2.0, size=(c,)).astype(np.float32)
    sd[prefix + ".num_batches_tracked"] = np.array(100, dtype=np.int64)


def _mlp(rng, channels, prefix, sd, last_relu=True):
    """Key layout of the reference's get_mlp / get_mlp2 (models/language_encoder.py:16-74):
    ``{prefix}.{layer}.0`` = Linear, ``{prefix}.{layer}.1`` = BatchNorm1d."""
    for i in range(1, len(channels)):
        _linear(rng, channels[i], channels[i - 1], f"{prefix}.{i - 1}.0", sd)
        _bn(rng, channels[i], f"{prefix}.{i - 1}.1", sd)


def _encoder_layer(rng, d, ff, prefix, sd):
    """Key layout of torch.nn.TransformerEncoderLayer (post-norm, as the reference uses it)."""
    b = np.sqrt(6.0 / (d + 3 * d))
    sd[prefix + ".self_attn.in_proj_weight"] = rng.uniform(-b, b, size=(3 * d, d)).astype(np.float32)
    sd[prefix + ".self_attn.in_proj_bias"] = (0.02 * rng.standard_normal(3 * d)).astype(np.float32)
    _linear(rng, d, d, prefix + ".self_attn.out_proj", sd)
    _linear(rng, ff, d, prefix + ".linear1", sd)
    _linear(rng, d, ff, prefix + ".linear2", sd)
    for n in ("norm1", "norm2"):
        sd[f"{prefix}.{n}.weight"] = rng.uniform(0.8, 1.2, size=(d,)).astype(np.float32)
        sd[f"{prefix}.{n}.bias"] = (0.05 * rng.standard_normal(d)).astype(np.float32)


def make_object_branch_weights(seed: int = 0, embed_dim: int = 256, num_layers: int = 2,
                               use_features=("class", "color", "position", "num")) -> dict:
    """state_dict (numpy) of the 3D-submap branch: ``object_encoder.*`` (minus PointNet++) and
    ``obj_inter_module.*``. Shapes: models/object_encoder.py:28-64, models/cell_retrieval.py:35."""
    rng = np.random.default_rng([seed, 0xC311])
    sd: dict = {}
    d = embed_dim
    emb = rng.standard_normal((len(KNOWN_CLASS) + 1, d)).astype(np.float32)
    emb[0] = 0.0  # padding_idx=0 row (object_encoder.py:33)
    sd["object_encoder.class_embedding.weight"] = emb
    # known_colors dict has 7 distinct names + "<unk>" = 8 rows (object_encoder.py:35-37)
    cemb = rng.standard_normal((len(set(COLOR_NAMES)) + 1, d)).astype(np.float32)
    cemb[0] = 0.0
    sd["object_encoder.color_embedding.weight"] = cemb
    _mlp(rng, [3, 64, d], "object_encoder.pos_encoder", sd)
    _mlp(rng, [3, 64, d], "object_encoder.color_encoder", sd)
    _mlp(rng, [1, 64, d], "object_encoder.num_encoder", sd)
    _mlp(rng, [256, d], "object_encoder.mlp_pointnet", sd)
    _mlp(rng, [len(use_features) * d, d], "object_encoder.mlp_merge", sd)
    for layer in range(num_layers):
        _encoder_layer(rng, d, 2 * d, f"obj_inter_module.{layer}", sd)
    return sd


def make_pointnet_weights(seed: int = 0, n_classes: int = 22, n_colors: int = 8) -> dict:
    """state_dict (numpy) of ``object_encoder.pointnet.*`` with the reference's key layout
    (models/pointcloud/pointnet2.py:52-64): three SetAbstraction get_mlp's, the global get_mlp, lin1, lin2 and the
    two classifier heads (read by the backbone's pretraining step only: ``pointnet_pretrain``, t2l_pointnet_cls_heads)."""
    rng = np.random.default_rng([seed, 0x9A27])
    sd: dict = {}
    p = "object_encoder.pointnet."
    _mlp(rng, [3 + 3, 32, 64], p + "sa1.point_conv.local_nn", sd)
    _mlp(rng, [64 + 3, 128, 128], p + "sa2.point_conv.local_nn", sd)
    _mlp(rng, [128 + 3, 256, 256], p + "sa3.point_conv.local_nn", sd)
    _mlp(rng, [256 + 3, 512, 1024], p + "ga.mlp", sd)
    _linear(rng, 512, 1024, p + "lin1", sd)
    _linear(rng, 256, 512, p + "lin2", sd)
    _linear(rng, n_classes, 256, p + "class_classifier", sd)
    _linear(rng, n_colors, 256, p + "color_classifier", sd)
    return sd


def make_sampled_points(cells: dict, seed: int = 0, n_points: int = 256):
    """(pos f32[total_objects, n_points, 3], rgb f32[total_objects, n_points, 3]): what the reference's dataloader hands
    PointNet++ per object after FixedPoints(256) + NormalizeScale (dataloading/kitti360pose/utils.py:91-147,
    training/coarse.py:182-193): positions centred and scaled into [-1,1]^3, colours in [0,1]. Objects are anisotropic
    Gaussian blobs so that the 0.2/0.3/0.4 ball queries see anything from 1 to >32 neighbours."""
    rng = np.random.default_rng([seed, 0xB10B])
    total = int(cells["offsets"][-1])
    scale = rng.uniform(0.05, 0.6, size=(total, 1, 3))
    pos = rng.standard_normal((total, n_points, 3)) * scale
    pos -= pos.mean(axis=1, keepdims=True)
    pos /= np.abs(pos).max(axis=(1, 2), keepdims=True) / 0.999999
    base = rng.uniform(0, 1, size=(total, 1, 3))
    rgb = np.clip(base + 0.1 * rng.standard_normal((total, n_points, 3)), 0, 1)
    return pos.astype(np.float32), rgb.astype(np.float32)


def _decoder_layer(rng, d, ff, prefix, sd):
    """Key layout of torch.nn.TransformerDecoderLayer (post-norm): self_attn, multihead_attn, linear1/2, norm1-3."""
    b = np.sqrt(6.0 / (d + 3 * d))
    for att in ("self_attn", "multihead_attn"):
        sd[f"{prefix}.{att}.in_proj_weight"] = rng.uniform(-b, b, size=(3 * d, d)).astype(np.float32)
        sd[f"{prefix}.{att}.in_proj_bias"] = (0.02 * rng.standard_normal(3 * d)).astype(np.float32)
        _linear(rng, d, d, f"{prefix}.{att}.out_proj", sd)
    _linear(rng, ff, d, prefix + ".linear1", sd)
    _linear(rng, d, ff, prefix + ".linear2", sd)
    for n in ("norm1", "norm2", "norm3"):
        sd[f"{prefix}.{n}.weight"] = rng.uniform(0.8, 1.2, size=(d,)).astype(np.float32)
        sd[f"{prefix}.{n}.bias"] = (0.05 * rng.standard_normal(d)).astype(np.float32)


def make_fine_weights(seed: int = 0, embed_dim: int = 128, num_layers: int = 2) -> dict:
    """state_dict (numpy) of the fine-stage ``CrossMatch`` without its text branch (models/cross_matcher.py:55-84):
    ``object_encoder.*`` at fine_embed_dim, ``cross_objects.{i}.*`` / ``cross_hints.{i}.*`` decoder layers, ``mlp_offsets``."""
    sd = {k: v for k, v in make_object_branch_weights(seed + 101, embed_dim=embed_dim, num_layers=0).items()
          if k.startswith("object_encoder.")}
    rng = np.random.default_rng([seed, 0xF17E])
    for i in range(num_layers):
        _decoder_layer(rng, embed_dim, 4 * embed_dim, f"cross_hints.{i}", sd)
        _decoder_layer(rng, embed_dim, 4 * embed_dim, f"cross_objects.{i}", sd)
    if num_layers == 0:  # fine_num_decoder_layers == 0: ONE cross_hints layer, no index in its keys, no cross_objects (cross_matcher.py:75-79)
        _decoder_layer(rng, embed_dim, 4 * embed_dim, "cross_hints", sd)
    _linear(rng, embed_dim // 2, embed_dim, "mlp_offsets.0", sd)
    _linear(rng, 2, embed_dim // 2, "mlp_offsets.2", sd)
    return sd


def make_language_head_weights(seed: int = 0, embed_dim: int = 256, t5_dim: int = 1024) -> dict:
    """state_dict (numpy) of the text head after T5 (models/language_encoder.py:95-101)."""
    rng = np.random.default_rng([seed, 0x7E47])
    sd: dict = {}
    _encoder_layer(rng, t5_dim, 4 * t5_dim, "language_encoder.intra_module.0", sd)
    _mlp(rng, [t5_dim, embed_dim], "language_encoder.inter_mlp", sd)
    _encoder_layer(rng, embed_dim, 4 * embed_dim, "language_encoder.inter_module.0", sd)
    return sd


# ----------------------------------------------------------------------------------------------
# cells (packed per-object features; the reference derives these from Object3d point sets)
# ----------------------------------------------------------------------------------------------
def nearest_color_index(rgb_mean: np.ndarray) -> np.ndarray:
    """Index into COLORS of the nearest centre (datapreparation/kitti360pose/imports.py:33-38)."""
    rgb_mean = np.atleast_2d(rgb_mean)
    d = np.linalg.norm(rgb_mean[:, None, :] - COLORS[None, :, :], axis=2)
    return np.argmin(d, axis=1)


def color_name_to_embed_index(color_table_index: np.ndarray) -> np.ndarray:
    """COLORS index -> row of ``color_embedding``: the reference builds
    ``{name: i for i, name in enumerate(COLOR_NAMES)}`` (object_encoder.py:35) so the duplicate
    'gray' maps both 1 and 4 to 4, and 'dark-green' -> 0 (the padding row)."""
    name_to_idx = {c: i for i, c in enumerate(COLOR_NAMES)}
    lut = np.array([name_to_idx[c] for c in COLOR_NAMES], dtype=np.int32)
    return lut[np.asarray(color_table_index)]


def make_cells(n_cells: int, seed: int = 0, min_obj: int = 6, max_obj: int = 35,
               with_pn_feat: bool = False) -> dict:
    """Packed SoA description of ``n_cells`` synthetic cells.

    Returns a dict with ``counts i32[B]``, ``offsets i32[B+1]`` and per-object arrays
    ``class_idx i32``, ``color_idx i32`` (row of color_embedding), ``rgb f32[.,3]``,
    ``center f32[.,3]``, ``n_pts f32`` and optionally ``pn_feat f32[.,256]``.
    """
    rng = np.random.default_rng([seed, 0xCE11])
    counts = rng.integers(min_obj, max_obj + 1, size=n_cells).astype(np.int32)
    offsets = np.zeros(n_cells + 1, dtype=np.int32)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    class_idx = rng.integers(1, len(KNOWN_CLASS) + 1, size=total).astype(np.int32)
    rgb = rng.uniform(0.0, 1.0, size=(total, 3))
    center = rng.uniform(0.0, 1.0, size=(total, 3))
    # log-normal with the mean/std hard-coded in the reference
    sigma2 = np.log(1.0 + (NUM_STD / NUM_MEAN) ** 2)
    mu = np.log(NUM_MEAN) - 0.5 * sigma2
    n_pts = np.clip(np.round(rng.lognormal(mu, np.sqrt(sigma2), size=total)), 25, 60000)
    out = {
        "counts": counts,
        "offsets": offsets,
        "class_idx": class_idx,
        "color_idx": color_name_to_embed_index(nearest_color_index(rgb)).astype(np.int32),
        "rgb": rgb.astype(np.float32),
        "center": center.astype(np.float32),
        "n_pts": n_pts.astype(np.float32),
    }
    if with_pn_feat:
        out["pn_feat"] = np.abs(rng.standard_normal((total, 256))).astype(np.float32)
    return out


def make_object_points(cells: dict, seed: int = 0):
    """Yield (cell, obj_in_cell, label, xyz f64[n,3], rgb f32[n,3]) point sets whose statistics follow
    ``cells``: stands in for the raw ``Object3d.xyz/.rgb`` the reference reduces on the host
    (datapreparation/kitti360pose/imports.py:28-41)."""
    rng = np.random.default_rng([seed, 0x0B7])
    for b in range(len(cells["counts"])):
        lo, hi = int(cells["offsets"][b]), int(cells["offsets"][b + 1])
        for o in range(lo, hi):
            n = int(cells["n_pts"][o])
            xyz = cells["center"][o].astype(np.float64) + 0.02 * rng.standard_normal((n, 3))
            rgb = np.clip(cells["rgb"][o].astype(np.float64) + 0.05 * rng.standard_normal((n, 3)), 0, 1)
            yield b, o - lo, KNOWN_CLASS[int(cells["class_idx"][o]) - 1], xyz, rgb.astype(np.float32)


def make_t5_hidden(n_sentences: int, n_tokens: int, dim: int = 1024, seed: int = 0) -> np.ndarray:
    """Stand-in for a frozen T5 encoder's last_hidden_state f32[n_sentences, n_tokens, dim]."""
    rng = np.random.default_rng([seed, 0x75])
    return (0.2 * rng.standard_normal((n_sentences, n_tokens, dim))).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# retrieval embeddings
# ----------------------------------------------------------------------------------------------
def unit_rows(x: np.ndarray) -> np.ndarray:
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.maximum(n, 1e-12)


def make_retrieval_problem(n_cells: int, n_queries: int, dim: int = 256, seed: int = 0,
                           noise: float = 0.5):
    """DB ``f32[N,dim]`` unit rows and queries ``f32[Q,dim]`` with a planted positive per query
    (``t_q = normalize(c_pi(q) + noise * unit-noise)``).
    Returns (db, queries, target_row i64[Q])."""
    rng = np.random.default_rng([seed, 0x5EA7])
    db = unit_rows(rng.standard_normal((n_cells, dim))).astype(np.float32)
    target = rng.integers(0, n_cells, size=n_queries)
    nz = unit_rows(rng.standard_normal((n_queries, dim)))
    q = unit_rows(db[target].astype(np.float64) + noise * nz).astype(np.float32)
    return db, q, target.astype(np.int64)


def make_queries_for(db: np.ndarray, n_queries: int, seed: int = 0, noise: float = 0.5):
    """Another batch of planted-positive queries for an existing DB (same recipe as ``make_retrieval_problem``).
    Returns (queries f32[Q,dim], target_row i64[Q])."""
    rng = np.random.default_rng([seed, 0xBA7C])
    target = rng.integers(0, len(db), size=n_queries)
    nz = unit_rows(rng.standard_normal((n_queries, db.shape[1])))
    q = unit_rows(db[target].astype(np.float64) + noise * nz).astype(np.float32)
    return q, target.astype(np.int64)


# ----------------------------------------------------------------------------------------------
# a whole KITTI360Pose-shaped dataset in memory (cells with raw object points, poses with hints)
# ----------------------------------------------------------------------------------------------
HINT_DIRECTIONS = ("north", "south", "east", "west", "on-top")


def make_k360_records(n_cells: int, n_poses: int, seed: int = 0, pts_per_obj=(24, 64), n_hints: int = 6,
                      cell_size: float = 30.0, cell_dist: float = 10.0, scene: str = "0010"):
    """(cells, poses): record objects shaped like the reference's pickled ``Cell`` / ``Object3d`` / ``Pose`` /
    ``DescriptionBestCell`` (datapreparation/kitti360pose/imports.py:8-245) — ``text2loc_amd.kitti360pose``'s record types, the
    same ones its reader returns — for ``Kitti360PoseDataset.from_records``. Cells follow ``make_cells`` (n_i ~ U{6..35}), every
    object carries RAW points (``pts_per_obj`` = inclusive range of point counts; KITTI360Pose's mean is 1,827 — kept small here so
    that 11,259 cells fit a bench host), cells sit on a square grid ``cell_dist`` apart (overlapping, as prepare.py lays them out),
    every pose lies in a random cell and is described by ``n_hints`` of that cell's objects with the template fields
    ``hint_sentences`` reads (direction, object_color_text, object_label)."""
    from .kitti360pose import CellRecord, HintRecord, ObjectRecord, PoseRecord

    cn = make_cells(n_cells, seed=seed)
    rng = np.random.default_rng([seed, 0x360])
    total = int(cn["offsets"][-1])
    npts = rng.integers(int(pts_per_obj[0]), int(pts_per_obj[1]) + 1, size=total).astype(np.int64)
    poff = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(npts, out=poff[1:])
    P = int(poff[-1])
    obj_of = np.repeat(np.arange(total), npts)
    xyz_all = cn["center"].astype(np.float64)[obj_of] + 0.02 * rng.standard_normal((P, 3))
    rgb_all = np.clip(cn["rgb"][obj_of] + (0.05 * rng.standard_normal((P, 3))).astype(np.float32), 0, 1).astype(np.float32)
    labels = [KNOWN_CLASS[int(c) - 1] for c in cn["class_idx"]]
    colors = [COLOR_NAMES[int(c)] for c in nearest_color_index(cn["rgb"])]
    side = int(np.ceil(np.sqrt(n_cells)))
    cells = []
    for b in range(n_cells):
        lo, hi = int(cn["offsets"][b]), int(cn["offsets"][b + 1])
        objs = []
        for o in range(lo, hi):
            r = ObjectRecord()
            r.__dict__.update(id=o, instance_id=o, xyz=xyz_all[poff[o]:poff[o + 1]], rgb=rgb_all[poff[o]:poff[o + 1]], label=labels[o])
            objs.append(r)
        x0, y0 = (b % side) * cell_dist, (b // side) * cell_dist
        c = CellRecord()
        c.__dict__.update(id=f"{scene}_{b:05d}", scene_name=scene, objects=objs, cell_size=float(cell_size),
                          bbox_w=np.array([x0, y0, 0.0, x0 + cell_size, y0 + cell_size, cell_size], dtype=np.float64))
        cells.append(c)
    poses = []
    target = rng.integers(0, n_cells, size=n_poses)
    in_cell = rng.uniform(0.25, 0.75, size=(n_poses, 3))
    for q in range(n_poses):
        b = int(target[q])
        lo, n_obj = int(cn["offsets"][b]), int(cn["counts"][b])
        pick = lo + rng.choice(n_obj, size=n_hints, replace=n_obj < n_hints)
        descs = []
        for o in pick:
            d = cn["center"][o][:2] - in_cell[q, :2]
            if float(np.abs(d).max()) < 0.05:
                direction = "on-top"
            elif abs(d[0]) >= abs(d[1]):
                direction = "east" if d[0] > 0 else "west"
            else:
                direction = "north" if d[1] > 0 else "south"
            h = HintRecord()
            h.__dict__.update(direction=direction, object_label=labels[o], object_color_text=colors[o], object_id=int(o),
                              closest_point=cn["center"][o].astype(np.float64).copy())
            descs.append(h)
        p = PoseRecord()
        bb = cells[b].bbox_w
        p.__dict__.update(pose=in_cell[q].copy(), pose_w=bb[0:3] + in_cell[q] * cell_size, cell_id=cells[b].id, scene_name=scene,
                          descriptions=descs)
        poses.append(p)
    return cells, poses


def make_text_cache(sentences, device, seed: int = 0, tok_range=(9, 14), max_tokens: int = 16, dim: int = 1024):
    """A ``TextCache`` over ``sentences`` whose "T5 hidden states" are seeded noise (the image holds no T5-large weights):
    BASELINE config 2's "frozen T5-large embeddings precomputed", with per-sentence token counts drawn from ``tok_range`` so that
    the batch-dependent padding length L of the reference's text path is exercised."""
    import torch

    from .text_cache import TextCache

    sentences = list(sentences)
    rng = np.random.default_rng([seed, 0x7C])
    cache = TextCache(None, None, device, max_tokens=max_tokens, dim=dim)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    cache.hidden = (0.2 * torch.randn(len(sentences), max_tokens, dim, generator=g)).to(device)
    cache.n_tok = rng.integers(int(tok_range[0]), int(tok_range[1]) + 1, size=len(sentences)).astype(np.int32)
    cache.index = {s: i for i, s in enumerate(sentences)}
    return cache


def coarse_args(**kw):
    """The published coarse configuration as the Namespace the reference's scripts hand the model (README.md:87-99,
    evaluation/args.py) — ``class_embed`` / ``color_embed`` off = PointNet++ features, the published mode."""
    import argparse

    a = argparse.Namespace(coarse_embed_dim=256, object_size=28, object_inter_module_num_heads=4, object_inter_module_num_layers=2,
                           hungging_model=None, fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4,
                           inter_module_num_layers=1, inter_module_num_heads=4, class_embed=False, color_embed=False,
                           use_features=["class", "color", "position", "num"], ranking_loss="contrastive", top_k=[1, 3, 5, 10],
                           threshs=[5, 10, 15], batch_size=1, no_pc_augment=True, pointnet_freeze=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def make_coarse_model(args, device="cuda", seed: int = 0, sentences=None):
    """``CellRetrievalNetwork`` with seeded weights for every branch (object branch, PointNet++, text head) in eval mode on
    ``device``; T5 is absent (``llm_model`` is a placeholder) — with ``sentences`` the text branch sits behind a synthetic
    ``TextCache`` over them (``make_text_cache``), i.e. BASELINE config 2's precomputed T5 embeddings."""
    import torch

    from .cell_retrieval import CellRetrievalNetwork, LanguageEncoder

    le = LanguageEncoder(256, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1, llm_model=object(),
                         tokenizer=None, input_dim=1024)
    model = CellRetrievalNetwork(list(KNOWN_CLASS), list(COLOR_NAMES), args, language_encoder=le)
    sd = dict(make_object_branch_weights(seed))
    sd.update(make_pointnet_weights(seed, n_classes=len(KNOWN_CLASS), n_colors=len(COLOR_NAMES)))
    sd.update(make_language_head_weights(seed))
    missing = model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.unexpected_keys], missing.unexpected_keys
    model = model.to(device).eval()
    if sentences is not None:
        le.text_cache = make_text_cache(sentences, device, seed=seed)
    return model
