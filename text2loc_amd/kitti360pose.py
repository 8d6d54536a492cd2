"""Reader for the reference's on-disk KITTI360Pose data — ``<base>/cells/<scene>.pkl`` and ``<base>/poses/<scene>.pkl``
(dataloading/kitti360pose/base.py:40-48) — WITHOUT the reference's classes on ``sys.path``.

The pickles hold instances of ``datapreparation.kitti360pose.imports.{Cell, Object3d, Pose, DescriptionBestCell,
DescriptionPoseCell}`` (plain attribute bags, imports.py:8-245). Unpickling normally imports those modules (and with them
cv2, easydict, ...). ``KittiUnpickler.find_class`` instead resolves every class of that package to a small record type
defined here, which receives the pickled ``__dict__`` unchanged: same attribute names, nothing else. The records are what
the rest of this package duck-types against (``.label/.xyz/.rgb``, ``.id/.objects/.cell_size/.bbox_w/.get_center()``,
``.pose_w/.cell_id/.descriptions[*].direction/.object_color_text/.object_label``).

On top of that, the dataset surface ``evaluation.pipeline`` / ``training.coarse.eval_epoch`` consume
(dataloading/kitti360pose/cells.py:36-205), with the training-time augmentations (``shuffle_hints``, ``flip_poses``):

    ds = Kitti360PoseDataset(base_path, scene_names)           # ~ Kitti360CoarseDatasetMulti(..., transform, shuffle_hints, flip_poses)
    ds.all_cells, ds.all_poses, ds.get_cell_dataset(), ds[i] -> {"poses","cells","objects","object_points","texts","cell_ids",...}
    dl = DataLoader(ds, batch_size=..., collate_fn=Kitti360PoseDataset.collate_fn)
    db = CellDatabase.build(model, ds.get_cell_dataset())

``object_points``: the reference hands PointNet++ a PyG batch of per-object FixedPoints(256) samples per cell — and nothing
else under ``--no_pc_augment``, which every published command passes; NormalizeScale (and RandomRotate in training) only
without the flag (dataloading/kitti360pose/utils.py:91-147, evaluation/pipeline.py:215-223, training/coarse.py:182-193).
``object_points="sample"`` builds those batches with ``packing.sample_object_points`` (host, seeded) under ``transform``
("fixed" by default = the published configuration); ``None`` skips them (class_embed mode does not read them).

The fine stage's counterpart (dataloading/kitti360pose/poses.py:36-172, 368-590) is ``Kitti360FineDataset``: one item per pose,
what ``load_pose_and_cell`` returns, for ``fine_training.train_epoch``. Its third point mode, ``object_points="ids"``, leaves the
points on the GPU: an item names 16 rows of the dataset's ``packing.PackedCellSet`` and ``fine_batches`` samples a whole batch of
them in one launch in the process that owns the engine.
``Kitti360PoseDataset(object_points="ids")`` with ``coarse_batches`` is the coarse stage's form of it: an item names its cell's rows
and a flip code instead of carrying a mirrored copy of the cell (t2l_gather_object_rows gathers its packed features by them).
What the two datasets share (loading, the point properties, ``packed()``, ``collate_fn``) is ``_PoseDataset``; their batches come out
of one loop, ``_batches``, and one launch per batch (``PackedCellSet.sample_rows``: t2l_sample_object_points_mirrored, the fine
stage's rows without a code) — each dataset adds only its own GPU step, ``_device_batch``.
"""
from __future__ import annotations

import io
import os.path as osp
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch.utils.data

from . import packing
from .tables import CLASS_TO_INDEX, SCENE_NAMES_TEST, SCENE_NAMES_TRAIN, SCENE_NAMES_VAL

_REF_PACKAGE = "datapreparation.kitti360pose"


class Record:
    """Attribute bag standing in for a pickled reference object (pickle restores ``__dict__`` through ``__setstate__``
    or, without one, by updating ``__dict__`` — both land here)."""

    _ref_class = "object"

    def __setstate__(self, state):
        if isinstance(state, tuple) and len(state) == 2:  # (dict, slots) form
            for part in state:
                if part:
                    self.__dict__.update(part)
        elif state:
            self.__dict__.update(state)

    def __repr__(self):
        return f"<{self._ref_class} {getattr(self, 'id', getattr(self, 'label', ''))}>"


class ObjectRecord(Record):
    """imports.py:8-83 ``Object3d``: id, instance_id, xyz f64[n,3], rgb [n,3], label."""

    _ref_class = "Object3d"

    def get_center(self):
        return np.mean(self.xyz, axis=0)

    def get_color_rgb(self):
        return np.mean(self.rgb, axis=0)

    def get_color_text(self):
        return packing.COLOR_NAMES[int(np.argmin(np.linalg.norm(np.mean(self.rgb, axis=0) - packing.COLORS, axis=1)))]


class CellRecord(Record):
    """imports.py:221-245 ``Cell``: id, scene_name, objects, cell_size, bbox_w."""

    _ref_class = "Cell"

    def get_center(self):
        b = np.asarray(self.bbox_w)
        return 0.5 * (b[0:3] + b[3:6])


class PoseRecord(Record):
    """imports.py:175-218 ``Pose``: pose, pose_w, cell_id, scene_name, descriptions, described_by."""

    _ref_class = "Pose"


class HintRecord(Record):
    """imports.py:86-172 ``DescriptionPoseCell`` / ``DescriptionBestCell``: direction, object_label, object_color_text, ..."""

    _ref_class = "Description"


_CLASS_MAP = {"Object3d": ObjectRecord, "Cell": CellRecord, "Pose": PoseRecord, "DescriptionBestCell": HintRecord,
              "DescriptionPoseCell": HintRecord, "Description": HintRecord}


# Exact (module, name) pairs a KITTI360Pose pickle may resolve besides the reference's own record classes: what numpy
# arrays / scalars and plain containers need to rebuild themselves (both numpy 1.x and 2.x module spellings). Nothing else
# — in particular nothing of ``builtins`` that can call or import (eval, exec, getattr, __import__) — is reachable, so a
# crafted dataset pickle cannot execute code through ``load_pickle``.
_SAFE_GLOBALS = {
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
    ("numpy", "ndarray"), ("numpy", "dtype"),
    ("_codecs", "encode"),
    ("collections", "OrderedDict"),
} | {("builtins", n) for n in ("list", "dict", "set", "tuple", "str", "int", "float", "bool", "bytes", "bytearray", "complex",
                                 "frozenset", "slice", "range", "object")}


class KittiUnpickler(pickle.Unpickler):
    """Resolves classes of the reference's ``datapreparation.kitti360pose`` package to the records above and the exact
    numpy / container reconstructors of ``_SAFE_GLOBALS``; every other global raises ``UnpicklingError``. Unknown classes
    of the reference's package become generic ``Record``s."""

    def find_class(self, module, name):
        if module == _REF_PACKAGE or module.startswith(_REF_PACKAGE + ".") or module.startswith("datapreparation.kitti360."):
            return _CLASS_MAP.get(name, Record)  # dataloading/__init__.py:8-10 aliases the old package name
        if (module, name) in _SAFE_GLOBALS:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing to resolve {module}.{name} while reading a KITTI360Pose pickle")


def load_pickle(path: str):
    with open(path, "rb") as f:
        return KittiUnpickler(io.BufferedReader(f)).load()


def load_scene(base_path: str, scene_name: str):
    """(cells, poses) of one scene, as base.py:40-48 reads them (ids must be unique inside the scene)."""
    cells = load_pickle(osp.join(base_path, "cells", f"{scene_name}.pkl"))
    poses = load_pickle(osp.join(base_path, "poses", f"{scene_name}.pkl"))
    ids = [c.id for c in cells]
    if len(set(ids)) != len(ids):
        raise ValueError(f"{scene_name}: cell ids repeat")
    return cells, poses


def hint_sentences(pose) -> List[str]:
    """base.py:60-68: one template sentence per description."""
    return [f"The pose is {d.direction} of a {d.object_color_text} {d.object_label}." for d in pose.descriptions]


def _swap_words(text: str, a: str, b: str) -> str:
    return text.replace(a, a + "-flipped").replace(b, a).replace(a + "-flipped", b)


def _flipped_pose(pose, code: int):
    """The pose half of a flip about x = 0.5 (bit 0 of ``code``) and / or y = 0.5 (bit 1): ONE copy (a pose is a few hundred bytes, its
    deep copy tens of microseconds) whose pose-in-cell and whose descriptions' ``closest_point`` are mirrored."""
    import copy

    pose = copy.deepcopy(pose)
    for ax in (0, 1):
        if code >> ax & 1:
            pose.pose[ax] = 1.0 - pose.pose[ax]
            for d in pose.descriptions:
                d.closest_point[ax] = 1.0 - d.closest_point[ax]
    return pose


def flip_pose_in_cell(pose, cell, text: str, direction: int):
    """dataloading/kitti360pose/utils.py:15-88 (the three-value form the coarse dataset uses): mirror the cell about x = 0.5
    (``direction`` +1, "horizontally": east <-> west in the text) or y = 0.5 (-1, "vertically": north <-> south). Pose and
    cell are copied first; object points, the pose-in-cell and every description's ``closest_point`` are mirrored, the
    descriptions' ``direction`` fields are NOT (as in the reference: only the text changes)."""
    import copy

    if direction not in (-1, 1):
        raise ValueError("direction must be +1 (horizontal) or -1 (vertical)")
    ax = 0 if direction == 1 else 1
    pose, cell = _flipped_pose(pose, 1 << ax), copy.deepcopy(cell)
    for obj in cell.objects:
        obj.xyz[:, ax] = 1 - obj.xyz[:, ax]
        if hasattr(obj, "_t2l_feat"):
            del obj._t2l_feat  # cached reductions of the un-mirrored points
    text = _swap_words(text, "east", "west") if direction == 1 else _swap_words(text, "north", "south")
    return pose, cell, text


class CellOnlyDataset:
    """cells.py:187-205 ``Kitti360CoarseCellOnlyDataset``: one item per database cell, in ``all_cells`` order (never flipped
    or shuffled, as in the reference)."""

    def __init__(self, cells: Sequence[CellRecord], object_points: Optional[str] = None, seed: int = 0, transform: str = "fixed",
                 packed_holder: Optional[dict] = None):
        self.cells = list(cells)
        self._points = object_points
        self._seed = seed
        self._transform = "normalize" if transform == "rotate_normalize" else transform  # val transform: no rotation
        self._packed_holder = packed_holder if packed_holder is not None else {}

    def __len__(self):
        return len(self.cells)

    # ---- the engine-sized path: every cell of the database flattened ONCE (packing.PackedCellSet) ---------------------------
    # ``coarse.eval_epoch`` / ``CellDatabase.build`` encode through it when it is there (CellRetrievalNetwork.encode_cell_set):
    # one host pass over the objects per DATASET instead of one per forward call, the per-object reductions, FixedPoints and
    # PointNet++ on the GPU over chunks of thousands of cells whatever ``args.batch_size`` says. The holder is shared with the
    # parent ``Kitti360PoseDataset`` (``get_cell_dataset`` builds a new CellOnlyDataset per call: the three validation passes per
    # epoch of training/coarse.py:283-287 must not flatten the database three times).
    @property
    def wants_points(self) -> bool:
        return self._points is not None

    @property
    def point_transform(self) -> str:
        return self._transform

    @property
    def point_seed(self) -> int:
        return int(self._seed)

    def packed(self):
        ps = self._packed_holder.get("set")
        if ps is None:
            ps = self._packed_holder["set"] = packing.PackedCellSet(self.cells)
        return ps

    def _object_points(self, cell, idx):
        if self._points is None:
            return None
        rng = np.random.default_rng([self._seed, idx])
        return packing.sample_object_points([cell.objects], 256, rng, transform=self._transform)[0]

    def __getitem__(self, idx):
        cell = self.cells[idx]
        return {"cells": cell, "cell_ids": cell.id, "objects": cell.objects, "object_points": self._object_points(cell, idx)}


class _PoseDataset:
    """What ``Kitti360PoseDataset`` and ``Kitti360FineDataset`` share: one item per pose over the scenes of a KITTI360Pose directory or
    of a dict ``{scene: (cells, poses)}`` of records already in memory, a point mode, and the cells flattened once."""

    def __init__(self, base_path, scene_names: Sequence[str], object_points: Optional[str], transform: str, seed, points: bool = True):
        if object_points not in (None, "sample", "ids"):
            raise ValueError("object_points must be None, 'sample' or 'ids'")
        if transform not in packing.POINT_TRANSFORMS:
            raise ValueError(f"transform must be one of {sorted(packing.POINT_TRANSFORMS)}")
        self.scene_names = list(scene_names)
        self._points, self._transform, self._seed, self._epoch = object_points, transform, seed, 0
        self.all_cells: List[CellRecord] = []
        self.all_poses: List[PoseRecord] = []
        self.hint_descriptions: List[List[str]] = []
        self._packed_holder: dict = {}
        self._ids_points = bool(points)
        self._scenes = []  # (scene, cells, poses) as loaded: each dataset builds its own tables (scene names, cell rows) from them
        for s in self.scene_names:
            cells, poses = base_path[s] if isinstance(base_path, dict) else load_scene(base_path, s)
            self._scenes.append((s, cells, poses))
            self.all_cells.extend(cells)
            self.all_poses.extend(poses)
            self.hint_descriptions.extend(hint_sentences(p) for p in poses)

    @classmethod
    def from_records(cls, cells: Sequence[CellRecord], poses: Sequence[PoseRecord], *args, scene_name: str = "in_memory", **kw):
        """The same dataset over records that are already in memory (one scene): what ``load_scene`` would have returned."""
        return cls({scene_name: (list(cells), list(poses))}, [scene_name], *args, **kw)

    def __len__(self):
        return len(self.all_poses)

    @property
    def point_mode(self) -> Optional[str]:
        return self._points

    @property
    def point_transform(self) -> str:
        return self._transform

    @property
    def point_seed(self) -> int:
        return int(self._seed)

    @property
    def wants_points(self) -> bool:
        """Whether a batch carries point rows: "sample" always; "ids" unless built with ``points=False``."""
        return self._points == "sample" or (self._points == "ids" and self._ids_points)

    def set_epoch(self, epoch: int):
        """Call once per epoch (as DistributedSampler.set_epoch): part of the key of the point draws that are redrawn per fetch — the
        coarse set's under transform="rotate_normalize" (DataLoader workers restart from a copy of this object every epoch), all of
        the fine set's, and ``draw_salts`` of both "ids" modes."""
        self._epoch = int(epoch)

    def packed(self) -> packing.PackedCellSet:
        """Every cell of the dataset flattened once; ``object_rows`` index its objects, its ``pad_row`` stands for a fine-stage pad."""
        ps = self._packed_holder.get("set")
        if ps is None:
            ps = self._packed_holder["set"] = packing.PackedCellSet(self.all_cells)
        return ps

    @staticmethod
    def collate_fn(data):
        return {key: [d[key] for d in data] for key in data[0].keys()}


class Kitti360PoseDataset(_PoseDataset):
    """One item per pose over several scenes (cells.py:36-185 ``Kitti360CoarseDataset`` / ``...Multi``).

    ``transform``: the point transform of ``object_points="sample"`` — "fixed" (FixedPoints(256) only: `--no_pc_augment`,
    what every published command passes and therefore the default), "normalize", "rotate_normalize"
    (``packing.point_transform_from_args(args, train=...)`` picks it the way the reference's scripts do).
    ``shuffle_hints`` / ``flip_poses``: the training-time augmentations of cells.py:80-91 (training/coarse.py:196-202 turns
    both on): the hint sentences are permuted, and with probability 1/2 each the cell is mirrored horizontally and
    vertically (``flip_pose_in_cell``). Their draws come from ``aug_rng`` — a ``numpy.random.RandomState`` consumed with the
    reference's own call sequence (one ``choice`` without replacement over the hints, then two ``choice((True, False))``), so
    ``RandomState(s)`` here reproduces the reference under ``np.random.seed(s)`` item for item; ``None`` = numpy's global
    stream, i.e. exactly what the reference draws from.
    ``object_points="ids"``: the same draws, texts and (copied, flipped) poses, but the cell is NOT copied and no point is touched.
    ``item["cells"]`` / ``item["objects"]`` are the resident, UN-MIRRORED record and its objects; the flips are the item's ``mirror``
    code (bit 0: horizontal, x -> 1 - x; bit 1: vertical, y -> 1 - y), ``cell_row`` is the cell's row in ``all_cells``,
    ``object_rows`` i32[n_i] its objects' rows in ``packed()`` and ``draw_salts`` u32[n_i] = ``draw_salts(epoch, idx, n_i)``;
    ``object_points`` is None. ``coarse_batches`` turns such items into batches on the GPU; ``points=False`` leaves the point rows
    out of them (embedding mode reads none). Resident cost: 24 B per raw point of the split."""

    def __init__(self, base_path: str, scene_names: Sequence[str], object_points: Optional[str] = None, seed: int = 0,
                 transform: str = "fixed", shuffle_hints: bool = False, flip_poses: bool = False, aug_rng=None, points: bool = True):
        super().__init__(base_path, scene_names, object_points, transform, seed, points)
        self.shuffle_hints, self.flip_poses = bool(shuffle_hints), bool(flip_poses)
        self._aug = aug_rng if aug_rng is not None else np.random
        self._epoch_draw = 0
        self._pose_scene: List[str] = [s for s, _, poses in self._scenes for _ in poses]
        ids = [c.id for c in self.all_cells]
        if len(set(ids)) != len(ids):
            raise ValueError("cell ids repeat across scenes")  # cells.py:137-138
        self.cells_dict: Dict[str, CellRecord] = {c.id: c for c in self.all_cells}
        self._cell_row = {c.id: i for i, c in enumerate(self.all_cells)}

    def eval_texts(self) -> Optional[List[str]]:
        """Every item's ``texts`` in item order WITHOUT building the items — None when items are augmented (then the texts are a
        function of the draw and only ``__getitem__`` knows them). ``coarse.eval_epoch`` reads the queries from here instead of
        iterating the DataLoader: an evaluation item also carries its cell's point batch (cells.py:91-107), which the query side
        never looks at."""
        if self.shuffle_hints or self.flip_poses:
            return None
        return [" ".join(h) for h in self.hint_descriptions]

    def _draw(self, idx):
        """The augmentation draws of item ``idx`` in the reference's order — one ``choice`` over the hints (cells.py:80-81), then the
        two ``choice((True, False))`` (cells.py:86-90) — as (hints, their text with the flips' word swaps, flip code: bit 0 horizontal,
        bit 1 vertical). No draw depends on a flip, so flipping afterwards consumes ``aug_rng`` as flipping in between did."""
        hints = self.hint_descriptions[idx]
        if self.shuffle_hints:
            hints = self._aug.choice(hints, size=len(hints), replace=False)
        text, code = " ".join(hints), 0
        if self.flip_poses:
            for bit, a, b in ((1, "east", "west"), (2, "north", "south")):
                if self._aug.choice((True, False)):
                    code |= bit
                    text = _swap_words(text, a, b)
        return hints, text, code

    def __getitem__(self, idx):
        idx = int(idx)
        pose = self.all_poses[idx]
        cell = self.cells_dict[pose.cell_id]
        hints, text, code = self._draw(idx)
        if self._points == "ids":  # the flips are the code and a flipped POSE copy; the resident cell is not copied, no point touched
            if code:
                pose = _flipped_pose(pose, code)
            ps, row = self.packed(), self._cell_row[cell.id]
            lo, hi = int(ps.offsets[row]), int(ps.offsets[row + 1])
            return {"poses": pose, "cells": cell, "objects": cell.objects, "object_points": None, "texts": text,
                    "cell_ids": pose.cell_id, "scene_names": self._pose_scene[idx], "debug_hint_descriptions": hints,
                    "cell_row": row, "mirror": code, "object_rows": np.arange(lo, hi, dtype=np.int32),
                    "draw_salts": draw_salts(self._epoch, idx, hi - lo)}
        for bit, direction in ((1, 1), (2, -1)):
            if code & bit:
                pose, cell, _ = flip_pose_in_cell(pose, cell, "", direction)  # ``text`` carries its swaps already
        pts = None
        if self._points == "sample":
            if self._transform == "rotate_normalize":  # a fresh rotation / draw every time an item is fetched
                # keyed on (seed, cell, epoch, DataLoader worker, per-process counter): a worker process starts from a COPY of the
                # parent's counter every epoch, so the counter alone repeated the draws across epochs and collided across workers
                self._epoch_draw += 1
                wi = torch.utils.data.get_worker_info()
                rng = np.random.default_rng([self._seed, self._cell_row[cell.id], self._epoch, 0 if wi is None else wi.id + 1, self._epoch_draw])
            else:
                rng = np.random.default_rng([self._seed, self._cell_row[cell.id]])
            pts = packing.sample_object_points([cell.objects], 256, rng, transform=self._transform)[0]
        return {"poses": pose, "cells": cell, "objects": cell.objects, "object_points": pts, "texts": text,
                "cell_ids": pose.cell_id, "scene_names": self._pose_scene[idx], "debug_hint_descriptions": hints}

    def get_known_classes(self):
        return list(packing.KNOWN_CLASS)

    def get_cell_dataset(self) -> CellOnlyDataset:
        points = self._points if self._points != "ids" else ("sample" if self._ids_points else None)  # the eval path is not row-indexed
        return CellOnlyDataset(self.all_cells, points, self._seed, self._transform, self._packed_holder)  # one packed set for both

    def _device_batch(self, batch, engine, device):
        """``_batches``' GPU step: ``batch["objects"]`` names the cells' rows and flip codes; when the dataset wants points, all objects
        of the batch in one launch, each under its cell's code, cut into one view pair per cell."""
        ps, rows = self.packed(), batch["object_rows"]
        mirror = np.array(batch["mirror"], dtype=np.uint8)
        batch["objects"] = CoarseBatchObjects(batch["objects"], ps, rows, mirror)
        if self._ids_points:
            counts = [len(r) for r in rows]
            pos, col = ps.sample_rows(engine, device, np.concatenate(rows), np.concatenate(batch["draw_salts"]), seed=self.point_seed,
                                      transform=self.point_transform, mirror=np.repeat(mirror, counts))
            batch["object_points"] = _row_views(pos, col, counts)


# ---- the fine stage's dataset ---------------------------------------------------------------------------------------------------------
# regressor_cell x regressor_learn as load_pose_and_cell distinguishes them (poses.py:55-75); with "all" regressor_learn is not read
FINE_REGRESSORS = (("pose", "closest"), ("pose", "center"), ("best", "closest"), ("best", "center"), ("all", None))

_MAP_CLONING_REFUSAL = (
    "pmc_prob > 0 (prototype-based map cloning) is not built: in the reference the branch cannot run as published. Its rematching loop "
    "collects POSITIONS in cell.objects into new_matching (dataloading/kitti360pose/poses.py:427-433, 469-476), and "
    "load_pose_and_cell_aug2 then looks them up as keys of a dict keyed by obj.id (poses.py:180-183, 219-220); the "
    "direction/<scene>.json file the branch opens is written by datapreparation/kitti360pose/add_relation.py:71, whose json.dump call "
    "has its arguments swapped (the file object where the data belongs), so that script cannot write it. See DESIGN.md section 6.")


def _mix32(x):
    """lowbias32 (the sampler's mixer, include/t2l.h) on uint64 arrays holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, dtype=np.uint64) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def draw_salts(epoch: int, item: int, n_slots: int = 16) -> np.ndarray:
    """The salt of (epoch, item, slot), u32[n_slots]: ``mix(mix(mix(epoch + 0x9E3779B9) ^ item) ^ slot)`` with mix = lowbias32, all
    in 32 bits. ``t2l_sample_object_points_indexed`` draws slot s of the item under ``seed ^ salt``: every fetch of an object — in
    another slot, item or epoch — gets its own 256 indices (the reference redraws per fetch from numpy's global stream), and the
    same (seed, epoch) always gives the same batch. mix is a bijection, so the salts of one item's slots are pairwise different."""
    h = _mix32((int(epoch) + 0x9E3779B9) & 0xFFFFFFFF)
    h = _mix32(h ^ np.uint64(int(item) & 0xFFFFFFFF))
    return _mix32(h ^ np.arange(n_slots, dtype=np.uint64)).astype(np.uint32)


class Kitti360FineDataset(_PoseDataset):
    """One item per pose over several scenes: ``Kitti360FineDatasetMulti`` over ``Kitti360FineDataset`` (poses.py:368-590), an item
    being what ``load_pose_and_cell`` (poses.py:36-172) returns.

    ``args``: ``pad_size``, ``num_mentioned``, ``regressor_cell``, ``regressor_learn`` (``FINE_REGRESSORS``; the published command
    trains with regressor_cell = "all": the pose inside the cell). ``base_path``: a KITTI360Pose directory, or a dict
    ``{scene: (cells, poses)}`` of records already in memory (``from_records``).
    Objects of an item: the matched objects in hint order, then the cell's other objects in cell order, cut to ``pad_size`` or
    padded with ``cross_matcher.PadObject`` — the project's fixed pad, as in ``run_fine`` (the reference draws a pad's 8 points
    from numpy's global stream on every fetch).
    ``object_points``: ``None`` (embedding mode: no points); ``"sample"`` (the item's point batch from
    ``packing.sample_object_points`` on the host, redrawn per (seed, epoch, item)); ``"ids"`` (no points: ``object_rows``
    i32[pad_size], the objects' rows in ``packed()`` with ``pad_row`` for pads, and ``draw_salts`` u32[pad_size] — ``fine_batches``
    samples them on the GPU).
    ``flip_pose`` is accepted and does nothing: ``load_pose_and_cell`` never reads its ``flip_pose`` / ``horizontal_flip`` /
    ``vertical_flip`` arguments (poses.py:36-37 is their only mention), and training/fine.py:168 passes False."""

    def __init__(self, base_path, scene_names: Sequence[str], args, object_points: Optional[str] = None, transform: str = "fixed",
                 seed: int = 0, flip_pose: bool = False, pmc_prob: float = 0.0, pmc_threshold: float = 0.4, count_threshold: int = 1):
        super().__init__(base_path, scene_names, object_points, transform, int(seed))
        if pmc_prob > 0.0:
            raise NotImplementedError(_MAP_CLONING_REFUSAL)
        cell, learn = getattr(args, "regressor_cell", None), getattr(args, "regressor_learn", None)
        if (cell, None if cell == "all" else learn) not in FINE_REGRESSORS:
            raise ValueError(f"regressor_cell / regressor_learn must be one of {FINE_REGRESSORS}, got {(cell, learn)}")
        from .cross_matcher import PadObject

        self.args, self.pad_size = args, int(args.pad_size)
        self.flip_pose = bool(flip_pose)
        self._pad = PadObject()  # ONE pad object per dataset: its reductions are cached on it like any other object's
        self._pose_cell_row: List[int] = []
        first = 0
        for s, cells, poses in self._scenes:
            ids = [c.id for c in cells]
            if len(set(ids)) != len(ids):
                raise ValueError(f"{s}: cell ids repeat")  # base.py:45-46
            row = {c.id: first + i for i, c in enumerate(cells)}  # per scene, as the reference's per-scene cells_dict
            self._pose_cell_row.extend(row[p.cell_id] for p in poses)
            first += len(cells)
        self._positions: Dict[int, Dict[object, int]] = {}

    def get_known_classes(self) -> List[str]:
        """poses.py:583-587 over base.py:70-71: the sorted names of the class index ('pad' included)."""
        return sorted(CLASS_TO_INDEX)

    def _offsets(self, pose, cell):
        a, ds = self.args, pose.descriptions
        if a.regressor_cell == "all":  # poses.py:74-75: the pose inside the cell, x and y
            b = cell.bbox_w
            return np.array([(pose.pose_w[0] - b[0]) / (b[3] - b[0]), (pose.pose_w[1] - b[1]) / (b[4] - b[1])])
        kind = "offset_" + a.regressor_learn
        if a.regressor_cell == "pose":  # poses.py:55-58
            return np.array([getattr(d, kind) for d in ds])[:, 0:2]
        return np.array([getattr(d, "best_" + kind if d.is_matched else kind)[0:2] for d in ds])  # "best": poses.py:59-72

    def __getitem__(self, idx):
        idx = int(idx)
        pose, cell_row = self.all_poses[idx], self._pose_cell_row[idx]
        cell, hints, ds = self.all_cells[cell_row], self.hint_descriptions[idx], self.all_poses[idx].descriptions
        if len(ds) != self.args.num_mentioned:
            raise ValueError(f"pose {idx} carries {len(ds)} descriptions, args.num_mentioned is {self.args.num_mentioned}")
        where = self._positions.get(cell_row)
        if where is None:
            where = self._positions[cell_row] = {o.id: i for i, o in enumerate(cell.objects)}
        matched_ids = [d.object_id for d in ds if d.is_matched]
        # the matched objects in hint order, then the rest in cell order (poses.py:89-105); positions in cell.objects
        order = [where[i] for i in matched_ids] + [i for i, o in enumerate(cell.objects) if o.id not in matched_ids]
        if len(order) != len(cell.objects):
            raise ValueError(f"pose {idx}: two hints are matched to one object of cell {cell.id}")  # the reference asserts here
        matches = [(k, h) for k, h in enumerate(h for h, d in enumerate(ds) if d.is_matched)]
        order = order[:self.pad_size]  # poses.py:115-121
        objects = [cell.objects[i] for i in order] + [self._pad] * (self.pad_size - len(order))
        n_obj, n_hint = len(objects), len(ds)
        all_matches = list(matches)
        all_matches += [(n_obj, h) for h, d in enumerate(ds) if not d.is_matched]  # unmatched hints -> the objects' bin
        all_matches += [(k, n_hint) for k, o in enumerate(objects) if getattr(o, "id", -1) not in matched_ids]  # and vice versa
        item = {"poses": pose, "cells": cell, "objects": objects, "object_points": None, "hint_descriptions": hints,
                "texts": " ".join(hints), "matches": np.array(matches), "all_matches": np.array(all_matches),
                "offsets": self._offsets(pose, cell),
                "offsets_best_center": np.array([(d.best_offset_center if d.is_matched else d.offset_center)[0:2] for d in ds]),
                "object_class_indices": [CLASS_TO_INDEX[o.label] for o in objects],
                "object_color_indices": [packing.COLOR_NAMES.index(packing.COLOR_NAMES[packing.object_features(o)[1]]) for o in objects]}
        if self._points == "sample":
            rng = np.random.default_rng([self._seed, self._epoch, idx])
            item["object_points"] = packing.sample_object_points([objects], 256, rng, transform=self._transform)[0]
        elif self._points == "ids":
            ps = self.packed()
            base = int(ps.offsets[cell_row])
            item["object_rows"] = np.array([base + i for i in order] + [ps.pad_row] * (self.pad_size - len(order)), dtype=np.int32)
            item["draw_salts"] = draw_salts(self._epoch, idx, self.pad_size)
        return item

    def _device_batch(self, batch, engine, device):
        """``_batches``' GPU step: the batch's pad_size * B rows in one launch, cut into one view pair per pose."""
        pos, col = self.packed().sample_rows(engine, device, np.concatenate(batch["object_rows"]), np.concatenate(batch["draw_salts"]),
                                             seed=self.point_seed, transform=self.point_transform)
        batch["object_points"] = _row_views(pos, col, [self.pad_size] * len(batch["object_rows"]))


def fine_datasets_from_args(args, object_points: Optional[str] = "sample", seed: int = 0, scenes=None):
    """(train, val, test) as training/fine.py:153-187 builds them: the transforms from ``--no_pc_augment``
    (``packing.fine_train_transforms_from_args``: validation and test never rotate), the three scene lists of the KITTI360Pose split
    (``scenes``: other (train, val, test) lists), ``flip_pose=False``; ``args.pmc_prob`` goes to the training set alone, which
    refuses it above 0. ``object_points``: the point mode of all three (None with ``--class_embed``)."""
    train_t, val_t = packing.fine_train_transforms_from_args(args)
    tr, va, te = scenes if scenes is not None else (SCENE_NAMES_TRAIN, SCENE_NAMES_VAL, SCENE_NAMES_TEST)
    return (Kitti360FineDataset(args.base_path, tr, args, object_points, train_t, seed, flip_pose=False,
                                pmc_prob=float(getattr(args, "pmc_prob", 0.0)), pmc_threshold=float(getattr(args, "pmc_threshold", 0.4))),
            Kitti360FineDataset(args.base_path, va, args, object_points, val_t, seed),
            Kitti360FineDataset(args.base_path, te, args, object_points, val_t, seed))


def _checked_batch_size(who: str, batch_size) -> int:
    """What ``who`` (fine_batches / coarse_batches) refuses before anything else: a DataLoader worker, a batch size below 1."""
    if torch.utils.data.get_worker_info() is not None:
        raise RuntimeError(f"{who} works on the GPU and must run in the process that owns the engine, not in a DataLoader worker: let "
                           f"workers build host items (object_points='sample') or iterate {who} in the main process")
    if int(batch_size) <= 0:
        raise ValueError("batch_size must be positive")
    return int(batch_size)


def _checked_split(who: str, batch_size, rank, world):
    """``_checked_batch_size`` plus the data-parallel split: -> (batch_size, rank, world) as ints, or ValueError."""
    batch_size, rank, world = _checked_batch_size(who, batch_size), int(rank), int(world)
    if world < 1 or not 0 <= rank < world or batch_size % world:
        raise ValueError(f"{who}: need 0 <= rank < world and batch_size a multiple of world (every rank takes an equal slice of each "
                         f"batch), got rank={rank}, world={world}, batch_size={batch_size}")
    return batch_size, rank, world


def _row_views(pos, col, counts):
    """(pos, rgb) f32[n_rows,256,3] of ``sample_rows`` cut into per-item ``{"pos", "x"}`` views [counts[i] * 256, 3] of consecutive rows."""
    ends = np.cumsum(counts).tolist()
    return [{"pos": pos[e - c:e].reshape(-1, 3), "x": col[e - c:e].reshape(-1, 3)} for c, e in zip(counts, ends)]


def _batches(dataset: _PoseDataset, who: str, batch_size, device, shuffle, seed, epoch, drop_last, engine, rank=0, world=1):
    """The one batch loop behind ``fine_batches`` and ``coarse_batches`` (``who``): the items of ``dataset`` in the order of
    ``default_rng([seed, epoch])`` (``shuffle``) or as they lie, collated ``batch_size`` at a time; an ``object_points="ids"`` dataset
    then finishes each batch on ``device`` (``_device_batch``). ``engine`` None: the weightless engine the dataset keeps per device.
    ``rank`` of ``world``: the same global batches, of which this rank collates its contiguous slice."""
    batch_size, rank, world = _checked_split(who, batch_size, rank, world)
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(len(dataset)) if shuffle else np.arange(len(dataset))
    if dataset.point_mode == "ids" and dataset.wants_points and engine is None:
        from .plumbing import engine_for

        engine, _ = engine_for(getattr(dataset, "_sampler_engine", None), torch.device(device), who)
        dataset._sampler_engine = engine
    for lo in range(0, len(order), batch_size):
        chunk = order[lo:lo + batch_size]
        if drop_last and len(chunk) < batch_size:
            return
        if world > 1:
            if len(chunk) < world:  # a tail that cannot give every rank an item: all ranks leave it, so they take the same number of steps
                return
            chunk = chunk[rank * len(chunk) // world:(rank + 1) * len(chunk) // world]
        batch = dataset.collate_fn([dataset[int(i)] for i in chunk])
        if dataset.point_mode == "ids":
            dataset._device_batch(batch, engine, device)
        yield batch


def fine_batches(dataset: Kitti360FineDataset, batch_size: int, device, shuffle: bool = False, seed: int = 0, epoch: int = 0,
                 drop_last: bool = False, engine=None, rank: int = 0, world: int = 1):
    """One epoch of ``Kitti360FineDataset.collate_fn`` batches for ``fine_training.train_epoch`` / ``eval_epoch``. With an
    ``object_points="ids"`` dataset the batch's 16 * B point rows are sampled on ``device`` in ONE launch
    (``PackedCellSet.sample_rows``: slot s of item i under ``dataset.point_seed ^ draw_salts(epoch, i)[s]``) and
    ``batch["object_points"]`` holds per pose the ``{"pos", "x"}`` views [16 * 256, 3] ``CrossMatch`` accepts; the other two point
    modes are collated as they are. ``shuffle``: the permutation of ``default_rng([seed, epoch])``. The same (dataset seed, seed,
    epoch) always gives the same batches.
    GPU work belongs to the process that owns the engine: a DataLoader worker may build host items, it may not run this generator.
    ``engine``: the ``Engine`` to sample with (e.g. ``model.engine()``); without one the dataset keeps a weightless one per device.
    Data parallel (``rank`` of ``world``): ``batch_size`` is the GLOBAL one and must be a multiple of ``world``; every global batch is
    the one-process batch, of which rank r yields its contiguous slice — the same items, draw salts and flips, so the ranks' slices
    concatenate to the batch one process would have collated. A short last batch is split as evenly as it goes (and left out by all
    ranks when it has fewer items than ranks); ``drop_last`` keeps the shards equal, which the mean of the ranks' gradients assumes."""
    batch_size, rank, world = _checked_split("fine_batches", batch_size, rank, world)  # a refused call leaves the dataset's epoch alone
    dataset.set_epoch(epoch)
    yield from _batches(dataset, "fine_batches", batch_size, device, shuffle, seed, epoch, drop_last, engine, rank, world)


# ---- coarse training batches from the resident cell set -------------------------------------------------------------------------------
class CoarseBatchObjects(list):
    """``batch["objects"]`` of ``coarse_batches``: per cell the resident (un-mirrored) object list, as any collated batch holds — plus
    where those objects sit in the dataset's ``PackedCellSet`` (``cell_set``, ``object_rows``: one i32 array per cell) and each cell's
    flip code (``mirror`` u8[B]). ``plumbing.pack_objects`` gathers the packed cells from the set by them and never walks the lists."""

    def __init__(self, lists, cell_set, object_rows, mirror):
        super().__init__(lists)
        self.cell_set, self.object_rows, self.mirror = cell_set, object_rows, mirror


class CoarseBatches:
    """What ``coarse_batches`` returns: iterate it once per epoch, e.g. by handing it to ``coarse.train_epoch`` as the dataloader."""

    def __init__(self, dataset, batch_size, device, shuffle, seed, drop_last, engine):
        self.dataset, self.batch_size, self.device = dataset, batch_size, device
        self.shuffle, self.seed, self.drop_last, self.engine = shuffle, seed, drop_last, engine

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        # train_epoch has advanced the dataset's epoch; the items' salts read the same value
        return _batches(self.dataset, "coarse_batches", self.batch_size, self.device, self.shuffle, self.seed, self.dataset._epoch,
                        self.drop_last, self.engine)


def coarse_batches(dataset: Kitti360PoseDataset, batch_size: int, device, shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                   engine=None) -> CoarseBatches:
    """The batches of ``coarse.train_epoch`` in place of a DataLoader: a re-iterable with ``.dataset`` and ``__len__``. ``train_epoch``
    advances ``dataset.set_epoch`` itself; every ``__iter__`` reads the dataset's current epoch, shuffles by
    ``default_rng([seed, epoch])`` and collates the items. With an ``object_points="ids"`` dataset nothing of a cell is copied or
    uploaded: ``batch["objects"]`` (``CoarseBatchObjects``) names the cells' rows of the resident ``PackedCellSet`` and their flip
    codes, from which ``model.encode_objects`` gathers the packed features in one launch (t2l_gather_object_rows); when the dataset
    wants points, all objects of the batch are sampled in ONE launch (t2l_sample_object_points_mirrored: object row under
    ``dataset.point_seed ^ draw_salts(epoch, item)[slot]``, its cell's flip code, the dataset's transform — the rotation of
    "rotate_normalize" does not depend on the code) and ``batch["object_points"]`` holds the per-cell ``{"pos", "x"}`` views.
    The other point modes are collated as they are. The same (dataset seed, seed, epoch) always gives the same batches.
    GPU work belongs to the process that owns the engine: iterating inside a DataLoader worker raises.
    ``engine``: the ``Engine`` to sample with (e.g. ``model.engine()``); without one the dataset keeps a weightless one per device."""
    batch_size = _checked_batch_size("coarse_batches", batch_size)
    return CoarseBatches(dataset, batch_size, device, bool(shuffle), int(seed), bool(drop_last), engine)
