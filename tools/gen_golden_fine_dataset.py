"""TEST INFRASTRUCTURE — build-container only (needs the reference tree).

Writes a tiny KITTI360Pose directory for the FINE stage with the reference's own classes — ``Cell / Object3d / Pose /
DescriptionPoseCell / DescriptionBestCell.from_matched / from_unmatched`` pickled as ``datapreparation`` leaves them on disk — into
``tests/golden/k360_fine_tiny/{cells,poses}/<scene>.pkl``, and next to it ``k360_fine_tiny.npz``: what the reference's own
``Kitti360FineDatasetMulti`` (dataloading/kitti360pose/poses.py:528-587) returns for every item under each of the five
regressor_cell x regressor_learn settings ``load_pose_and_cell`` distinguishes — everything but the randomly drawn points: object ids
and labels in order (pads: id -1, label 'pad'), texts, hint sentences, matches, all_matches, offsets, offsets_best_center and the two
index lists. Two scenes; cells of 3 to 20 objects (padding and the cut at 16 both occur); at most 60 points per object; poses with
0, 1, 3 and 6 matched hints out of 6; one pose whose matched object sits at position 18 of its 20-object cell.
The pickles and the arrays are DATA; tests/test_fine_dataset_cpu.py reads them with text2loc_amd.kitti360pose — no reference on
sys.path. Re-run: ``python tools/gen_golden_fine_dataset.py`` (deterministic).
"""
from __future__ import annotations

import argparse
import os
import os.path as osp
import pickle
import shutil
import sys

import numpy as np

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(REPO, "oracle"))
sys.path.insert(0, REPO)
import ref_harness as H  # noqa: E402

H.setup_reference_imports()

from text2loc_amd import synth  # noqa: E402

OUT = osp.join(REPO, "tests", "golden", "k360_fine_tiny")
SCENES = ["2013_05_28_drive_0010_sync", "2013_05_28_drive_0003_sync"]
COUNTS = [[3, 20, 7, 16], [17, 5, 12]]  # objects per cell
# per pose: (cell, matched hints out of 6, position in cell.objects the FIRST matched hint must use, or None)
POSES = [[(0, 0, None), (1, 1, 18), (1, 6, None), (2, 3, None), (3, 6, None), (0, 1, None)],
         [(0, 3, None), (1, 0, None), (2, 6, None), (0, 1, 16), (1, 3, None)]]
SETTINGS = [("pose", "closest"), ("pose", "center"), ("best", "closest"), ("best", "center"), ("all", "center")]
DIRECTIONS = ["north", "south", "east", "west", "on-top"]
PAD, NH, CELL_SIZE = 16, 6, 30.0


def write_scene(si, scene):
    from datapreparation.kitti360pose.imports import Cell, DescriptionBestCell, DescriptionPoseCell, Pose

    rng = np.random.default_rng([si, 0xF19E])
    counts = COUNTS[si]
    cn = synth.make_cells(len(counts), seed=70 + si, min_obj=20, max_obj=20)
    cn["n_pts"] = np.minimum(cn["n_pts"], 60).astype(np.float32)
    objects = [objs[:n] for objs, n in zip(H.build_objects(cn, seed=70 + si), counts)]
    short = scene.split("_")[-2]
    cells = []
    for i, objs in enumerate(objects):
        lo = np.array([i * CELL_SIZE / 2.0, si * CELL_SIZE, 0.0])
        cells.append(Cell(i, short, objs, CELL_SIZE, np.hstack((lo, lo + CELL_SIZE))))
    poses = []
    for ci, n_matched, first in POSES[si]:
        cell = cells[ci]
        other = cells[(ci + 1) % len(cells)]  # the "pose cell" an unmatched hint's object comes from
        pin = rng.uniform(0.3, 0.7, size=3)
        picks = [int(p) for p in rng.permutation(len(cell.objects))]
        if first is not None:
            picks.remove(first)
            picks.insert(0, first)
        descs = []
        for h in range(NH):
            matched = h < n_matched
            obj = cell.objects[picks[h]] if matched else other.objects[int(rng.integers(0, len(other.objects)))]
            closest = obj.get_closest_point(pin)
            d = DescriptionPoseCell(obj, DIRECTIONS[int(rng.integers(0, 5))], pin - obj.get_center(), pin - closest, closest)
            if matched:  # the best cell sees the object a little elsewhere than the pose cell did
                shift = rng.normal(0, 0.02, size=3)
                descs.append(DescriptionBestCell.from_matched(d, obj.id, closest + shift, pin - obj.get_center() - shift, pin - closest - shift))
            else:
                descs.append(DescriptionBestCell.from_unmatched(d))
        order = rng.permutation(NH)  # matched and unmatched hints interleaved
        poses.append(Pose(pin, cell.bbox_w[0:3] + pin * CELL_SIZE, cell.id, short, [descs[int(k)] for k in order]))
    os.makedirs(osp.join(OUT, "cells"), exist_ok=True)
    os.makedirs(osp.join(OUT, "poses"), exist_ok=True)
    pickle.dump(cells, open(osp.join(OUT, "cells", scene + ".pkl"), "wb"))
    pickle.dump(poses, open(osp.join(OUT, "poses", scene + ".pkl"), "wb"))


def main():
    import torch_geometric.transforms as T
    from dataloading.kitti360pose.poses import Kitti360FineDatasetMulti

    shutil.rmtree(OUT, ignore_errors=True)
    for si, scene in enumerate(SCENES):
        write_scene(si, scene)
    arrays = {"scenes": np.array(SCENES), "settings": np.array(["/".join(s) for s in SETTINGS]), "pad_size": PAD, "num_mentioned": NH}
    for k, (cell, learn) in enumerate(SETTINGS):
        args = argparse.Namespace(pad_size=PAD, num_mentioned=NH, regressor_cell=cell, regressor_learn=learn)
        ds = Kitti360FineDatasetMulti(OUT, SCENES, T.FixedPoints(256), args)
        items = [ds[i] for i in range(len(ds))]
        p = f"r{k}_"
        arrays[p + "object_ids"] = np.array([[o.id for o in it["objects"]] for it in items], dtype=np.int64)
        arrays[p + "object_labels"] = np.array([[o.label for o in it["objects"]] for it in items])
        arrays[p + "object_npts"] = np.array([[len(o.xyz) for o in it["objects"]] for it in items], dtype=np.int64)
        arrays[p + "texts"] = np.array([it["texts"] for it in items])
        arrays[p + "hint_descriptions"] = np.array([list(it["hint_descriptions"]) for it in items])
        arrays[p + "matches_n"] = np.array([len(it["matches"]) for it in items], dtype=np.int64)
        arrays[p + "matches"] = np.concatenate([np.asarray(it["matches"], dtype=np.int64).reshape(-1, 2) for it in items])
        arrays[p + "all_matches_n"] = np.array([len(it["all_matches"]) for it in items], dtype=np.int64)
        arrays[p + "all_matches"] = np.concatenate([np.asarray(it["all_matches"], dtype=np.int64).reshape(-1, 2) for it in items])
        arrays[p + "offsets"] = np.array([it["offsets"] for it in items], dtype=np.float64)
        arrays[p + "offsets_best_center"] = np.array([it["offsets_best_center"] for it in items], dtype=np.float64)
        arrays[p + "object_class_indices"] = np.array([it["object_class_indices"] for it in items], dtype=np.int64)
        arrays[p + "object_color_indices"] = np.array([it["object_color_indices"] for it in items], dtype=np.int64)
        arrays[p + "pose_cell_ids"] = np.array([it["poses"].cell_id for it in items])
        arrays[p + "pose_in_cell"] = np.array([it["poses"].pose for it in items], dtype=np.float64)
        if k == 0:
            arrays["known_classes"] = np.array([str(c) for c in ds.get_known_classes()])
            arrays["cell_counts"] = np.array([len(c.objects) for c in ds.all_cells], dtype=np.int64)
    np.savez_compressed(osp.join(osp.dirname(OUT), "k360_fine_tiny.npz"), **arrays)
    print("wrote", OUT, "items", len(items), "matched per item", arrays["r0_matches_n"].tolist())


if __name__ == "__main__":
    main()
