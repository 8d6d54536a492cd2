"""What a fine-stage training batch costs BEFORE the step, per batch, on a synthetic KITTI360Pose set of the published size
(``synth.make_k360_records``: 11,259 cells, 24-64 raw points per object — the real mean is 1,827, which neither sampler's cost depends
on: both draw 256 indices per object whatever its size), at B = 32 and B = 256:

  host_sample_ms   ``Kitti360FineDataset(object_points="sample")``: items + collate, the points drawn on the host per object
                   (``packing.sample_object_points``: the only way before ``"ids"``), wall time per batch in this process;
  host_upload_ms   what the step then does with those batches first: concatenate and copy them over (``plumbing.point_batch_tensors``);
  ids_host_ms      ``object_points="ids"`` + ``fine_batches``: items + collate + the ONE launch, host time per batch (the launch is
                   asynchronous; ``ids_wall_ms`` is the same loop with the device drained at the end of the 20 batches);
  sample_rows_ms   device time of that launch (the row sampler over 16 * B rows, no mirror codes), by events;
  pack_first_ms /  ``plumbing.pack_objects`` on a batch's objects, the first time that batch is packed and again. An item's colour indices
  pack_again_ms    already put every object's reductions into the host cache (``packing.object_features``), so neither goes through
                   t2l_reduce_objects here: both are the host packing of cached values plus their copy;
  item_ms          building one item without points (the list work both modes share): the first touch of its objects, which caches
                   their reductions on them, and a later touch;
  step_ms          the full published-mode training step beside them (``tools/bench_fine_train.py --points``: bench_points).

Every figure is the median over ``--reps`` repetitions of the mean over ``--iters`` batches, with the spread (max - min) of the
repetitions. Prints one JSON line.

    python tools/bench_fine_dataset.py [--batches 32,256] [--iters 20] [--reps 5] [--cells 11259]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os.path as osp
import sys
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2loc_amd import kitti360pose as K  # noqa: E402
from text2loc_amd import plumbing, synth  # noqa: E402


def fine_records(n_cells, n_poses, seed=0):
    """``make_k360_records`` plus the fields of a matched ``DescriptionBestCell`` the fine items read (every hint matched: its
    object is one of the cell's; offsets relative to the object's centre)."""
    cells, poses = synth.make_k360_records(n_cells, n_poses, seed=seed)
    for p in poses:
        for d in p.descriptions:
            off = np.asarray(p.pose[:2] - d.closest_point[:2], dtype=np.float64)
            d.__dict__.update(is_matched=True, object_instance_id=d.object_id, offset_center=off, offset_closest=off,
                              best_offset_center=off, best_offset_closest=off)
    return cells, poses


def med(values):
    return {"median": round(float(np.median(values)), 4), "spread": round(float(max(values) - min(values)), 4)}


def timed_batches(make_iter, iters, reps, drain):
    """ms per batch: per repetition the mean over ``iters`` batches of a fresh iterator; ``drain``: wait for the device at the end."""
    out = []
    for rep in range(reps):
        it = make_iter(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            next(it)
        if drain:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def bench(cells, poses, B, iters, reps, model, bench_points):
    args = argparse.Namespace(pad_size=16, num_mentioned=6, regressor_cell="all", regressor_learn="center")
    ds_s = K.Kitti360FineDataset.from_records(cells, poses, args, object_points="sample")
    ds_i = K.Kitti360FineDataset.from_records(cells, poses, args, object_points="ids")
    ps = ds_i.packed()
    ps.on_device("cuda")
    # both datasets share the records: touch every item once, so that neither loop pays the per-object reductions an item's colour
    # indices need (packing.object_features caches them on the object — the first epoch of either mode pays them once)
    ds_n = K.Kitti360FineDataset.from_records(cells, poses, args)
    t0 = time.perf_counter()
    for i in range(len(ds_n)):
        ds_n[i]
    first_pass = (time.perf_counter() - t0) * 1e3 / len(ds_n)
    t0 = time.perf_counter()
    for i in range(len(ds_n)):
        ds_n[i]
    row_items = {"first_touch_ms_per_item": round(first_pass, 4), "later_ms_per_item": round((time.perf_counter() - t0) * 1e3 / len(ds_n), 4)}
    row = {"B": B, "rows_per_launch": 16 * B, "item_ms": row_items}
    # the first repetition of each loop is a warm-up (page faults, the engine's staging buffer, the allocator) and is dropped
    row["host_sample_ms"] = med(timed_batches(lambda r: K.fine_batches(ds_s, B, "cuda", shuffle=True, seed=1, epoch=r), iters, reps + 1, False)[1:])
    row["ids_host_ms"] = med(timed_batches(lambda r: K.fine_batches(ds_i, B, "cuda", shuffle=True, seed=1, epoch=r), iters, reps + 1, False)[1:])
    row["ids_wall_ms"] = med(timed_batches(lambda r: K.fine_batches(ds_i, B, "cuda", shuffle=True, seed=1, epoch=r), iters, reps + 1, True)[1:])
    batch_s = next(K.fine_batches(ds_s, B, "cuda", shuffle=True, seed=1, epoch=9))
    up = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            plumbing.point_batch_tensors(batch_s["object_points"], True, torch.device("cuda"))
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3 / iters)
    row["host_upload_ms"] = med(up[1:])
    batch_i = next(K.fine_batches(ds_i, B, "cuda", shuffle=True, seed=1, epoch=9))
    rows, salts = np.concatenate(batch_i["object_rows"]), np.concatenate(batch_i["draw_salts"])
    eng = ds_i._sampler_engine
    dev = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ps.sample_rows(eng, "cuda", rows, salts, seed=0)
        b.record()
        torch.cuda.synchronize()
        dev.append(a.elapsed_time(b) / iters)
    row["sample_rows_ms"] = med(dev[1:])
    # pack_objects: a batch packed for the first time, then the same batch again and again
    eng_m = model.engine() if hasattr(model, "engine") else eng
    first, again = [], []
    fresh = K.fine_batches(ds_i, B, "cuda", shuffle=True, seed=7, epoch=3)
    for _ in range(reps + 1):
        b = next(fresh)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plumbing.pack_objects(eng_m, b["objects"], model.object_encoder, torch.device("cuda"))
        torch.cuda.synchronize()
        first.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(iters):
            plumbing.pack_objects(eng_m, b["objects"], model.object_encoder, torch.device("cuda"))
        torch.cuda.synchronize()
        again.append((time.perf_counter() - t0) * 1e3 / iters)
    row["pack_first_ms"], row["pack_again_ms"] = med(first[1:]), med(again[1:])
    step = bench_points(B, iters, 10, reps)
    row["step_ms"] = {"median": step["ms_engine"], "spread": step["spread_ms"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=11259)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("bench_fine_train", osp.join(ROOT, "tools", "bench_fine_train.py"))
    bft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bft)
    from text2loc_amd.cross_matcher import CrossMatch

    torch.manual_seed(0)
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, bft.make_args(False), language_encoder=torch.nn.Identity())
    sd = dict(synth.make_fine_weights(0))
    sd.update(synth.make_pointnet_weights(0))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda().train()
    batches = [int(b) for b in a.batches.split(",")]
    n_poses = max(batches) * a.iters  # an epoch of the shuffled set serves the --iters batches of a repetition
    t0 = time.perf_counter()
    cells, poses = fine_records(a.cells, n_poses)
    built = time.perf_counter() - t0
    rows = [bench(cells, poses, B, a.iters, a.reps, model, bft.bench_points) for B in batches]
    print(json.dumps({"metric": "fine-stage batch production per batch, host sampling vs rows sampled on the device, beside the training step",
                      "unit": "ms/batch", "cells": a.cells, "poses": n_poses, "records_built_s": round(built, 1), "iters": a.iters,
                      "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
