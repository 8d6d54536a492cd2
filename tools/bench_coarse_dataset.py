"""What a coarse training batch costs around the step, per batch, ``object_points="sample"`` (host items: flipped cells are deep
copies, points drawn per object with numpy) against ``object_points="ids"`` + ``coarse_batches`` (rows of the resident
``PackedCellSet``), in one process, at B = 64 with ``flip_poses`` and ``shuffle_hints`` on, published PointNet++ mode, transforms
"fixed" and "rotate_normalize", on two synthetic sets (``synth.make_k360_records``):

  heavy   ``--heavy-cells`` cells with KITTI360Pose's point counts (1,500-2,100 raw points per object: about 1 GB of float32 points per
          1,000 cells on the device, and as much again twice over for the float64 records on the host);
  wide    11,259 cells (the published database size) with 24-64 points per object, as profiles/fine_dataset.md used.

Per mode and transform:
  host_ms        items + collate (+ sampling): "sample" = ``collate_fn([ds[i] ...])`` with the host draws inside the items; "ids" =
                 one ``coarse_batches`` batch, the ONE sampler launch included (asynchronous: host time);
  pack_ms        ``plumbing.pack_objects`` on such a batch as the step calls it, device drained, and ``pack_bytes``, what it uploads:
                 "sample" re-uploads the raw points of the whole batch as soon as one cell is a flipped copy (its cached reductions are
                 gone) and reduces them again; "ids" uploads the row list (4 B per object + 1 B flip code + the offsets);
  batch_ms       host_ms + pack_ms, spreads added: the figure the two modes are compared by;
  sample_rows_ms / gather_rows_ms   device time of the two launches of the "ids" mode, by events;
  epoch_ms       wall time per batch of ``coarse.train_epoch`` over ``DataLoader(num_workers=0)`` ("sample") and over
                 ``coarse_batches`` ("ids"); step_ms beside them: device time of one training step on a resident batch, by events.

Every figure: the median over ``--reps`` repetitions of the mean over ``--iters`` batches with the spread (max - min) of the
repetitions; one more repetition runs first and is dropped. Prints one JSON line.

    python tools/bench_coarse_dataset.py [--batch 64] [--iters 20] [--reps 5] [--heavy-cells 1000] [--wide-cells 11259] [--sets heavy,wide]
"""
from __future__ import annotations

import argparse
import json
import os.path as osp
import sys
import time
import zlib

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2loc_amd import coarse, plumbing, synth  # noqa: E402
from text2loc_amd import kitti360pose as K  # noqa: E402

DEV = torch.device("cuda")
AUG = dict(shuffle_hints=True, flip_poses=True)


class HashText(torch.nn.Module):
    """Text-branch stand-in with a trainable table (the text branch is the same in both modes and not what is measured)."""

    def __init__(self, n=4096):
        super().__init__()
        self.table = torch.nn.Parameter(torch.randn(n, 256, generator=torch.Generator().manual_seed(1)))

    def forward(self, texts):
        return self.table[torch.as_tensor([zlib.crc32(t.encode()) % len(self.table) for t in texts], device=self.table.device)]

    @property
    def device(self):
        return self.table.device


def make_model(B):
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    args = argparse.Namespace(coarse_embed_dim=256, object_size=28, object_inter_module_num_heads=4, object_inter_module_num_layers=2,
                              hungging_model=None, fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4,
                              inter_module_num_layers=1, inter_module_num_heads=4, class_embed=False, color_embed=False,
                              pointnet_freeze=False, use_features=["class", "color", "position", "num"], ranking_loss="contrastive",
                              top_k=[1, 3, 5], threshs=[5, 10, 15], batch_size=B, temperature=0.1)
    model = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=HashText())
    sd = dict(synth.make_object_branch_weights(3))
    sd.update(synth.make_pointnet_weights(2))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    return model.to(DEV).train(), args


def med(values):
    return {"median": round(float(np.median(values)), 4), "spread": round(float(max(values) - min(values)), 4)}


def add(a, b):
    return {"median": round(a["median"] + b["median"], 4), "spread": round(a["spread"] + b["spread"], 4)}


def timed(make_iter, iters, reps, drain=False):
    """ms per batch: per repetition the mean over ``iters`` batches of a fresh iterator; the first repetition is dropped."""
    out = []
    for rep in range(reps + 1):
        it = make_iter(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            next(it)
        if drain:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return med(out[1:])


def host_batches(ds, B, seed, epoch):
    ds.set_epoch(epoch)
    order = np.random.default_rng([seed, epoch]).permutation(len(ds))
    for lo in range(0, len(order), B):
        yield K.Kitti360PoseDataset.collate_fn([ds[int(i)] for i in order[lo:lo + B]])


def pack_bytes(batch, mode):
    objs = [o for cell in batch["objects"] for o in cell]
    if mode == "ids":
        return 4 * (len(batch["objects"]) + 1) + 5 * len(objs)
    if any(getattr(o, "_t2l_feat", None) is None for o in objs):  # plumbing.pack_objects: then pack_cells_gpu for the whole batch
        return 24 * sum(len(o.xyz) for o in objs) + 4 * (len(batch["objects"]) + 1) + 4 * len(objs)
    return 4 * (len(batch["objects"]) + 1) + 36 * len(objs)


def timed_pack(model, batches, iters, reps, mode):
    eng, oe = model.engine(), model.object_encoder
    out, nbytes = [], []
    for rep in range(reps + 1):
        chunk = [next(batches) for _ in range(iters)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in chunk:
            plumbing.pack_objects(eng, b["objects"], oe, DEV)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
        nbytes.append(np.mean([pack_bytes(b, mode) for b in chunk]))
    return med(out[1:]), int(np.mean(nbytes[1:]))


def by_events(call, iters, reps):
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return med(out[1:])


def timed_epochs(model, args, loader, n_batches, reps):
    from text2loc_amd.losses import ContrastiveLoss
    from text2loc_amd.optim import Adam

    opt, crit = Adam(model, lr=1e-4), ContrastiveLoss(temperature=0.1)
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        coarse.train_epoch(model, loader, args, opt, crit)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / n_batches)
    return med(out[1:])


def step_ms(model, batch, iters, reps):
    from text2loc_amd.losses import ContrastiveLoss
    from text2loc_amd.optim import Adam

    opt, crit = Adam(model, lr=1e-4), ContrastiveLoss(temperature=0.1)

    def step():
        opt.zero_grad()
        loss = crit(model.encode_text(batch["texts"]), model.encode_objects(batch["objects"], batch["object_points"]))
        loss.backward()
        opt.step()

    return by_events(step, iters, reps)


def bench(name, cells, poses, B, iters, reps, transform):
    model, args = make_model(B)
    mk = lambda mode: K.Kitti360PoseDataset.from_records(cells, poses, object_points=mode, transform=transform, seed=3,  # noqa: E731
                                                         aug_rng=np.random.RandomState(5), **AUG)
    ds_s, ds_i = mk("sample"), mk("ids")
    ps = ds_i.packed()
    ps.on_device(DEV)
    ps.object_table(model.engine(), DEV, model.object_encoder.known_classes, model.object_encoder.known_colors)  # resident before timing
    torch.cuda.synchronize()
    ids_iter = lambda r, seed=1: iter(K.coarse_batches(_at(ds_i, r), B, DEV, shuffle=True, seed=seed, engine=model.engine()))  # noqa: E731
    row = {"set": name, "transform": transform, "B": B, "cells": len(cells), "objects": ps.n_objects, "points": ps.n_points,
           "resident_MB": round(24 * ps.n_points / 2 ** 20, 1)}
    s_host = timed(lambda r: host_batches(ds_s, B, 1, r), iters, reps)
    i_host = timed(ids_iter, iters, reps)
    i_wall = timed(ids_iter, iters, reps, drain=True)
    s_pack, s_bytes = timed_pack(model, _cycle(lambda e: host_batches(ds_s, B, 7, e)), iters, reps, "sample")
    i_pack, i_bytes = timed_pack(model, _cycle(lambda e: ids_iter(e, 7)), iters, reps, "ids")
    row["sample"] = {"host_ms": s_host, "pack_ms": s_pack, "pack_bytes": s_bytes, "batch_ms": add(s_host, s_pack)}
    row["ids"] = {"host_ms": i_host, "host_drained_ms": i_wall, "pack_ms": i_pack, "pack_bytes": i_bytes, "batch_ms": add(i_host, i_pack)}
    b = next(ids_iter(9))
    rows, salts = np.concatenate(b["object_rows"]), np.concatenate(b["draw_salts"])
    mirror = np.repeat(b["objects"].mirror, [len(r) for r in b["object_rows"]])
    eng, oe = model.engine(), model.object_encoder
    row["rows_per_launch"] = int(len(rows))
    row["sample_rows_ms"] = by_events(lambda: ps.sample_rows(eng, DEV, rows, salts, seed=3, transform=transform, mirror=mirror), iters, reps)
    row["gather_rows_ms"] = by_events(lambda: eng.gather_object_rows(ps.object_table(eng, DEV, oe.known_classes, oe.known_colors), rows, mirror),
                                      iters, reps)
    row["step_ms"] = step_ms(model, b, iters, reps)
    n_batches = len(poses) // B
    loader = torch.utils.data.DataLoader(ds_s, batch_size=B, shuffle=True, num_workers=0, drop_last=True,
                                         collate_fn=K.Kitti360PoseDataset.collate_fn)
    row["sample"]["epoch_ms"] = timed_epochs(model, args, loader, n_batches, reps)
    row["ids"]["epoch_ms"] = timed_epochs(model, args, K.coarse_batches(ds_i, B, DEV, shuffle=True, seed=1, drop_last=True, engine=eng),
                                          n_batches, reps)
    gap = row["sample"]["batch_ms"]["median"] - row["ids"]["batch_ms"]["median"]
    row["ids_below_sample_by_more_than_both_spreads"] = bool(gap > row["sample"]["batch_ms"]["spread"] + row["ids"]["batch_ms"]["spread"])
    ps.release_device()
    return row


def _at(ds, epoch):
    ds.set_epoch(epoch)
    return ds


def _cycle(make):
    epoch = 0
    while True:
        yield from make(epoch)
        epoch += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--heavy-cells", type=int, default=1000)
    ap.add_argument("--wide-cells", type=int, default=11259)
    ap.add_argument("--sets", default="heavy,wide")
    ap.add_argument("--transforms", default="fixed,rotate_normalize")
    a = ap.parse_args()
    torch.manual_seed(0)
    n_poses = a.batch * a.iters  # an epoch of the shuffled set serves the --iters batches of a repetition
    rows = []
    for name in a.sets.split(","):
        n_cells, ppo = (a.heavy_cells, (1500, 2100)) if name == "heavy" else (a.wide_cells, (24, 64))
        t0 = time.perf_counter()
        cells, poses = synth.make_k360_records(n_cells, n_poses, seed=0, pts_per_obj=ppo)
        built = round(time.perf_counter() - t0, 1)
        for transform in a.transforms.split(","):
            row = bench(name, cells, poses, a.batch, a.iters, a.reps, transform)
            row["records_built_s"] = built
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del cells, poses
    print(json.dumps({"metric": "coarse batch production per batch, host items ('sample') vs rows of the resident cell set ('ids'), beside the "
                                "training step", "unit": "ms/batch", "poses": n_poses, "iters": a.iters, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
