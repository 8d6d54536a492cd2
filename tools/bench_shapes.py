"""ms per `t2l_encode_cells` over the 11,259-cell synthetic database at each compiled shape of the cell encoder, beside the
published shape on the one-cell kernel (`encoder_two_cells = 0`: the <256, 64> instance with object_size 28) measured in the SAME
run — the baseline every ratio in the table is taken against — and its default two-cell kernel for orientation.

Kernel time comes from the library's device events around the launch (`profile_events = 1`, `Engine.kernel_stats("encode_cells")`).
Every case is warmed up (`--warmup` calls), then timed `--reps` times over `--iters` calls each; the cases are ALTERNATED inside
every repetition, so drift of the machine lands on all of them alike. Reported: the median and the spread (min .. max) of the
per-repetition means, the ratio of medians to the baseline, and the MFMA work of one cell relative to the published shape
(counted from the shapes: projections and feed-forward ~ D^2, attention core ~ 32 * 32 * D).

    python tools/bench_shapes.py [--cells 11259] [--iters 20] [--warmup 5] [--reps 7] [--f32 | --f16] [--markdown OUT.md]

`--f16` sets option `encoder_f16`, which acts on the two published rows only. `T2L_LIB=path/to/libt2l.so` in the environment times
another build of the library (engine.py).
Prints one JSON line; `--markdown` also writes the table. Bar (asserted, exit status 1): the (128, 4 heads) split-f16 time must
not exceed the baseline's — a quarter of the D^2 work on the same 32-row tiles; it catches a non-MFMA or badly occupied kernel.
"""
from __future__ import annotations

import argparse
import json
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from text2loc_amd import synth  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402

# (label, D, heads, layers, object_size, encoder_two_cells)
CASES = [
    ("published one-cell (baseline)", 256, 4, 2, 28, 0),
    ("published two-cell (default)", 256, 4, 2, 28, 1),
    ("D=128 h=4 S=28", 128, 4, 2, 28, 0),
    ("D=128 h=2 S=28", 128, 2, 2, 28, 0),
    ("D=128 h=2 L=3 S=20", 128, 2, 3, 20, 0),
    ("D=256 h=8 S=28", 256, 8, 2, 28, 0),
    ("D=256 h=8 L=1 S=32", 256, 8, 1, 32, 0),
    ("D=256 h=4 S=24", 256, 4, 2, 24, 0),
    ("D=256 h=4 S=32", 256, 4, 2, 32, 0),
]


def mfma_work(D, layers, nfeat=4):
    """Multiply-adds per cell on 32-row tiles: merge + per layer (q/k/v, out_proj, two feed-forward products, S and P V)."""
    return 32 * (nfeat * D * D + layers * (3 * D * D + D * D + 4 * D * D + 2 * 32 * D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=11259)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    arith = ap.add_mutually_exclusive_group()
    arith.add_argument("--f32", action="store_true", help="the all-f32 instances (option encoder_f32) instead of split-f16")
    arith.add_argument("--f16", action="store_true", help="plain f16 (option encoder_f16) at the published shape")
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shapes.py measures on the GPU; there is nothing to time without one")
    cells = synth.make_cells(a.cells, seed=4)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    engines = []
    for label, D, heads, layers, osz, two in CASES:  # one context per case: no weight re-load inside the timed loop
        e = Engine(0)
        e.set_option("profile_events", 1)
        e.set_option("encoder_f32", 1 if a.f32 else 0)
        e.set_option("encoder_f16", 1 if a.f16 else 0)
        e.set_option("encoder_two_cells", two)
        sd = synth.make_object_branch_weights(0, embed_dim=D, num_layers=layers)
        e.load_weights(sd, class_embed=True, color_embed=True, num_layers=layers, num_heads=heads, embed_dim=D, object_size=osz)
        for _ in range(a.warmup):
            e.encode_cells(packed)
        torch.cuda.synchronize()
        e.kernel_stats("encode_cells")  # drop the warm-up launches
        engines.append(e)
    per_rep = [[] for _ in CASES]
    for _ in range(a.reps):
        for i, e in enumerate(engines):  # alternate the cases inside every repetition
            for _ in range(a.iters):
                e.encode_cells(packed)
            torch.cuda.synchronize()
            ms, n = e.kernel_stats("encode_cells")
            assert n == a.iters, (n, a.iters)
            per_rep[i].append(ms)
    for e in engines:
        e.close()
    base = float(np.median(per_rep[0]))
    pub_work = mfma_work(256, 2)
    rows = []
    for (label, D, heads, layers, osz, two), t in zip(CASES, per_rep):
        med = float(np.median(t))
        rows.append(dict(case=label, embed_dim=D, heads=heads, layers=layers, object_size=osz, ms=round(med, 4),
                         ms_min=round(float(min(t)), 4), ms_max=round(float(max(t)), 4), ratio_to_baseline=round(med / base, 3),
                         mfma_work_ratio=round(mfma_work(D, layers) / pub_work, 3)))
    ok = rows[2]["ms"] <= rows[0]["ms"]
    out = dict(tool="bench_shapes", cells=a.cells, iters=a.iters, reps=a.reps, arithmetic="f32" if a.f32 else "plain-f16" if a.f16 else "split-f16",
               device=torch.cuda.get_device_name(0), rows=rows, d128_bar_holds=bool(ok))
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(f"| case | ms / {a.cells} cells (median of {a.reps} x {a.iters}) | min .. max | ratio to baseline | MFMA work ratio |\n")
            f.write("|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['case']} | {r['ms']:.3f} | {r['ms_min']:.3f} .. {r['ms_max']:.3f} | {r['ratio_to_baseline']:.2f} | "
                        f"{r['mfma_work_ratio']:.2f} |\n")
    print(json.dumps(out))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
