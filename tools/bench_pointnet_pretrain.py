"""ms per step of the PointNet++ backbone's pretraining as a classifier (text2loc_amd/pointnet_pretrain.py), device events around
`--iters` steps after `--warmup` steps; the median of `--reps` repetitions and their spread (max - min). Prints one JSON line.

`--mode step` (default): the full step on the engine — ``PointNet2.forward`` under ``train()`` (t2l_pointnet_cls_forward, the batch
as ONE BatchNorm segment), ``ClassifierLoss`` (t2l_pointnet_cls_heads: forward-only at the loss, forward + backward in ONE launch at
``backward()``), t2l_pointnet_cls_backward, ``torch.optim.Adam``. The backbone has no torch form on this machine (the reference's
needs torch_geometric), so there is no PyTorch column for the full step.

`--mode heads`: the heads and their loss alone, forward + backward, on the same features2 [B,256]: the engine's one launch against
the same graph as torch ops (two ``F.linear``, two ``F.cross_entropy``, ``backward()``), same weights and labels.

`--mode segments --segments S`: the backbone's training-mode forward + backward alone (t2l_pointnet_features_train /
t2l_pointnet_backward) with the same B objects cut into S BatchNorm segments (S = 1: what the pretraining step runs; S = B: one
object per segment) — for a kernel trace of the ``pt_bn_*`` kernels under both layouts of their float64 accumulator rows.

    python tools/bench_pointnet_pretrain.py [--mode step|heads|segments] [--batch 64] [--segments 1] [--iters 10] [--warmup 3] [--reps 3]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_pointnet_pretrain.py --mode step --iters 5 --warmup 2 --reps 1
"""
from __future__ import annotations

import argparse
import json
import os.path as osp
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from text2loc_amd import synth  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402
from text2loc_amd.pointnet_pretrain import ClassifierLoss, PointNet2  # noqa: E402

P = "object_encoder.pointnet."


def problem(B):
    cells = synth.make_cells(1, seed=1, min_obj=B, max_obj=B)
    pos, rgb = synth.make_sampled_points(cells, 2)
    rng = np.random.default_rng(3)
    return (torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), synth.make_pointnet_weights(0),
            rng.integers(0, 22, B).astype(np.int32), rng.integers(0, 8, B).astype(np.int32))


def timed(step, iters, warmup, reps):
    """-> (median ms per step over the repetitions, spread max - min)."""
    for _ in range(warmup):
        step()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(max(ms) - min(ms))


def mode_step(a):
    pos, rgb, sd, lc, lk = problem(a.batch)
    model = PointNet2(22, 8)
    model.load_state_dict({k[len(P):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda().train()
    opt, crit = torch.optim.Adam(model.parameters(), lr=1e-3), ClassifierLoss()
    batch = {"pos": pos, "x": rgb}

    def step():
        opt.zero_grad()
        crit(model(batch), lc, lk).backward()
        opt.step()

    torch.cuda.reset_peak_memory_stats()
    ms, spread = timed(step, a.iters, a.warmup, a.reps)
    return {"engine_ms": ms, "engine_spread_ms": spread}


def mode_heads(a):
    B = a.batch
    _, _, sd, lc, lk = problem(B)
    x = torch.from_numpy(np.abs(np.random.default_rng(4).standard_normal((B, 256))).astype(np.float32)).cuda()
    eng = Engine(0)
    tensors = {}
    for k, v in sd.items():
        if not k.endswith("num_batches_tracked"):
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.pointnet_cls_bind(tensors)
    e_ms, e_sp = timed(lambda: eng.pointnet_cls_heads(x, lc, lk, need_logits=False), a.iters, a.warmup, a.reps)
    params = [tensors[P + h + s][0].clone().requires_grad_(True) for h in ("class_classifier", "color_classifier") for s in (".weight", ".bias")]
    tc, tk = torch.from_numpy(lc).long().cuda(), torch.from_numpy(lk).long().cuda()
    xt = x.clone().requires_grad_(True)

    def torch_step():
        for p in params + [xt]:
            p.grad = None
        loss = F.cross_entropy(F.linear(xt, params[0], params[1]), tc) + F.cross_entropy(F.linear(xt, params[2], params[3]), tk)
        loss.backward()

    t_ms, t_sp = timed(torch_step, a.iters, a.warmup, a.reps)
    eng.close()
    return {"engine_ms": e_ms, "engine_spread_ms": e_sp, "torch_ms": t_ms, "torch_spread_ms": t_sp}


def mode_segments(a):
    B, S = a.batch, a.segments
    if B % S:
        raise SystemExit("--segments must divide --batch")
    pos, rgb, sd, _, _ = problem(B)
    eng = Engine(0)
    tensors = {}
    for k, v in list(synth.make_object_branch_weights(2).items()) + list(sd.items()):
        if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight") or "classifier" in k:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tensors[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tensors, class_embed=False, color_embed=False)
    offs = np.arange(0, B + 1, B // S, dtype=np.int32)
    g = torch.randn(B, 256, device="cuda")

    def step():
        eng.pointnet_features_train(pos, rgb, offs)
        eng.pointnet_backward(g)

    ms, spread = timed(step, a.iters, a.warmup, a.reps)
    eng.close()
    return {"engine_ms": ms, "engine_spread_ms": spread, "segments": S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "heads", "segments"], default="step")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--segments", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = {"mode": a.mode, "batch": a.batch, "iters": a.iters, "warmup": a.warmup, "reps": a.reps}
    out.update({"step": mode_step, "heads": mode_heads, "segments": mode_segments}[a.mode](a))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
