#!/usr/bin/env python3
"""What the engine path of PairwiseRankingLoss / HardestRankingLoss costs beside the torch formulation (the parent behaviour).

    python tools/bench_ranking_loss.py [--calls 300] [--repeats 3] [--steps 60] [--out profiles/ranking_loss.json]
    python tools/bench_ranking_loss.py --bars        # no GPU: the float32 CPU mirror vs float64, the table behind RANK_T

Per call: forward + backward through the module (``loss = crit(im, s); loss.backward()``) on [B,256] leaves, device events around
``--calls`` calls after a warm-up of every shape, engine and ``use_engine = False`` alternated in the same process, the whole run
repeated ``--repeats`` times to show the spread. B = 32 (the reference's --batch_size default), 64, 128, and 512 as a global batch.
Full step: the loop of ``bench.full_train_step_measure`` at B = 64 (engine text head, split-bf16 GEMMs) with the criterion swapped
for the pairwise module, wall clock per step. Prints one JSON document."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def bars():
    from tests import ranking_loss_ref as R

    rows = R.bars_table()
    print("| kind | B | a | margin | resampling rounds | loss rel err | d im worst / rms | d s worst / rms |")
    print("|---|---|---|---|---|---|---|---|")
    for kind, B, a, m, rounds, le, gi, gs in rows:
        print(f"| {kind} | {B} | {a} | {m} | {rounds} | {le:.1e} | {gi:.2e} | {gs:.2e} |")
    for kind in R.KINDS:
        worst = max(max(r[6], r[7]) for r in rows if r[0] == kind)
        print(f"{kind}: worst {worst:.3e} -> T = 4 x worst = {4 * worst:.3e} (RANK_T = {R.RANK_T[kind]:.1e})")


def per_call(calls, repeats):
    import torch

    from tests import ranking_loss_ref as R
    from text2loc_amd.losses import HardestRankingLoss, PairwiseRankingLoss

    shapes = (32, 64, 128, 512)
    data = {}
    for B in shapes:
        im, s, _ = R.conditioned_inputs(B, 0.9, 0.35)
        data[B] = (torch.tensor(np.asarray(im)).cuda().requires_grad_(), torch.tensor(np.asarray(s)).cuda().requires_grad_())

    def one(crit, x, y):
        x.grad = y.grad = None
        crit(x, y).backward()

    def timed(crit, x, y):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            one(crit, x, y)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls * 1e3

    out = {}
    for kind, cls in (("pairwise", PairwiseRankingLoss), ("hardest", HardestRankingLoss)):
        crits = {}
        for path in ("engine", "torch"):
            crits[path] = cls(0.35)
            crits[path].use_engine = path == "engine"
        for B in shapes:  # the warm-up of every shape on both paths
            for path in crits:
                for _ in range(50):
                    one(crits[path], *data[B])
        for B in shapes:
            runs = {"engine": [], "torch": []}
            for _ in range(repeats):
                for path in ("engine", "torch"):
                    runs[path].append(timed(crits[path], *data[B]))
            out[f"{kind}_B{B}"] = {p + "_us_per_call": [round(v, 1) for v in runs[p]] for p in runs}
    return out


def full_step(n_steps, repeats, B=64, n_hints=6, n_tok=16):
    """bench.full_train_step_measure's loop (engine text head, split-bf16) with the criterion a module: the embeddings become leaves,
    the module's backward fills their .grad, and those go where the contrastive call's gradients went."""
    import torch
    import torch.nn.functional as F

    from text2loc_amd import synth
    from text2loc_amd.cell_retrieval import LanguageEncoder
    from text2loc_amd.engine import Engine
    from text2loc_amd.losses import PairwiseRankingLoss

    eng = Engine(0)
    sd = synth.make_object_branch_weights(0)
    tens = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or ".color_encoder." in k or ".mlp_pointnet." in k or ".pointnet." in k:
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tens, class_embed=True, color_embed=True)
    cells = synth.make_cells(B, seed=9)
    p64 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    enc = LanguageEncoder(256, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1,
                          llm_model=object(), tokenizer=None, input_dim=1024)
    enc.load_state_dict({k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(0).items()}, strict=False)
    enc = enc.cuda().train()
    enc.use_engine_train_head = True
    eng.set_option("train_bf16", 2)
    hidden = 0.2 * torch.randn(B * n_hints, n_tok, 1024, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    crits = {}
    for path in ("engine", "torch"):
        crits[path] = PairwiseRankingLoss(0.35)
        crits[path].use_engine = path == "engine"

    def step(i, crit):
        eng.zero_grad()
        enc.engine_zero_grad()
        anchor = F.normalize(enc.head(hidden, B))
        pos = eng.encode_cells_train(p64, dropout_p=0.1, seed=i)
        a, p = anchor.detach().requires_grad_(), pos.detach().requires_grad_()
        loss = crit(a, p)
        loss.backward()
        eng.encode_cells_backward(p.grad)
        anchor.backward(a.grad)
        eng.adam_step(1e-3)
        enc.engine_adam_step(1e-4)
        return loss

    for i in range(6):
        for crit in crits.values():
            step(i, crit)
    enc._th_train_engine.set_option("text_train_bf16", 2)
    for i in range(3):
        for crit in crits.values():
            step(i, crit)
    runs = {"engine": [], "torch": []}
    for _ in range(repeats):
        for path, crit in crits.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_steps):
                last = step(100 + i, crit)
            torch.cuda.synchronize()
            runs[path].append(round((time.perf_counter() - t0) / n_steps * 1e3, 3))
    eng.close()
    return {"pairwise_" + p + "_ms_per_step_wall": v for p, v in runs.items()} | {"final_loss": float(last)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bars", action="store_true")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.bars:
        return bars()
    if args.calls < 200:
        ap.error("--calls: at least 200 per measurement")
    res = {"per_call": per_call(args.calls, args.repeats), "full_step_b64": full_step(args.steps, args.repeats)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
