"""ms per full training step of the fine stage downstream of the text branch (forward, offset_lambda * MSE, backward,
torch.optim.Adam) on the engine (t2l_fine_train_*) and, beside it, the same step on PyTorch-ROCm: the package's CrossMatch
parameter containers (nn.Linear / nn.BatchNorm1d / nn.TransformerDecoderLayer, float32, dropout 0.1) run as
models/cross_matcher.py:86-135 runs them. Same weights, inputs and batch. Device events around `--iters` steps after
`--warmup` steps; the median of `--reps` repetitions and their spread (max - min). Prints one JSON line.

`--points`: the published configuration instead — features2 from the PointNet++ backbone on each pair's point batch
(t2l_fine_train_forward_points), trained jointly (the backward continues into it, Adam steps it too). Engine only: the
reference's backbone needs torch_geometric, which this machine does not have, so there is no PyTorch column. The row also
gives the device memory the first step claimed (the backbone's saved activations and scratch plus the fine step's arena).

`--text`: the WHOLE step, text branch included — ``CrossMatch.forward`` under ``train()`` with a real ``LanguageEncoder(is_fine=True)``
behind a stub T5 that hands back fixed hidden states [B * 6, --tokens, 1024] (T5 itself is frozen and out of scope), offset_lambda * MSE,
``backward`` and ``torch.optim.Adam(model.parameters())``. Two rows per batch size: ``use_engine_train_head`` on (t2l_text_head_train /
_backward) and off (the head on its PyTorch modules: exactly the step before the engine served the fine head); everything else —
the packing of the objects, the engine's decoder step, the optimizer — is the same code in both. Every row gives the five
repetitions' medians' median and their spread (max - min). ``--text-only on|off`` runs one of the two (a kernel trace of its own).

`--optimizer engine|torch|both`: the step through ``CrossMatch.forward`` under ``train()`` (embedding mode, `--points`: point batches
with the backbone trained jointly, `--text`: with the real hint encoder; the two combine) with ``text2loc_amd.optim.Adam(model)`` — t2l_fine_zero_grad /
t2l_fine_adam_step, the hint encoder's head on t2l_text_adam_step — or ``torch.optim.Adam(model.parameters())``, which is the step as it
was before the engine had the fine stage's optimizer. ``both`` puts the two rows of a size side by side in one run, with the gain and
whether it exceeds the larger of the two spreads.

    python tools/bench_fine_train.py [--batches 32,256] [--iters 20] [--warmup 10] [--reps 5] [--points | --text [--tokens 12]]
                                     [--optimizer engine|torch|both]
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
from text2loc_amd.cross_matcher import CrossMatch  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402

NUM_MEAN, NUM_STD = 1826.6844940968194, 2516.8905096993817
LAMBDA = 5.0


def make_args(embed):
    return argparse.Namespace(fine_embed_dim=128, fine_num_decoder_heads=4, fine_num_decoder_layers=2, pad_size=16, num_mentioned=6,
                              fine_intra_module_num_layers=1, fine_intra_module_num_heads=4, hungging_model=None, fixed_embedding=True,
                              class_embed=embed, color_embed=embed, pointnet_freeze=True, use_features=["class", "color", "position", "num"])


def problem(embed, B, H=6):
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, make_args(embed), language_encoder=torch.nn.Identity())
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_fine_weights(0).items()}, strict=False)
    model = model.cuda().train()
    cells = synth.make_cells(B, seed=1, min_obj=16, max_obj=16)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    rng = np.random.default_rng(2)
    hints = torch.from_numpy(rng.standard_normal((B, H, 128)).astype(np.float32)).cuda()
    pn = None if embed else torch.from_numpy(np.abs(rng.standard_normal((B * 16, 256))).astype(np.float32)).cuda()
    target = torch.from_numpy(rng.random((B, 2)).astype(np.float32)).cuda()
    return model, packed, hints, pn, target


def torch_forward(model, packed, hints, pn):
    a, oe = model.args, model.object_encoder
    emb = [F.normalize(oe.class_embedding(packed["class_idx"].long()) if a.class_embed else oe.mlp_pointnet(pn), dim=-1),
           F.normalize(oe.color_embedding(packed["color_idx"].long()) if a.color_embed else oe.color_encoder(packed["rgb"]), dim=-1),
           F.normalize(oe.pos_encoder(packed["center"]), dim=-1),
           F.normalize(oe.num_encoder(((packed["n_pts"] - NUM_MEAN) / NUM_STD)[:, None]), dim=-1)]
    obj = F.normalize(oe.mlp_merge(torch.cat(emb, -1)), dim=-1).reshape(hints.shape[0], 16, 128).transpose(0, 1)
    hint = hints.transpose(0, 1)
    for i in range(a.fine_num_decoder_layers):
        obj = model.cross_objects[i](obj, hint)
        hint = model.cross_hints[i](hint, obj)
    return model.mlp_offsets(hint.max(dim=0).values)


def time_steps(step, iters, warmup, reps, all_reps=False):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return [float(x) for x in ms] if all_reps else float(np.median(ms))


def bench(embed, B, iters, warmup, reps):
    model, packed, hints, pn, target = problem(embed, B)
    params = [p for p in model.parameters() if p.requires_grad]
    # ---- engine: t2l_fine_train_forward / _backward on the live tensors, torch's MSE and Adam around them
    eng = Engine(torch.cuda.current_device())
    run, with_grad = model._fine_train_modules()
    tensors = model._fine_train_tensors()
    eng.fine_train_bind(tensors, class_embed=embed, color_embed=embed, use_features=tuple(model.args.use_features), num_layers=2)
    opt_e = torch.optim.Adam([p for n, p in model.named_parameters() if p.grad is not None], lr=1e-4)
    gh = torch.empty_like(hints)
    gp = None if pn is None else torch.empty_like(pn)
    seed = [0]

    def engine_step():
        opt_e.zero_grad(set_to_none=False)
        seed[0] += 1
        out = eng.fine_train_forward(packed, pn, hints, dropout_p=0.1, seed=seed[0]).requires_grad_(True)
        loss = LAMBDA * F.mse_loss(out, target)
        loss.backward()
        eng.fine_train_backward(out.grad, gh, gp)
        opt_e.step()

    reps_engine = time_steps(engine_step, iters, warmup, reps, all_reps=True)
    ms_engine = float(np.median(reps_engine))
    eng.close()
    # ---- PyTorch-ROCm: the same step through torch's own modules (fresh copy of the weights)
    model2, _, _, _, _ = problem(embed, B)
    h_leaf = hints.clone().requires_grad_(True)
    pn_leaf = None if pn is None else pn.clone().requires_grad_(True)
    opt_t = torch.optim.Adam([p for p in model2.parameters() if p.requires_grad], lr=1e-4)

    def torch_step():
        opt_t.zero_grad(set_to_none=False)
        loss = LAMBDA * F.mse_loss(torch_forward(model2, packed, h_leaf, pn_leaf), target)
        loss.backward()
        opt_t.step()

    ms_torch = time_steps(torch_step, iters, warmup, reps)
    del params
    return {"mode": "embed" if embed else "features2", "B": B, "ms_engine": round(ms_engine, 4),
            "spread_ms": round(max(reps_engine) - min(reps_engine), 4), "ms_pytorch": round(ms_torch, 4), "speedup": round(ms_torch / ms_engine, 3)}


def bench_points(B, iters, warmup, reps):
    args = make_args(False)
    args.pointnet_freeze = False  # the published fine command: the backbone trains with everything else
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=torch.nn.Identity())
    sd = dict(synth.make_fine_weights(0))
    sd.update(synth.make_pointnet_weights(0))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda().train()
    cells = synth.make_cells(B, seed=1, min_obj=16, max_obj=16)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    pos, rgb = (torch.from_numpy(a).cuda() for a in synth.make_sampled_points(cells, 3))
    rng = np.random.default_rng(2)
    hints = torch.from_numpy(rng.standard_normal((B, 6, 128)).astype(np.float32)).cuda()
    target = torch.from_numpy(rng.random((B, 2)).astype(np.float32)).cuda()
    eng = Engine(torch.cuda.current_device())
    tensors = model._fine_train_tensors()
    eng.fine_train_bind(tensors, class_embed=False, color_embed=False, use_features=tuple(model.args.use_features), num_layers=2)
    for t, g in model._fine_train_pn_live:  # the backbone's buffers as .grad: every step's backward goes through it
        t.grad = g
    opt = torch.optim.Adam([p for n, p in model.named_parameters() if p.grad is not None], lr=1e-4)
    gh = torch.empty_like(hints)
    seed = [0]

    def engine_step():
        opt.zero_grad(set_to_none=False)
        seed[0] += 1
        out = eng.fine_train_forward_points(packed, pos, rgb, hints, dropout_p=0.1, seed=seed[0]).requires_grad_(True)
        loss = LAMBDA * F.mse_loss(out, target)
        loss.backward()
        eng.fine_train_backward(out.grad, gh, None)
        opt.step()

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    engine_step()
    torch.cuda.synchronize()
    claimed = free0 - torch.cuda.mem_get_info()[0]
    ms = time_steps(engine_step, iters, warmup, reps, all_reps=True)
    eng.close()
    return {"mode": "points (backbone trained)", "B": B, "objects": 16 * B, "ms_engine": round(float(np.median(ms)), 4),
            "spread_ms": round(max(ms) - min(ms), 4), "ms_pytorch": None,
            "first_step_device_gb": round(claimed / 1e9, 3)}


class _Obj:  # duck-types the reference's Object3d (xyz, rgb, label)
    def __init__(self, label, xyz, rgb):
        self.label, self.xyz, self.rgb = label, xyz, rgb


class _StubT5:
    def __init__(self, hidden):
        self.hidden = hidden

    def __call__(self, input_ids=None, attention_mask=None, output_attentions=False):
        return argparse.Namespace(last_hidden_state=self.hidden)


def _stub_tokenizer(sentences, return_tensors="pt", padding="longest"):
    ids = torch.zeros((len(sentences), 4), dtype=torch.long)
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def _objects(B):
    from text2loc_amd.cross_matcher import pad_objects

    cells = synth.make_cells(B, seed=1, min_obj=16, max_obj=16)
    objects = [[] for _ in range(B)]
    for b, o, label, xyz, rgb in synth.make_object_points(cells, 1):
        objects[b].append(_Obj(label, xyz, rgb))
    return cells, [pad_objects(o) for o in objects]


def bench_optimizer(mode, B, kind, L, iters, warmup, reps, H=6):
    """One row: the model-level step in ``mode`` (embed / points / text / points+text) stepped by ``kind`` (engine: optim.Adam(model);
    torch)."""
    from text2loc_amd import optim

    target = torch.from_numpy(np.random.default_rng(2).random((B, 2)).astype(np.float32)).cuda()
    points = None
    if mode in ("text", "points+text"):
        model, objects, hints, cells = _text_problem(B, L, True, H, points=mode == "points+text")
    else:
        args = make_args(mode == "embed")
        args.pointnet_freeze = mode != "points"
        model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=torch.nn.Identity())
        sd = dict(synth.make_fine_weights(0))
        if mode == "points":
            sd.update(synth.make_pointnet_weights(0))
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
        model = model.cuda().train()
        cells, objects = _objects(B)
        hints = torch.from_numpy(np.random.default_rng(2).standard_normal((B, H, 128)).astype(np.float32)).cuda()
    if mode in ("points", "points+text"):
        pos, rgb = (torch.from_numpy(a).cuda() for a in synth.make_sampled_points(cells, 3))
        points = [{"pos": pos[16 * b:16 * b + 16].reshape(-1, 3), "x": rgb[16 * b:16 * b + 16].reshape(-1, 3)} for b in range(B)]
    opt = optim.Adam(model, lr=1e-4) if kind == "engine" else torch.optim.Adam(model.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=False)
        loss = LAMBDA * F.mse_loss(model(objects, hints, points), target)
        loss.backward()
        opt.step()

    ms = time_steps(step, iters, warmup, reps, all_reps=True)
    return {"mode": mode, "B": B, "optimizer": kind, "ms_step": round(float(np.median(ms)), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "reps_ms": [round(x, 4) for x in ms]}


def _text_problem(B, L, engine_head, H=6, points=False):
    from text2loc_amd.cell_retrieval import LanguageEncoder

    hidden = torch.from_numpy(synth.make_t5_hidden(B * H, L, seed=3)).cuda()
    enc = LanguageEncoder(128, fixed_embedding=True, intra_module_num_layers=1, is_fine=True, llm_model=_StubT5(hidden),
                          tokenizer=_stub_tokenizer, input_dim=1024)
    head = {k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(1, embed_dim=128).items()
            if ".inter_module." not in k}
    enc.load_state_dict(head, strict=False)
    enc.use_engine_train_head = bool(engine_head)
    args = make_args(not points)
    args.pointnet_freeze = not points  # point batches: the published command, the backbone trains with everything else
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=enc)
    sd = dict(synth.make_fine_weights(0))
    if points:
        sd.update(synth.make_pointnet_weights(0))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    model = model.cuda().train()
    cells, objects = _objects(B)
    texts = [" ".join(["The pose is north of a gray pole."] * H)] * B
    return model, objects, texts, cells


def bench_text(B, L, engine_head, iters, warmup, reps, H=6):
    from text2loc_amd.cell_retrieval import LanguageEncoder

    model, objects, texts, _ = _text_problem(B, L, engine_head, H)
    target = torch.from_numpy(np.random.default_rng(2).random((B, 2)).astype(np.float32)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    n0 = LanguageEncoder.train_engine_calls

    def step():
        opt.zero_grad(set_to_none=False)
        loss = LAMBDA * F.mse_loss(model(objects, texts, None), target)
        loss.backward()
        opt.step()

    ms = time_steps(step, iters, warmup, reps, all_reps=True)
    served = LanguageEncoder.train_engine_calls - n0
    assert served == ((warmup + iters * reps) if engine_head else 0), served  # the row measures the path it names
    return {"B": B, "sentences": B * H, "tokens": L, "text_head": "engine" if engine_head else "pytorch", "ms_step": round(float(np.median(ms)), 4),
            "spread_ms": round(max(ms) - min(ms), 4), "reps_ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", action="store_true", help="features2 from the jointly trained PointNet++ backbone (engine only)")
    ap.add_argument("--text", action="store_true", help="the whole step with a real LanguageEncoder(is_fine) behind fixed hidden states")
    ap.add_argument("--tokens", type=int, default=12, help="--text: tokens per hint sentence")
    ap.add_argument("--text-only", choices=["on", "off"], default=None, help="--text: only the row with the engine head on / off")
    ap.add_argument("--optimizer", choices=["engine", "torch", "both"], default=None,
                    help="the model-level step with optim.Adam(model) (engine), torch.optim.Adam(model.parameters()) (torch), or both rows")
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.optimizer is not None:
        mode = "points+text" if (a.text and a.points) else "text" if a.text else "points" if a.points else "embed"
        kinds = ["engine", "torch"] if a.optimizer == "both" else [a.optimizer]
        rows = [bench_optimizer(mode, int(B), k, a.tokens, a.iters, a.warmup, a.reps) for B in a.batches.split(",") for k in kinds]
        by = {(r["B"], r["optimizer"]): r for r in rows}
        for B in {r["B"] for r in rows}:
            if (B, "engine") in by and (B, "torch") in by:
                e, t = by[(B, "engine")], by[(B, "torch")]
                e["gain_ms"] = round(t["ms_step"] - e["ms_step"], 4)
                e["beats_torch_adam_by_more_than_the_spread"] = bool(e["gain_ms"] > max(e["spread_ms"], t["spread_ms"]))
        print(json.dumps({"metric": "fine-stage training step through CrossMatch.forward under train() (fwd + offset_lambda*MSE + bwd + "
                                    "zero_grad + Adam), 2 decoder layers, 6 hints, dropout 0.1, by optimizer", "unit": "ms/step", "rows": rows}))
        return
    if a.text:
        heads = [True, False] if a.text_only is None else [a.text_only == "on"]
        rows = [bench_text(int(B), a.tokens, h, a.iters, a.warmup, a.reps) for B in a.batches.split(",") for h in heads]
        by = {(r["B"], r["text_head"]): r for r in rows}
        for B in {r["B"] for r in rows}:
            if (B, "engine") in by and (B, "pytorch") in by:
                e, t = by[(B, "engine")], by[(B, "pytorch")]
                e["gain_ms"] = round(t["ms_step"] - e["ms_step"], 4)
                e["beats_pytorch_head_by_more_than_the_spread"] = bool(e["gain_ms"] > max(e["spread_ms"], t["spread_ms"]))
        print(json.dumps({"metric": "full fine-stage training step with the text head (CrossMatch.forward under train(): text head fwd + "
                                    "decoder fwd + offset_lambda*MSE + bwd + text head bwd + Adam), 2 decoder layers, 6 hints of --tokens tokens, dropout 0.1, embedding mode",
                          "unit": "ms/step", "rows": rows}))
        return
    if a.points:
        rows = [bench_points(int(B), a.iters, a.warmup, a.reps) for B in a.batches.split(",")]
        print(json.dumps({"metric": "fine-stage training step with the PointNet++ backbone trained jointly (backbone fwd + fwd + "
                                    "offset_lambda*MSE + bwd + backbone bwd + Adam), L=2, 6 hints, dropout 0.1, 256 points per object",
                          "unit": "ms/step", "rows": rows,
                          "pytorch": "no PyTorch column: the reference's PointNet++ needs torch_geometric, which is not installed"}))
        return
    rows = [bench(embed, int(B), a.iters, a.warmup, a.reps) for embed in (True, False) for B in a.batches.split(",")]
    print(json.dumps({"metric": "fine-stage training step (fwd + offset_lambda*MSE + bwd + Adam), L=2, 6 hints, dropout 0.1",
                      "unit": "ms/step", "rows": rows}))


if __name__ == "__main__":
    main()
