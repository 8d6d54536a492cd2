"""dev: the phases of the training step that contain a TransformerEncoderLayer, timed with the library named by T2L_LIB (A/B: alternate
fresh processes, one library each). Prints one JSON line:
  train_forward / train_backward / adam_step ms per step of the object branch at B = 64, dropout 0.1, f32 and split-bf16 operands;
  text_head_forward_ms / text_head_backward_ms of the full step (bench.full_train_step_measure's step: 64 x 6 sentences x 16 tokens).
--pn-feat: the object branch WITHOUT embedding tables (class_embed = color_embed = False, PointNet++ features supplied as pn_feat: the
mlp_pointnet block and three small branches), and no text head.
Every figure is the mean over the event pairs of a window of at least MIN_WINDOW_S seconds behind a warm-up, as bench.py times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text2loc_amd import synth  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402

MIN_WINDOW_S = 0.6


def window(step, warm, events):
    """warm steps, then steps with event pairs for MIN_WINDOW_S; returns {event: mean ms} and the number of steps"""
    engines = {id(e): e for e, _ in events}.values()
    for i in range(warm):
        step(i)
    torch.cuda.synchronize()
    for e in engines:
        e.set_option("profile_events", 1)
    for e, name in events:
        e.kernel_stats(name)
    t0, n = time.perf_counter(), 0
    while n < 50 or time.perf_counter() - t0 < MIN_WINDOW_S:
        step(1000 + n)
        n += 1
        if n % 25 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = {name: e.kernel_stats(name)[0] for e, name in events}
    for e in engines:
        e.set_option("profile_events", 0)
    return out, n


def main(embed, B=64, n_hints=6, n_tok=16):
    import torch.nn.functional as F

    from text2loc_amd.cell_retrieval import LanguageEncoder

    eng = Engine(0)
    sd = synth.make_object_branch_weights(0)
    cells = synth.make_cells(B, seed=9, with_pn_feat=not embed)
    tens = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or ".pointnet." in k:
            continue
        if (".color_encoder." in k or ".mlp_pointnet." in k) if embed else k.endswith("_embedding.weight"):
            continue
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
    eng.train_bind(tens, class_embed=embed, color_embed=embed)
    gpn = None if embed else torch.zeros((int(cells["offsets"][-1]), 256), device="cuda")
    p64 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    anchor = F.normalize(torch.randn(B, 256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)))
    res = {"lib": os.environ.get("T2L_LIB", "shipped"), "config": "embed" if embed else "pn_feat"}

    def cell_step(i):
        eng.zero_grad()
        pos = eng.encode_cells_train(p64, dropout_p=0.1, seed=i)
        _, _, gp = eng.contrastive_loss(anchor, pos, 0.1)
        eng.encode_cells_backward(gp, gpn)
        eng.adam_step(1e-3)

    for name, bf16 in (("f32", 0), ("split_bf16", 2)):
        eng.set_option("train_bf16", bf16)
        ms, n = window(cell_step, 100, [(eng, "train_forward"), (eng, "train_backward"), (eng, "adam_step")])
        res["train_forward_ms_" + name], res["train_backward_ms_" + name], res["steps_" + name] = ms["train_forward"], ms["train_backward"], n
        res["adam_step_ms_" + name] = ms["adam_step"]
    eng.set_option("train_bf16", 2)
    if not embed:
        eng.close()
        print(json.dumps(res))
        return

    enc = LanguageEncoder(256, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1, llm_model=object(), tokenizer=None,
                          input_dim=1024)
    enc.load_state_dict({k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(0).items()}, strict=False)
    enc = enc.cuda().train()
    enc.use_engine_train_head = True
    hidden = 0.2 * torch.randn(B * n_hints, n_tok, 1024, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    def full_step(i):
        eng.zero_grad()
        enc.engine_zero_grad()
        a = F.normalize(enc.head(hidden, B))
        pos = eng.encode_cells_train(p64, dropout_p=0.1, seed=i)
        _, ga, gp = eng.contrastive_loss(a.detach().contiguous(), pos, 0.1)
        eng.encode_cells_backward(gp)
        a.backward(ga)
        eng.adam_step(1e-3)
        enc.engine_adam_step(1e-4)

    for i in range(3):  # (the head's own engine context exists after the first step)
        full_step(i)
    te = enc._th_train_engine
    ms, n = window(full_step, 30, [(te, "text_train_forward"), (te, "text_train_backward")])
    res["text_head_forward_ms"], res["text_head_backward_ms"], res["steps_full"] = ms["text_train_forward"], ms["text_train_backward"], n
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn-feat", action="store_true", help="the object branch without embedding tables, pn_feat supplied; no text head")
    main(embed=not ap.parse_args().pn_feat)
