"""t2l_text_inter at every compiled (width, heads) against the same layer on the PyTorch modules — what LanguageEncoder ran at the
shapes other than (256, 4) before they were compiled — at 4,096 descriptions x 6 sentences, in ONE process: device events, a warm-up
per shape and variant, windows of >= 0.5 s, the two variants alternating over --repeats rounds. (256, 4) is the control.

    python tools/inter_shapes_time.py [--n_desc 4096] [--sentences 6] [--repeats 5] [--json out.json]

Per shape: median, min and max of the per-call time of both variants over the rounds, the engine's achieved TFLOP/s (FLOPs from the
shapes: per sentence row 24 D^2 for the six D x D-equivalents of in_proj / out_proj / linear1 / linear2 + 4 S D for the scores and
P V), the largest |engine - PyTorch| on this input, and whether the engine's slowest round beats PyTorch's fastest."""
import argparse
import json
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from text2loc_amd import synth  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402

SHAPES = [(256, 4), (128, 4), (128, 2), (256, 8)]


def window_ms(fn, min_s=0.5):
    """Per-call time of fn over a window of at least min_s seconds of device time (device events around batches of calls)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total, batch = 0, 0.0, 50
    while total < min_s * 1e3:
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        calls += batch
    return total / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_desc", type=int, default=4096)
    ap.add_argument("--sentences", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    n, S = a.n_desc, a.sentences
    rows = []
    for D, heads in SHAPES:
        sd = synth.make_language_head_weights(1, embed_dim=D)
        eng = Engine(0)
        eng.text_head_load_weights(sd, inter_num_heads=heads)
        layer = torch.nn.TransformerEncoderLayer(D, heads, dim_feedforward=4 * D)
        p = "language_encoder.inter_module.0."
        layer.load_state_dict({k[len(p):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith(p)})
        layer = layer.cuda().eval()
        x = torch.from_numpy(np.random.default_rng(D + heads).standard_normal((n * S, D)).astype(np.float32)).cuda()

        def engine_call():
            return eng.text_inter(x, n, check=False)[0]

        def torch_call():  # LanguageEncoder._head_second_half on the modules
            with torch.no_grad():
                y = x.view(n, S, -1).permute(1, 0, 2)
                y = y + layer(y)
                return y.max(dim=0)[0]

        err = float((engine_call() - torch_call()).abs().max())
        for fn in (engine_call, torch_call):  # warm-up of both variants at this shape
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        te, tt = [], []
        for _ in range(a.repeats):  # alternating
            te.append(window_ms(engine_call))
            tt.append(window_ms(torch_call))
        flop = n * S * (24.0 * D * D + 4.0 * S * D)
        row = {"D": D, "heads": heads, "n_desc": n, "sentences": S,
               "engine_ms": {"median": float(np.median(te)), "min": min(te), "max": max(te)},
               "pytorch_ms": {"median": float(np.median(tt)), "min": min(tt), "max": max(tt)},
               "engine_tflops": flop / (float(np.median(te)) * 1e-3) / 1e12, "max_abs_diff": err,
               "engine_wins_outside_the_spread": max(te) < min(tt)}
        rows.append(row)
        print(f"({D}, {heads}): engine {row['engine_ms']['median']:.4f} ms [{min(te):.4f}, {max(te):.4f}]  pytorch "
              f"{row['pytorch_ms']['median']:.4f} ms [{min(tt):.4f}, {max(tt):.4f}]  {row['engine_tflops']:.1f} TFLOP/s  "
              f"|diff| {err:.1e}  engine wins: {row['engine_wins_outside_the_spread']}", flush=True)
        eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
