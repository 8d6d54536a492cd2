"""dev: does another build of the library compute what this one computes in the training step? Per case — the object branch on
tests/golden/train_step_embed.npz and train_step_pn.npz, the text head on train_step_text.npz — through the Engine calls:
  step:  one forward + loss + backward from the fixture's weights, dropout 0.1, fixed seed: every output, gradient and running statistic.
         The inputs are the same in every run; the runs differ only where float and float64 atomics add in a different order.
  adam:  two Adam steps on gradients WRITTEN by this script (the same bits in every run): every parameter after them. adam_kernel is
         element-wise, so these must agree bit for bit. (Stepping on the step's own gradients would not be the same computation in two
         runs: where the true gradient is 0, lr * g / (|g| + eps) turns the sign of 1e-8-sized atomics noise into +-lr.)

    python tools/train_host_compare.py --parent path/to/parent/libt2l.so --new text2loc_amd/libt2l.so [--parent-runs N] --out table.md

runs the parent library N times (default 2) and the new one once, each in a fresh process (T2L_LIB names the library, as for
tools/train_layer_time.py). The rule, on parent runs 1 and 2: a tensor on which they agree bit for bit must agree bit for bit with
the new build; any other may differ from either of them by at most twice what they differ by. Exit status 1 when a tensor does not.
With N > 2 the table also has the parent's scatter over all N runs, and every further parent run is put through the same rule in the
new build's place: how often the parent breaks the rule against itself."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
P = "language_encoder."


def dump(path):
    import torch

    from tests.test_oracle_train import load_case
    from text2loc_amd import synth
    from text2loc_amd.engine import Engine

    res = {}

    def keep(tag, tensors, what):
        for k, (p, g) in tensors.items():
            t = g if what == "grad" else p
            if t is not None and (what != "running" or "running_" in k):
                res[f"{tag}/{k}"] = t.cpu().numpy().copy()

    def tens(sd, names):
        out = {}
        for k in names:
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).cuda()
            out[k] = (t, None if "running_" in k else torch.zeros_like(t))
        return out

    def adam(tag, tensors, step):
        for i in (1, 2):
            for j, (k, (p, g)) in enumerate(sorted(tensors.items())):
                if g is not None:
                    g.copy_(torch.from_numpy(np.random.default_rng([i, j]).standard_normal(tuple(g.shape), dtype=np.float32) * 0.01))
            step(1e-3)
            torch.cuda.synchronize()
        keep(f"{tag}/adam/after", {k: v for k, v in tensors.items() if v[1] is not None}, "param")

    for mode in ("embed", "pn"):
        g = np.load(os.path.join(GOLDEN, f"train_step_{mode}.npz"))
        cells, sd, embed = load_case(g, mode)
        names = [k for k in sd if not (k.endswith("num_batches_tracked") or k.startswith("object_encoder.pointnet.")
                                       or (embed and (".color_encoder." in k or ".mlp_pointnet." in k))
                                       or (not embed and k.endswith("_embedding.weight")))]
        eng = Engine(0)
        tensors = tens(sd, names)
        eng.train_bind(tensors, class_embed=embed, color_embed=embed)
        keys = ["offsets", "class_idx", "color_idx", "rgb", "center", "n_pts"] + ([] if embed else ["pn_feat"])
        dcells = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).cuda() for k in keys}
        eng.zero_grad()
        out = eng.encode_cells_train(dcells, dropout_p=0.1, seed=41)
        _, _, gp = eng.contrastive_loss(torch.from_numpy(g["anchor"]).cuda(), out, float(g["temperature"]))
        gpn = None if embed else torch.zeros((int(cells["offsets"][-1]), 256), device="cuda")
        eng.encode_cells_backward(gp, gpn)
        torch.cuda.synchronize()
        res[f"{mode}/step/out"] = out.cpu().numpy().copy()
        if gpn is not None:
            res[f"{mode}/step/grad_pn_feat"] = gpn.cpu().numpy().copy()
        keep(f"{mode}/step/grad", tensors, "grad")
        keep(f"{mode}/step/after", tensors, "running")
        adam(mode, tensors, eng.adam_step)
        eng.close()

    g = np.load(os.path.join(GOLDEN, "train_step_text.npz"))
    B, S, L = int(g["batch"]), int(g["n_hints"]), int(g["n_tokens"])
    sd = synth.make_language_head_weights(int(g["weight_seed"]))
    names = [k for k in sd if k.startswith((P + "intra_module.0.", P + "inter_mlp.0.", P + "inter_module.0.")) and not k.endswith("num_batches_tracked")]
    eng = Engine(0)
    tensors = tens(sd, names)
    eng.text_train_bind(tensors)
    hidden = torch.from_numpy(synth.make_t5_hidden(B * S, L, seed=int(g["hidden_seed"]))).cuda()
    G = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 256)).astype(np.float32) * 0.05).cuda()
    eng.text_zero_grad()
    out = eng.text_head_train(hidden, B, dropout_p=0.1, seed=51)
    eng.text_head_backward(G)
    torch.cuda.synchronize()
    res["text/step/out"] = out.cpu().numpy().copy()
    keep("text/step/grad", tensors, "grad")
    keep("text/step/after", tensors, "running")
    adam("text", tensors, eng.text_adam_step)
    eng.close()
    np.savez(path, **res)


def mx(a, b):
    return float(np.abs(a.astype(np.float64) - b).max()) if a.size else 0.0


def rule(a, b, c):
    """(ok, 'bit-equal' | 'within 2 x', parent 1 vs 2, c vs either) for candidate c against parent runs a, b"""
    d_pp, d_c = mx(a, b), max(mx(c, a), mx(c, b))
    if a.tobytes() == b.tobytes():
        return c.tobytes() == a.tobytes(), "bit-equal", d_pp, d_c
    return d_c <= 2 * d_pp, "within 2 x", d_pp, d_c


def compare(parents, new, out):
    ps, nw = [np.load(p) for p in parents], np.load(new)
    files = ps[0].files
    assert all(sorted(p.files) == sorted(files) for p in ps + [nw])
    more = len(ps) > 2
    lines = ["| tensor | parent run 1 vs 2, max abs | new vs parent run 1 or 2, max abs | |" + (f" parent, all {len(ps)} runs, max abs | further parent runs outside the rule |" if more else ""),
             "|---|---|---|---|" + ("---|---|" if more else "")]
    bad = exact = 0
    self_bad = [0] * (len(ps) - 2)
    for k in files:
        ok, what, d_pp, d_np = rule(ps[0][k], ps[1][k], nw[k])
        exact += ok and what == "bit-equal"
        bad += not ok
        extra = ""
        if more:
            own = [not rule(ps[0][k], ps[1][k], p[k])[0] for p in ps[2:]]
            self_bad = [x + y for x, y in zip(self_bad, own)]
            extra = f" {max(mx(a[k], b[k]) for i, a in enumerate(ps) for b in ps[i + 1:]):.3g} | {sum(own)} |"
        lines.append(f"| {k} | {d_pp:.3g} | {d_np:.3g} | {what if ok else 'NOT ' + what} |" + extra)
    lines.append("")
    lines.append(f"{len(files)} tensors: {exact} bit-equal in parent runs 1, 2 and the new run, {len(files) - exact - bad} within twice the scatter of parent runs 1 and 2, {bad} outside.")
    if more:
        lines.append(f"The same rule with parent run 3, 4, ... in the new build's place: {', '.join(str(x) for x in self_bad)} tensors outside.")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--parent-runs", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, lib in enumerate([a.parent] * max(2, a.parent_runs) + [a.new]):  # one fresh process per run; a run that fails ends the comparison
            paths.append(os.path.join(tmp, f"run{i}.npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", paths[-1]], env=dict(os.environ, T2L_LIB=os.path.abspath(lib)),
                           check=True, timeout=240)
        return compare(paths[:-1], paths[-1], a.out)


if __name__ == "__main__":
    sys.exit(main())
