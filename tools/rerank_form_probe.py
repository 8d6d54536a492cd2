"""dev: step time of the headline search (Q = 4096, N = 11,259, K = 10) under search_rerank_form = 0 (round 7's re-rank of merged
records) and = 1 (row-local merge, the twelve early rows in one round trip), alternated on ONE engine on one device: per round and arm
1,500 untimed ramp steps, then 400 timed stream-ordered steps of the bench loop over its four rotated query batches. Prints the raw
rounds, per-arm median / min / max, and the verdict rule: a gain only if the new arm's slowest round beats the old arm's fastest.
Then, alternated rounds per arm, the scan's and the re-rank's kernel times (HIP events on every 4th launch, span stamps), same rule.
    python tools/rerank_form_probe.py [rounds] [--parent /path/to/parent/libt2l.so] [--parts /path/to/libt2l_parts.so]
--parent: a further arm, a library built from the parent commit loaded beside the shipped one (its only form is arm 0's): shows that
the kept old path has not itself slowed down.
--parts: a library built with -DT2L_RERANK_PARTS instead of the shipped one; the arms are then form 0, 1, 2 (the row-local merge alone)
and 3 (the one round trip alone), every one judged against form 0 by the same rule."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text2loc_amd import engine as E, synth

N, Q, K, N_BATCH, N_OUT, RAMP, TIMED = 11259, 4096, 10, 4, 12, 1500, 400
argv = sys.argv[1:]
parent = None
if "--parent" in argv:
    i = argv.index("--parent")
    parent = argv[i + 1]
    del argv[i:i + 2]
parts = None
if "--parts" in argv:
    i = argv.index("--parts")
    parts = argv[i + 1]
    del argv[i:i + 2]
rounds = int(argv[0]) if argv else 6

db, qs, _ = synth.make_retrieval_problem(N, Q, 256, seed=1, noise=0.5)
batches = [qs] + [synth.make_queries_for(db, Q, seed=100 + bi, noise=0.5)[0] for bi in range(1, N_BATCH)]
d_db = torch.from_numpy(db).cuda()
d_qs = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in batches]
outs = [(torch.empty((Q, K), dtype=torch.int32, device="cuda"), torch.empty((Q, K), dtype=torch.float64, device="cuda")) for _ in range(N_OUT)]


def make_engine(path=None):
    if path:
        E._LIB_PATH, E._lib = path, None
    eng = E.Engine(0)
    eng.db_set(d_db)
    return eng


eng = make_engine(parts)
forms = (0, 1, 2, 3) if parts else (0, 1)
arms = [("form=%d" % f, eng, f) for f in forms]
if parent:
    arms.append(("parent", make_engine(parent), None))


def run(eng, steps):
    for i in range(steps):
        eng.search(d_qs[i % N_BATCH], K, out=outs[i % N_OUT])


ref = {}
times = {name: [] for name, _, _ in arms}
for rnd in range(rounds):
    for name, e, epi in arms:
        if epi is not None:
            e.set_option("search_rerank_form", epi)
        run(e, RAMP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(e, TIMED)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / TIMED * 1e6)
        if rnd == 0:  # the last timed step was batch (TIMED - 1) % N_BATCH into outs[(TIMED - 1) % N_OUT]
            ref[name] = tuple(t.clone() for t in outs[(TIMED - 1) % N_OUT])
    print("round %d: " % rnd + ", ".join("%s %.2f us/step" % (name, times[name][-1]) for name, _, _ in arms), flush=True)
for name, _, _ in arms:
    t = times[name]
    print("%s: median %.2f, min %.2f, max %.2f, spread %.2f us/step over %d rounds" % (name, statistics.median(t), min(t), max(t), max(t) - min(t), len(t)))
    print("  ids equal to form=0: %s, scores equal: %s" % (bool(torch.equal(ref[name][0], ref["form=0"][0])), bool(torch.equal(ref[name][1], ref["form=0"][1]))))
m0 = statistics.median(times["form=0"])
for f in forms[1:]:
    t = times["form=%d" % f]
    print("form=%d against form=0: difference of medians %.2f us/step; its slowest %.2f, form=0 fastest %.2f -> %s"
          % (f, m0 - statistics.median(t), max(t), min(times["form=0"]), "a gain" if max(t) < min(times["form=0"]) else "not a gain by the rule"))
# kernel times of the two arms (HIP events around every 4th launch: they cost the stream ~6 us, the same in both arms; the scan's span
# stamps cost nothing)
names = ("search_scan", "search_rerank", "search_scan_span", "search_scan_busy")
kt = {f: [] for f in forms}
for rnd in range(max(3, rounds // 2)):
    for epi in forms:
        eng.set_option("search_rerank_form", epi)
        run(eng, 300)
        eng.set_option("profile_events", 4)
        eng.set_option("profile_rerank", 1)
        for nme in names:
            eng.kernel_stats(nme)
        run(eng, 400)
        torch.cuda.synchronize()
        kt[epi].append({nme: round(eng.kernel_stats(nme)[0] * 1e3, 2) for nme in names})
        eng.set_option("profile_events", 0)
        print("kernel times (us), form=%d:" % epi, kt[epi][-1], flush=True)
for nme in ("search_rerank", "search_scan"):
    a0 = [k[nme] for k in kt[0]]
    for f in forms[1:]:
        a1 = [k[nme] for k in kt[f]]
        print("%s: form=0 median %.2f (%.2f-%.2f), form=%d median %.2f (%.2f-%.2f) us -> %s" % (
            nme, statistics.median(a0), min(a0), max(a0), f, statistics.median(a1), min(a1), max(a1),
            "form=%d faster by the rule" % f if max(a1) < min(a0) else "no difference by the rule"))
if parent:
    print("arm 0 against the parent build: %.2f us/step (medians)" % (m0 - statistics.median(times["parent"])))
