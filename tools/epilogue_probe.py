"""dev: step time of the headline search (Q = 4096, N = 11,259, K = 10) under search_epilogue = 0 (round 6's scan epilogue and record
order) and = 1 (the short epilogue + XCD-contiguous records), alternated on ONE engine on one device: per round and arm 1,500 untimed
ramp steps, then 400 timed stream-ordered steps of the bench loop over its four rotated query batches. Prints the raw rounds, per-arm
median / min / spread (max - min), and the verdict rule: a gain only if the medians differ by more than the larger arm's spread.
Then, three alternated rounds per arm, the scan's and the re-rank's kernel times (HIP events on every 4th launch, span stamps).
    python tools/epilogue_probe.py [rounds] [--parent /path/to/parent/libt2l.so]
--parent: a third arm, a library built from the parent commit loaded beside the shipped one (its only epilogue is arm 0's): shows that
the kept old path has not itself slowed down."""
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


eng = make_engine()
arms = [("epilogue=0", eng, 0), ("epilogue=1", eng, 1)]
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
            e.set_option("search_epilogue", epi)
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
    print("  ids equal to epilogue=0: %s, scores equal: %s" % (bool(torch.equal(ref[name][0], ref["epilogue=0"][0])), bool(torch.equal(ref[name][1], ref["epilogue=0"][1]))))
m0, m1 = statistics.median(times["epilogue=0"]), statistics.median(times["epilogue=1"])
spread = max(max(times[a]) - min(times[a]) for a in ("epilogue=0", "epilogue=1"))
print("difference of medians (0 - 1): %.2f us/step; larger spread %.2f -> %s" % (m0 - m1, spread, "a gain" if m0 - m1 > spread else "not a gain by the rule"))
# kernel times of the two arms (HIP events around every 4th launch: they cost the stream ~6 us, the same in both arms; the scan's span
# stamps cost nothing): is the re-rank, which reads the new record order, any slower?
names = ("search_scan", "search_rerank", "search_scan_span", "search_scan_busy")
kt = {0: [], 1: []}
for rnd in range(3):
    for epi in (0, 1):
        eng.set_option("search_epilogue", epi)
        run(eng, 300)
        eng.set_option("profile_events", 4)
        eng.set_option("profile_rerank", 1)
        for nme in names:
            eng.kernel_stats(nme)
        run(eng, 400)
        torch.cuda.synchronize()
        kt[epi].append({nme: round(eng.kernel_stats(nme)[0] * 1e3, 2) for nme in names})
        eng.set_option("profile_events", 0)
        print("kernel times (us), epilogue=%d:" % epi, kt[epi][-1], flush=True)
if parent:
    print("arm 0 against the parent build: %.2f us/step (medians)" % (m0 - statistics.median(times["parent"])))
