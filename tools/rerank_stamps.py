"""dev: what the time of the merged-record re-rank is made of. Needs the stamps build (make -C text2loc_amd/csrc stamps): every query
wave leaves the 100 MHz clock at seven points (search.hip: T2L_RR_STAMP) and the SIMD it ran on. Headline shape (Q = 4096, N = 11,259,
k = 10), both settings of search_rerank_form, the last of back-to-back calls after a clock ramp.
    python tools/rerank_stamps.py [search_rerank_form values, default: 0 1 0 1]
Prints per form: the phases of a wave (mean and 10 / 90 % over the 4,096 waves); the same by age rank on the SIMD (the four resident
waves of a SIMD, oldest first: do they go through merge -> wait -> score together, or staggered?); and, over the kernel's span in
0.5 us bins, how many waves have row loads in flight (between "merge done" and "last row arrived") — the time the gather engine of the
whole device is given work."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text2loc_amd import engine as E, synth

E._LIB_PATH = os.path.join(os.path.dirname(E._LIB_PATH), "libt2l_stamps.so")
N, Q, K = 11259, 4096, 10
forms = [int(a) for a in sys.argv[1:]] or [0, 1, 0, 1]
eng = E.Engine(0)
db, qs, _ = synth.make_retrieval_problem(N, Q, seed=1, noise=0.5)
eng.db_set(torch.from_numpy(db).cuda())
dq = torch.from_numpy(qs).cuda()
eng.lib.t2l_debug_rerank_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
buf = np.zeros((Q, 8), dtype=np.int64)
PH = ("start -> records", "records -> merge done", "merge done -> first row", "first row -> last row", "last row -> early stored", "early stored -> end")


def us(x):
    return x / 100.0


for form in forms:
    eng.set_option("search_rerank_form", form)
    for _ in range(1500):
        eng.search(dq, K)
    assert eng.lib.t2l_debug_rerank_stamps(eng._h, buf.ctypes.data, Q) == 0
    st = buf.copy()
    early = st[:, 5] != 0
    t0 = st[:, 0].min()
    print("== search_rerank_form = %d: %d of %d waves on the early path; kernel span (first wave start -> last wave end) %.2f us" % (
        form, int(early.sum()), Q, us(st[:, 6].max() - t0)))
    e = st[early]
    d = np.diff(e[:, :7], axis=1)
    for i, nm in enumerate(PH):
        print("   %-26s mean %5.2f us  (10%% %5.2f, 90%% %5.2f)" % (nm, us(d[:, i].mean()), us(np.percentile(d[:, i], 10)), us(np.percentile(d[:, i], 90))))
    hw = st[:, 7]
    h, xcc = hw & 0xFFFFFFFF, hw >> 32
    key = (xcc & 15) << 16 | ((h >> 13) & 7) << 12 | ((h >> 12) & 1) << 11 | ((h >> 8) & 15) << 4 | ((h >> 4) & 3)
    ranks = {}
    sizes = []
    for k in np.unique(key):
        w = np.nonzero(key == k)[0]
        w = w[np.argsort(st[w, 0], kind="stable")]
        sizes.append(len(w))
        for r, i in enumerate(w):
            ranks.setdefault(r, []).append(i)
    print("   SIMDs seen: %d, waves per SIMD: min %d, max %d" % (len(sizes), min(sizes), max(sizes)))
    print("   by age on the SIMD (us from the kernel's first wave start; mean over SIMDs):   start  records  merged  row0   row11  stored   end")
    for r in sorted(ranks)[:6]:
        w = np.array([i for i in ranks[r] if early[i]])
        if len(w) == 0:
            continue
        m = [us((st[w, c] - t0).mean()) for c in range(7)]
        print("      wave %d of the SIMD (%4d waves): " % (r, len(w)) + " ".join("%7.2f" % x for x in m))
    # stagger inside a SIMD: spread of "merge done" among the SIMD's waves against the length of the merge
    spread = []
    for k in np.unique(key):
        w = np.nonzero((key == k) & early)[0]
        if len(w) >= 2:
            spread.append(st[w, 2].max() - st[w, 2].min())
    print("   spread of 'merge done' among the waves of one SIMD: mean %.2f us (merge itself: %.2f us)" % (us(np.mean(spread)), us(d[:, 1].mean())))
    span = int(st[:, 6].max() - t0)
    bins = np.arange(0, span + 50, 50)
    inflight = [(int(((st[:, 2] - t0 < b + 50) & (st[:, 4] - t0 > b) & early).sum())) for b in bins[:-1]]
    print("   waves with row loads in flight per 0.5 us bin: " + " ".join("%d" % x for x in inflight))
