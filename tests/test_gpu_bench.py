"""GPU tier: a plain ``bench.py`` run (no --full) prints the headline alone, and --dump-outputs writes what its last timed step
returned: the ids and scores of the float64 ranking of the query batch that step searched."""
import json
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle
from text2loc_amd import synth

pytestmark = pytest.mark.gpu
REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def test_plain_run_dumps_its_last_timed_step(tmp_path):
    steps = 3  # the timed steps rotate bench.py's 4 query batches: the last one searches batch (steps - 1) % 4 = 2
    r = subprocess.run([sys.executable, osp.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    o = json.loads(r.stdout.splitlines()[-1])
    assert o["steps"] == steps and o["unit"] == "queries/s" and o["higher_is_better"] is True and o["dtype"] == "f16"
    assert o["ms_per_step"] > 0 and o["value"] == pytest.approx(4096 * 1e3 / o["ms_per_step"], rel=1e-4)
    assert not {"roofline", "parity", "cpu_baseline", "steady_state", "side_ms"} & set(o)  # what --full adds
    ids, sc = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "scores.npy")
    assert ids.dtype == sc.dtype == np.float64 and ids.shape == sc.shape == (4096, 10)
    db, _, _ = synth.make_retrieval_problem(11259, 4096, 256, seed=1, noise=0.5)
    qs, _ = synth.make_queries_for(db, 4096, seed=100 + (steps - 1) % 4, noise=0.5)
    ridx, rsc = c_oracle.retrieve_topk(db, qs[:512], 10)
    assert np.array_equal(ids[:512].astype(np.int64), ridx)
    assert np.abs(sc[:512] - rsc).max() < 1e-12
