"""Guard-band and call-history tiers for t2l_text_inter at the compiled shapes other than the published one (README, DESIGN 1a: new
ground gets both). tests/guards.py as it is, through the helpers of tests/test_gpu_memory_safety.py (run_guarded, dev, engine) and
tests/test_gpu_call_history.py (check_history). Halos and NaN / 4e4 inputs are ordinary data to the kernel: nothing here is meant to
fault."""
import numpy as np
import pytest

from tests.test_gpu_call_history import assert_same, check_history, snapshot
from tests.test_gpu_memory_safety import dev, engine, run_guarded
from tests.test_gpu_text_inter_shapes import SHAPE_IDS, SHAPES, head_sd, inter_oracle

pytestmark = pytest.mark.gpu


def shaped_engine(D, heads):
    e = engine()
    e.text_head_load_weights(head_sd(D), inter_num_heads=heads)
    return e


# ---- guard bands ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SHAPES, ids=SHAPE_IDS)
def shaped(request):
    D, heads = request.param
    e = shaped_engine(D, heads)
    e._D, e._heads = D, heads
    yield e
    e.close()


@pytest.mark.parametrize("n_desc,S", [(1, 1), (7, 5), (2, 17)])
def test_text_inter_between_guard_bands(shaped, n_desc, S):
    """The input between poisoned halos (NaN, then 3e38), the [n_desc, D] output and the flag carved from patterned buffers: halos intact,
    every output word written, flag 0, the bits of the plain run — and that run within the restatement's bound."""
    D, heads = shaped._D, shaped._heads
    sent = np.random.default_rng(n_desc * 100 + S).standard_normal((n_desc * S, D)).astype(np.float32)
    plain, runs = run_guarded(lambda a: shaped.text_inter(a["sent"], n_desc, check=False), {"sent": dev(sent)}, 2)
    ref = inter_oracle(sent, head_sd(D), n_desc, D, heads)
    assert all(tuple(r[0].shape) == (n_desc, D) and int(r[1].item()) == 0 for r in [plain] + runs)
    assert np.abs(plain[0].cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


# ---- call history --------------------------------------------------------------------------------------------------------------
def _small(D, n_desc, n_sent):
    d = dev(np.random.default_rng(n_desc * 100 + n_sent).standard_normal((n_desc * n_sent, D)).astype(np.float32))

    def call(e):
        out, bad = e.text_inter(d, n_desc)
        return {"out": out, "overflow": bad}
    return call


@pytest.mark.parametrize("D,heads", SHAPES, ids=SHAPE_IDS)
def test_text_inter_after_an_overflowing_batch(D, heads):
    sent = np.random.default_rng(7).standard_normal((40 * 13, D)).astype(np.float32)
    sent[17, 3] = np.nan
    sent[400, D - 56] = 4.0e4
    d_big = dev(sent)

    def dirty(e):
        _, bad = e.text_inter(d_big, 40)
        assert bad

    check_history(lambda: shaped_engine(D, heads), dirty, [_small(D, 2, 17), _small(D, 1, 1)])


def test_text_inter_after_a_reload_at_another_width():
    """A 256-wide head, a call, a 128-wide head loaded into the SAME context, a call: the bits and flag of a fresh context that only
    ever held the 128-wide head."""
    small = _small(128, 2, 17)
    fresh = shaped_engine(128, 4)
    try:
        ref = snapshot(small(fresh))
    finally:
        fresh.close()
    e = shaped_engine(256, 4)
    try:
        out, bad = e.text_inter(dev(np.random.default_rng(1).standard_normal((40 * 13, 256)).astype(np.float32)), 40)
        assert not bad and tuple(out.shape) == (40, 256)
        e.text_head_load_weights(head_sd(128), inter_num_heads=4)
        assert_same(snapshot(small(e)), ref, "the 128-wide call behind a 256-wide head")
    finally:
        e.close()
