"""GPU tier: the ranking losses' rows of the two tiers of DESIGN.md 1a. Guard bands (tests/guards.py, ``run_guarded`` of
tests/test_gpu_memory_safety.py): inputs between poisoned halos, outputs carved from patterned buffers — halos intact, outputs
written in full, the bits of the plain run. Call history (tests/test_gpu_call_history.py): ``loss_ws`` is shared with the
contrastive loss, so neither may see what the other, or a larger non-finite call, left there. No atomics in loss.hip: bit identity
throughout."""
import numpy as np
import pytest

from tests import ranking_loss_ref as R
from tests.test_gpu_call_history import check_history, loss_call
from tests.test_gpu_memory_safety import dev, engine, run_guarded

pytestmark = pytest.mark.gpu

M = 0.35


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "forward"])
@pytest.mark.parametrize("B", [1, 31, 33, 129, 200])
@pytest.mark.parametrize("kind", R.KINDS)
def test_guard_bands(eng, kind, B, need_grad):
    """One row past the 32-row tile, and one past the 128-row fused kernel: the ragged blocks of every stage."""
    im, s, _ = R.conditioned_inputs(B, 0.45, M)

    def call(x):
        out = eng.ranking_loss(x["im"], x["s"], kind, M, R.SCALES[kind], need_grad=need_grad)
        return tuple(t for t in out if t is not None)

    plain, _ = run_guarded(call, {"im": dev(im.copy()), "s": dev(s.copy())}, 3 if need_grad else 1)
    rl, rgi, rgs = R.conditioned_reference(B, 0.45, M, kind)
    R.assert_loss(float(plain[0].item()), rl, "loss")
    if need_grad:
        R.assert_grad(plain[1].cpu().numpy(), rgi, kind, "d im")
        R.assert_grad(plain[2].cpu().numpy(), rgs, kind, "d s")


def ranking_call(kind, B, scale):
    im, s, _ = R.conditioned_inputs(B, 0.45, M)
    d_im, d_s = dev(im * np.float32(scale)), dev(s * np.float32(scale))

    def call(e):
        loss, g_im, g_s = e.ranking_loss(d_im, d_s, kind, M, R.SCALES[kind])
        forward_only = e.ranking_loss(d_im, d_s, kind, M, R.SCALES[kind], need_grad=False)[0]
        return {"loss": loss, "grad_im": g_im, "grad_s": g_s, "forward_only": forward_only}

    return call


@pytest.mark.parametrize("kind", R.KINDS)
def test_ranking_loss_after_1024_non_finite_rows_and_a_contrastive_call(kind):
    """Rows x 1e30 overflow their squared norms and their products (1e60): the inverse norms are 0, every cosine of the 1024-row
    call is inf * 0 = NaN, and that is what stays in the workspace, which the contrastive call before it sized and filled otherwise. 33 rows (fused: no workspace), 129 and 200 (the chain at other strides)."""
    contrastive, huge = loss_call(200, 1.0, 200), ranking_call(kind, 1024, 1e30)

    def dirty(e):
        contrastive(e)
        huge(e)

    check_history(engine, dirty, [ranking_call(kind, 33, 1.0), ranking_call(kind, 129, 1.0), ranking_call(kind, 200, 1.0)])


@pytest.mark.parametrize("kind", R.KINDS)
def test_contrastive_loss_after_a_ranking_call(kind):
    check_history(engine, ranking_call(kind, 1024, 1e30), [loss_call(129, 1.0, 129), loss_call(33, 1.0, 33)])
