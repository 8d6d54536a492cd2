"""GPU tier: the rows of the two tiers of DESIGN.md 1a for t2l_pointnet_cls_forward / _heads / _backward. Guard bands
(tests/guards.py, ``run_guarded`` of tests/test_gpu_memory_safety.py): inputs — the bound head tensors and their gradient buffers
included — between NaN and 3e38 halos, outputs carved from patterned buffers: halos intact, outputs written in full, the bits of the
ordinary run. Call history (tests/test_gpu_call_history.py): a small call behind a larger one that left the partial-sum workspace
of the heads and the backbone's activation workspace full of huge and non-finite values gives the bits of a fresh context.
Logits, loss, counts, d features2 and features2 have a fixed summation order (bit identity at every n); the head gradients are
summed over workgroups with float atomics, so they are held to the same bits up to one workgroup (32 rows) only, and the backbone's
gradients (atomics throughout) to closeness."""
import numpy as np
import pytest
import torch

from tests import pointnet_cls_ref as R
from tests.test_gpu_call_history import check_history
from tests.test_gpu_memory_safety import dev, engine, run_guarded
from tests.test_gpu_pointnet_pretrain import assert_heads, step_inputs
from text2loc_amd import synth

pytestmark = pytest.mark.gpu

P = R.P
HEAD_KEYS = [P + h + s for h in R.HEADS for s in (".weight", ".bias")]


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


def backbone_tensors(sd):
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked") or "classifier" in k:
            continue
        t = dev(np.asarray(v, dtype=np.float32))
        out[k] = (t, None if "running_" in k else torch.zeros_like(t))
    return out


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "forward"])
@pytest.mark.parametrize("classes", R.HEAD_CLASSES)
@pytest.mark.parametrize("n", R.HEAD_ROWS)
def test_heads_guard_bands(eng, n, classes, need_grad):
    x, sd, lc, lk, ref, b = R.heads_case(n, classes)
    back = backbone_tensors(sd)
    args = {"x": dev(x)}
    for k in HEAD_KEYS:
        args[k] = dev(np.asarray(sd[k], dtype=np.float32))
        args[k + ".grad"] = torch.zeros_like(args[k])
    one_wg = n <= R.ROWS_PER_WG

    def call(a):
        tensors = dict(back)
        tensors.update({k: (a[k], a[k + ".grad"]) for k in HEAD_KEYS})
        eng.pointnet_cls_bind(tensors)
        out = eng.pointnet_cls_heads(a["x"], lc, lk, R.W_CLASS, R.W_COLOR, need_grad=need_grad)
        out = tuple(t for t in out if t is not None)
        if not need_grad:  # no gradient buffer is touched
            assert all(not a[k + ".grad"].any() for k in HEAD_KEYS)
        return out + (tuple(a[k + ".grad"] for k in HEAD_KEYS) if need_grad and one_wg else ())

    plain, _ = run_guarded(call, args, 4 if need_grad else 3)
    got = (plain[0], plain[1], plain[2], plain[3] if need_grad else None)
    grads = {k: (None, g) for k, g in zip(HEAD_KEYS, plain[4:])} if need_grad and one_wg else None
    assert_heads(got, ref, b, grads, f"guarded n={n} classes={classes}")


@pytest.mark.parametrize("n_obj", [1, 3])
def test_forward_and_backward_guard_bands(eng, n_obj):
    pos, rgb, sd, lc, lk = step_inputs(n_obj, 60 + n_obj)
    grad = np.random.default_rng(n_obj).standard_normal((n_obj, 256)).astype(np.float32)
    state = {}

    def forward(a):
        state["tensors"] = backbone_tensors(sd)
        state["tensors"].update({k: (dev(np.asarray(sd[k], dtype=np.float32)), dev(np.zeros_like(sd[k], dtype=np.float32))) for k in HEAD_KEYS})
        eng.pointnet_cls_bind(state["tensors"])
        return (eng.pointnet_cls_forward(a["pos"], a["rgb"]),)

    run_guarded(forward, {"pos": dev(pos), "rgb": dev(rgb)}, 1)

    def backward(a):  # (behind the last guarded forward: its activations)
        for v in state["tensors"].values():
            if v[1] is not None:
                v[1].zero_()
        eng.pointnet_cls_backward(a["g"])
        return (state["tensors"][P + "lin2.weight"][1].clone(), state["tensors"][P + "sa1.point_conv.local_nn.1.0.weight"][1].clone())

    plain, runs = run_guarded(backward, {"g": dev(grad)}, 0, exact=False)
    for out in runs:
        for a, b in zip(out, plain):
            assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=1e-3, atol=1e-5 * float(b.abs().max()) + 1e-9)
    assert plain[0].abs().max() > 0


def heads_call(n, classes, scale=1.0):
    x, sd, lc, lk, _, _ = R.heads_case(n, classes) if (n, classes) in R.HEAD_SEEDS else (R.make_heads_inputs(n, classes, 0) + (None, None))
    d_x = dev(x * np.float32(scale))

    def call(e):
        tensors = backbone_tensors(sd)
        tensors.update({k: (dev(np.asarray(sd[k], dtype=np.float32)), dev(np.zeros_like(sd[k], dtype=np.float32))) for k in HEAD_KEYS})
        e.pointnet_cls_bind(tensors)
        logits, loss, correct, dx = e.pointnet_cls_heads(d_x, lc, lk, R.W_CLASS, R.W_COLOR)
        fwd = e.pointnet_cls_heads(d_x, lc, lk, R.W_CLASS, R.W_COLOR, need_grad=False)
        out = {"logits": logits, "loss": loss, "correct": correct, "dx": dx, "forward_only_loss": fwd[1], "forward_only_correct": fwd[2]}
        if n <= R.ROWS_PER_WG:  # one workgroup: the atomics add one value to zero
            out.update({k: tensors[k][1] for k in HEAD_KEYS})
        return out

    return call


def step_call(n_obj, seed, rgb_scale=1.0):
    pos, rgb, sd, lc, lk = step_inputs(n_obj, seed)
    d_pos, d_rgb = dev(pos), dev(rgb * np.float32(rgb_scale))

    def call(e):
        tensors = backbone_tensors(sd)
        tensors.update({k: (dev(np.asarray(sd[k], dtype=np.float32)), dev(np.zeros_like(sd[k], dtype=np.float32))) for k in HEAD_KEYS})
        e.pointnet_cls_bind(tensors)
        f2 = e.pointnet_cls_forward(d_pos, d_rgb)
        logits, loss, correct, dx = e.pointnet_cls_heads(f2, lc, lk)
        e.pointnet_cls_backward(dx)  # (its gradients are atomically summed: run, not compared)
        return {"features2": f2, "logits": logits, "loss": loss, "correct": correct, "dx": dx}

    return call


def test_small_calls_after_large_non_finite_ones():
    """The dirtying calls: 200 rows of features2 x 1e30 (logits overflow: the per-workgroup loss partials of 7 workgroups are inf / NaN)
    and a 12-object step whose colours x 1e30 overflow every activation of the backbone's workspace."""
    huge_heads, huge_step = heads_call(200, (22, 8), 1e30), step_call(12, 90, 1e30)

    def dirty(e):
        huge_heads(e)
        huge_step(e)

    check_history(engine, dirty, [heads_call(5, (22, 8)), heads_call(70, (2, 32)), step_call(2, 91)])
