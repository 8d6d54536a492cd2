"""GPU tier, DESIGN.md 1a for the fine stage's new entry points — t2l_fine_zero_grad, t2l_fine_adam_step, t2l_fine_adam_state and the
cross-rank form of t2l_fine_train_forward / _backward (t2l_train_sync_bn set) — in the two forms the existing entry points are held
to: between guard bands (tests/guards.py: poisoned halos, patterned outputs; tests/test_gpu_memory_safety.py) and behind a dirtying
call (tests/test_gpu_call_history.py: a small call after a large one that left huge and non-finite contents in the workspaces, the
moments and the accumulator slots must give the bits and counters of a fresh context).

The cross-rank sum of ONE rank is the identity, so the callback here only counts: the step must then equal the one-process step
(the float64 twin's bars of tests/test_gpu_fine_train.py), and its slots — handed over full of NaN — must be stored before they are read."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guards as G
from tests.test_gpu_call_history import check_history
from tests.test_gpu_fine_train import ALL, bind, rel
from tests.test_gpu_memory_safety import cell_int_fills, dev, engine, run_guarded, same_bits
from tests.test_oracle_fine_train import problem
from text2loc_amd import engine as E

pytestmark = pytest.mark.gpu
STAGES = 3  # exchanges per direction with all four features (include/t2l.h)


def one_rank_sync(e):
    """t2l_train_sync_bn with the sum over a world of one: nothing to add, one more call counted. The slots start as NaN."""
    n = int(e.lib.t2l_train_sync_bn_doubles())
    buf = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    calls = [0]

    def _sum(_user, _ptr, _count, _stream):
        calls[0] += 1
        return 0

    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(_sum)
    e._check(e.lib.t2l_train_sync_bn(e._h, buf.data_ptr(), n, C.cast(cb, C.c_void_p), None))
    e._sync_bn = (buf, cb, calls)  # (the library keeps raw pointers to both)
    return e


def step_args(cells, hints, pn, gout):
    args = {k: dev(v) for k, v in cells.items() if k != "counts"}
    args.update(pn=dev(pn), hints=dev(hints), gout=dev(gout), gh=torch.zeros(hints.shape, device="cuda"), gp=torch.zeros(pn.shape, device="cuda"))
    return args


def step(e, cells, a):
    off = e.fine_train_forward({k: v for k, v in a.items() if k in cells and k != "counts"}, a["pn"], a["hints"], dropout_p=0.0, seed=0)
    e.fine_train_backward(a["gout"], a["gh"], a["gp"])
    return off


# ------------------------------------------------------------------------------------------------------------------ guard bands
def test_sync_forward_and_backward_between_guard_bands():
    """The case of test_gpu_memory_safety.py::test_fine_train_forward_and_backward (5 pairs, 6 hints, 1 layer, PointNet mode: all four
    MLP branches, a features2 gradient) with the cross-rank form on."""
    from tests.fine_train_twin import Twin

    B, H, L = 5, 6, 1
    sd, cells, hints, pn, gout = problem(False, L, P=B, H=H, seed=B + H, use=ALL)
    off_t, g_t, gh_t, gp_t = Twin(sd, False, False, ALL, L).step(cells, hints, gout, pn)
    e = one_rank_sync(engine())
    try:
        bound = {}

        def call(a):
            bound["t"] = bind(e, sd, False, ALL, L)
            return step(e, cells, a), a["gh"], a["gp"]

        n0 = e.sync_bn_calls()
        plain, runs = run_guarded(call, step_args(cells, hints, pn, gout), 1, ints=cell_int_fills(cells), exact=False)
        assert e.sync_bn_calls() - n0 == 3 * 2 * STAGES
        for off, gh, gp in [plain] + runs:
            assert np.abs(off.cpu().numpy() - off_t).max() < 1e-4
            assert rel(gh.cpu().numpy(), gh_t) < 2e-3 and rel(gp.cpu().numpy(), gp_t) < 2e-3
        for n in ("object_encoder.mlp_merge.0.1.weight", "object_encoder.pos_encoder.1.1.bias", "object_encoder.mlp_pointnet.0.1.weight"):
            assert rel(bound["t"][n][1].cpu().numpy(), g_t[n]) < 2e-3, n  # dγ / dβ: taken in the statistics launch
    finally:
        e.close()


def optimizer_tensors(L, seed, fill):
    """The embedding configuration's tensors with every parameter, gradient and running buffer between halos of ``fill`` (None: plain)."""
    sd, _, _, _, _ = problem(True, L, seed=seed)
    rng = np.random.default_rng(seed)
    wrap = (lambda t: t) if fill is None else (lambda t: G.guarded(t, fill))
    tensors = {}
    for k, v in sd.items():
        if k.startswith(("language_encoder.", "object_encoder.pointnet.")) or k.endswith("num_batches_tracked"):
            continue
        t = wrap(dev(np.asarray(v, dtype=np.float32)))
        frozen = "running_" in k or k == "mlp_offsets.2.bias"
        tensors[k] = (t, None if frozen else wrap(dev(rng.standard_normal(np.shape(v)).astype(np.float32))))
    return tensors


def optimizer_run(e, L, fill):
    tensors = optimizer_tensors(L, 3, fill)
    e.fine_train_bind(tensors, class_embed=True, color_embed=True, use_features=ALL, num_layers=L)
    e.fine_adam_step(1e-3)
    e.fine_zero_grad()
    return tensors


def test_zero_grad_adam_step_and_state_between_guard_bands():
    """Bound parameters, gradients and buffers all between halos (sizes from 2 to 3 * 128 * 128 elements: chunks that end inside a
    1024-element workgroup), the moments returned into patterned buffers and taken from guarded ones."""
    e = engine()
    try:
        plain = optimizer_run(e, 0, None)
        m0, v0, s0 = e.fine_adam_state()
        for fill in G.FLOAT_FILLS:
            t = optimizer_run(e, 0, fill)
            with G.guarded_outputs(E) as g:
                m, v, s = e.fine_adam_state()
            assert g.count == 2 and s == s0 == 1
            assert same_bits(m, m0) and same_bits(v, v0)
            flat = [x for pair in t.values() for x in pair if x is not None]
            G.check_halos(*flat)
            for n, (p, gr) in t.items():
                assert same_bits(p, plain[n][0]), n  # frozen tensors and running buffers included: they equal their initial values
                assert gr is None or not bool(gr.any()), n
            gm, gv = G.guarded(m0 * 2, fill), G.guarded(v0 * 3, fill)
            e.set_fine_adam_state(gm, gv, 7)
            G.check_halos(gm, gv)
            m2, v2, s2 = e.fine_adam_state()
            assert s2 == 7 and same_bits(m2, m0 * 2) and same_bits(v2, v0 * 3)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ call history
def poisoned_step(e, L):
    """33 pairs, 8 hints, L layers, PointNet mode, through hint encodings and an offsets gradient full of huge and non-finite values:
    the arena, the gradients it is bound to, and with them the next Adam step's moments, end up non-finite."""
    sd, cells, hints, pn, gout = problem(False, L, P=33, H=8, seed=9)
    hints = hints.copy()
    hints.reshape(-1)[::7] = np.float32(3e38)
    hints.reshape(-1)[3::11] = np.nan
    hints.reshape(-1)[5::13] = -np.inf
    gout = np.full_like(gout, 3e38)
    bind(e, sd, False, ALL, L)
    step(e, cells, step_args(cells, hints, pn, gout))
    e.fine_adam_step(1e30)
    torch.cuda.synchronize()


def test_the_optimizer_does_not_depend_on_what_an_earlier_binding_left():
    def small(e):
        t = optimizer_run(e, 0, None)
        for _, g in t.values():
            if g is not None:
                g.fill_(0.5)
        e.fine_adam_step(3e-3, 0.8, 0.99, 1e-6)
        m, v, s = e.fine_adam_state()
        return {"params": torch.cat([p.reshape(-1) for p, _ in t.values()]), "m": m, "v": v, "step": s}

    check_history(engine, lambda e: poisoned_step(e, 4), [small])


def test_the_sync_step_does_not_depend_on_what_an_earlier_step_left():
    """S: 2 pairs, 3 hints, 1 layer, PointNet mode — no embedding scatter and one workgroup per reduction, so the whole step is
    deterministic: offsets, both returned gradients, the running statistics and the exchange count, bit for bit."""
    sd, cells, hints, pn, gout = problem(False, 1, P=2, H=3, seed=5)

    def small(e):
        t = bind(e, sd, False, ALL, 1)
        a = step_args(cells, hints, pn, gout)
        n0 = e.sync_bn_calls()
        off = step(e, cells, a)
        out = {"off": off, "gh": a["gh"], "gp": a["gp"], "exchanges": e.sync_bn_calls() - n0}
        out.update({n: b for n, (b, _) in t.items() if "running_" in n})
        out.update({"d " + n: t[n][1] for n in ("object_encoder.mlp_merge.0.1.weight", "object_encoder.num_encoder.0.1.bias")})
        return out

    def make():
        return one_rank_sync(engine())

    check_history(make, lambda e: poisoned_step(e, 4), [small])
    e = make()
    try:
        ref = small(e)
        assert ref["exchanges"] == 2 * STAGES and bool(torch.isfinite(ref["off"]).all()) and bool(torch.isfinite(ref["gp"]).all())
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ a failing callback
def test_a_failing_callback_fails_the_step_and_ends_its_exchanges():
    """The callback returns non-zero at its k-th call: that forward (k <= 3) or backward fails with T2L_ESTATE and issues no further
    exchange; a forward that failed cannot be differentiated; the next step runs again."""
    from text2loc_amd.engine import T2LError

    sd, cells, hints, pn, gout = problem(False, 1, P=2, H=3, seed=5)
    for fail_at in (1, 2, 3, 4, 6):
        e = engine()
        try:
            n = int(e.lib.t2l_train_sync_bn_doubles())
            buf = torch.zeros((n,), dtype=torch.float64, device="cuda")
            calls, armed = [0], [True]

            def _sum(_user, _ptr, _count, _stream):
                calls[0] += 1
                return 1 if (armed[0] and calls[0] == fail_at) else 0

            cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(_sum)
            e._check(e.lib.t2l_train_sync_bn(e._h, buf.data_ptr(), n, C.cast(cb, C.c_void_p), None))
            e._sync_bn = (buf, cb, calls)
            bind(e, sd, False, ALL, 1)
            a = step_args(cells, hints, pn, gout)
            with pytest.raises(T2LError, match="callback"):
                step(e, cells, a)
            assert calls[0] == fail_at  # nothing was exchanged behind the failure
            if fail_at <= STAGES:
                with pytest.raises(T2LError, match="no training-mode forward"):
                    e.fine_train_backward(a["gout"], a["gh"], a["gp"])
            armed[0] = False
            off = step(e, cells, a)
            torch.cuda.synchronize()
            assert calls[0] == fail_at + 2 * STAGES and bool(torch.isfinite(off).all())
        finally:
            e.close()
