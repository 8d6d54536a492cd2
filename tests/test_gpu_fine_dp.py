"""GPU tier: the fine stage's data-parallel step takes THE REFERENCE'S step. The reference trains one process on the whole batch
(training/fine.py:38-91): every BatchNorm1d of the ObjectEncoder normalises over the 16 * B objects of all B pairs. With cross-rank
BatchNorm statistics in t2l_fine_train_forward / _backward (t2l_train_sync_bn: each stage's per-channel sums are added up over the
ranks between its statistics and its apply launch) W ranks x 8/W pairs reproduce the goldens of the reference's own B = 8 step
(tests/golden/fine_train_{embed,pn,text}.npz): offsets, loss, the averaged parameter gradients, d hint encodings, the running
statistics. The fine loss is a MEAN over the local rows, so a rank's gradients are W times its share of the one-process gradient and
the ranks' MEAN is the one-process gradient. Dropout is 0 throughout. Processes share GPU 0 under gloo, as in tests/test_gpu_sync_bn.py
(at most 4 here)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_gpu_sync_bn import GOLDEN, _free_port, _slice_cells

pytestmark = pytest.mark.gpu
ALL = ("class", "color", "position", "num")
# exchanges per direction with all four features: layer 0 of the branches' MLPs, layer 1, mlp_merge (include/t2l.h)
STAGES = 3
NOISE = (".0.bias", "num_encoder.0.0.weight")  # in front of a BatchNorm: true gradient 0 / an eps residual


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _engine_worker(rank, world, port, name, sync, out_q):
    dist = _init(rank, world, port)
    from tests.test_gpu_fine_train import bind
    from tests.test_oracle_fine_train import golden_case
    from text2loc_amd.engine import Engine

    g = np.load(os.path.join(GOLDEN, f"fine_train_{name}.npz"), allow_pickle=True)
    embed, L, sd, cells, pn = golden_case(g)
    B = len(g["targets"])
    lo, hi = rank * B // world, (rank + 1) * B // world
    eng = Engine(0)
    tensors = bind(eng, sd, embed, ALL, L)
    if sync:
        eng.train_sync_bn()
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _slice_cells(cells, lo, hi).items()}
    h = torch.from_numpy(np.ascontiguousarray(g["hint_encodings"][lo:hi])).cuda()
    pnt = None if pn is None else torch.from_numpy(np.ascontiguousarray(pn[16 * lo:16 * hi])).cuda()
    out = eng.fine_train_forward(packed, pnt, h, dropout_p=0.0, seed=0)
    o = out.detach().clone().requires_grad_(True)
    loss = float(g["offset_lambda"]) * torch.nn.MSELoss()(o, torch.from_numpy(g["targets"][lo:hi]).cuda())
    loss.backward()
    gh = torch.empty_like(h)
    gp = None if pnt is None else torch.empty_like(pnt)
    eng.fine_train_backward(o.grad.contiguous(), gh, gp)
    torch.cuda.synchronize()
    grads = {}
    for n in [str(x) for x in g["used_params"]]:
        t = tensors[n][1].cpu()
        dist.all_reduce(t)  # what optim.Adam(data_parallel=True, grad_reduce="mean") does on the flat buffer
        grads[n] = (t / world).numpy()
    bufs = {k: v[0].cpu().numpy() for k, v in tensors.items() if "running_" in k}
    out_q.put((rank, out.cpu().numpy(), float(loss), grads, bufs, eng.sync_bn_calls(), gh.cpu().numpy() / world,
               None if gp is None else gp.cpu().numpy() / world))
    dist.barrier()
    eng.close()
    dist.destroy_process_group()


def _run(target, world, *args):
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (out_q,)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([out_q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=120)
    assert [p.exitcode for p in procs] == [0] * world
    return res


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.sqrt((b ** 2).mean()), 1e-30))


@pytest.mark.parametrize("world,name", [(2, "embed"), (2, "pn"), (4, "embed")])
def test_ranks_with_cross_rank_batchnorm_take_the_reference_step(world, name):
    """The bounds of tests/test_gpu_fine_train.py::test_step_matches_the_reference_goldens, for the one-process step."""
    from tests.test_oracle_fine_train import grad_errors

    g = np.load(os.path.join(GOLDEN, f"fine_train_{name}.npz"), allow_pickle=True)
    B = len(g["targets"])
    res = _run(_engine_worker, world, name, True)
    assert abs(np.mean([r[2] for r in res]) - float(g["loss"])) < 1e-4 * max(1.0, float(g["loss"]))
    for rank, out, loss, grads, bufs, calls, gh, gp in res:
        lo, hi = rank * B // world, (rank + 1) * B // world
        assert calls == 2 * STAGES
        assert np.abs(out - g["offsets_out"][lo:hi]).max() < 1e-4
        ref_gh = g["grad_hint"].astype(np.float64)
        assert np.abs(gh - ref_gh[lo:hi]).max() / np.sqrt((ref_gh ** 2).mean()) < 2e-3
        if gp is not None:
            ref_gp = g["grad_pn"].astype(np.float64)
            assert np.abs(gp - ref_gp[16 * lo:16 * hi]).max() / np.sqrt((ref_gp ** 2).mean()) < 2e-3
        for n in [str(x) for x in g["used_params"]]:
            err, rms = grad_errors(g, n, grads[n])
            if n.startswith("object_encoder.") and n.endswith(".0.bias"):
                assert err < 1e-4, n  # true gradient 0 (a BatchNorm follows)
                continue
            if n.endswith("num_encoder.0.0.weight"):
                assert err < 2e-4, n  # scale-invariant [64,1] Linear before a BatchNorm: an eps residual
                continue
            assert err < 2e-3 * rms + 1e-9, (n, err, rms)
            nrm = float(np.sqrt((grads[n].astype(np.float64) ** 2).sum()))
            assert abs(nrm - float(g[f"grad_norm/{n}"])) < 2e-3 * float(g[f"grad_norm/{n}"]), n
        for k in g.files:
            if k.startswith("buf/"):
                assert np.allclose(bufs[k[4:]], g[k], rtol=2e-4, atol=2e-5), k
    for r in res[1:]:  # every rank holds the same reduced gradients and running statistics, bit for bit
        for n, v in res[0][3].items():
            assert np.array_equal(v, r[3][n]), n
        for n, v in res[0][4].items():
            assert np.array_equal(v, r[4][n]), n


def test_per_rank_statistics_do_not_take_the_reference_step():
    """The control: without the exchange two ranks x 4 pairs normalise over their own 64 objects, not the batch's 128 — a different
    (legitimate) model of the step, measurably not the reference's."""
    g = np.load(os.path.join(GOLDEN, "fine_train_embed.npz"), allow_pickle=True)
    res = _run(_engine_worker, 2, "embed", False)
    assert all(r[5] == 0 for r in res)
    assert max(np.abs(r[1] - g["offsets_out"][4 * r[0]:4 * r[0] + 4]).max() for r in res) > 1e-4


# ---- the hint encoder's BatchNorm joins -----------------------------------------------------------------------------------------
def _text_worker(rank, world, port, out_q):
    dist = _init(rank, world, port)
    from tests.test_gpu_fine_text_train import _cross_match
    from tests.test_oracle_fine_text import golden_text_case

    g = np.load(os.path.join(GOLDEN, "fine_train_text.npz"), allow_pickle=True)
    _, hidden, B, S = golden_text_case(g)
    lo, hi = rank * B // world, (rank + 1) * B // world
    model, t5, objects = _cross_match(int(g["weight_seed"]), int(g["head_seed"]), int(g["cell_seed"]), B)
    t5.hidden = torch.from_numpy(np.ascontiguousarray(hidden[lo * S:hi * S]))
    model.train()
    model.sync_batchnorm()
    kept = {}
    hook = model.language_encoder.register_forward_hook(lambda mod, i, o: kept.update(hints=o))
    out = model(objects[lo:hi], [" ".join(["The pose is north of a gray pole."] * S)] * (hi - lo), None)
    hook.remove()
    loss = float(g["offset_lambda"]) * torch.nn.MSELoss()(out, torch.from_numpy(g["targets"][lo:hi]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {}
    for n in [str(x) for x in g["used_params"]]:
        t = dict(model.named_parameters())[n].grad.cpu()
        dist.all_reduce(t)
        grads[n] = (t / world).numpy()
    bufs = {n: b.cpu().numpy() for n, b in model.named_buffers() if "running_" in n}
    out_q.put((rank, out.detach().cpu().numpy(), float(loss.detach()), grads, bufs,
               (model._engine.sync_bn_calls(), model.language_encoder._th_train_engine.sync_bn_calls()),
               kept["hints"].detach().cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_the_hint_encoders_batchnorm_joins():
    """2 x 4 poses against the reference's B = 8 step with the real ``LanguageEncoder(is_fine=True)`` (fine_train_text.npz): inter_mlp's
    BatchNorm over the 48 hints of BOTH ranks (the text slots), the ObjectEncoder's over the 128 objects."""
    from tests.test_oracle_train import golden_view

    g = np.load(os.path.join(GOLDEN, "fine_train_text.npz"), allow_pickle=True)
    B, world = int(g["batch"]), 2
    res = _run(_text_worker, world)
    assert abs(np.mean([r[2] for r in res]) - float(g["loss"])) < 1e-4 * max(1.0, float(g["loss"]))
    for rank, out, loss, grads, bufs, calls, hints in res:
        lo, hi = rank * B // world, (rank + 1) * B // world
        assert calls == (2 * STAGES, 2)
        assert np.abs(hints - g["hint_encodings"][lo:hi]).max() < 5e-5 * max(1.0, np.abs(g["hint_encodings"]).max())
        assert np.abs(out - g["offsets_out"][lo:hi]).max() < 1e-4
        for n in [str(x) for x in g["used_params"]]:  # the rule of test_cross_match_train_step_with_the_text_branch_matches_the_reference_step
            exp, got = golden_view(g, "grad", n, grads[n])
            rms = float(g[f"grad_norm/{n}"]) / np.sqrt(max(grads[n].size, 1))
            if n.endswith(("inter_mlp.0.0.bias", "intra_module.0.norm2.bias")):
                assert np.abs(got).max() < 1e-4, n
                continue
            if n.endswith("in_proj_bias") and len(got) <= 1024:
                D = len(got) // 3
                sel = np.r_[0:D, 2 * D:3 * D]
                exp, got = exp[sel], got[sel]
            err = np.abs(got - exp)
            assert (err < 1e-2 * rms + 1e-6).mean() >= 0.95 and err.max() < 0.2 * rms + 1e-5, (n, float(err.max()), rms)
        for k in g.files:
            if k.startswith("buf/") and "running_" in k:
                assert np.allclose(bufs[k[4:]], g[k], rtol=2e-4, atol=2e-5), k
    for n, v in res[0][4].items():
        assert np.array_equal(v, res[1][4][n]), n


# ---- the whole optimizer step ---------------------------------------------------------------------------------------------------
def _whole_batch():
    from tests.test_gpu_fine_text_train import _no_dropout
    from tests.test_gpu_fine_train import drop_in

    model, objects, texts, pts, target = drop_in()
    _no_dropout(model)
    return model.train(), objects, texts, torch.from_numpy(target).cuda()


def _adam_worker(rank, world, port, out_q):
    _init(rank, world, port)
    from text2loc_amd import optim

    model, objects, texts, target = _whole_batch()
    B = len(objects)
    lo, hi = rank * B // world, (rank + 1) * B // world
    sent = []
    plain = optim.all_reduce_flat

    def counted(buf, group=None, mean=False):
        sent.append((int(buf.numel()), bool(mean)))
        return plain(buf, group, mean)

    optim.all_reduce_flat = counted
    opt = optim.Adam(model, lr=1e-3, data_parallel=True, sync_bn=True, grad_reduce="mean")
    w0 = {n: q.detach().clone() for n, q in model.named_parameters()}
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects[lo:hi], texts[lo:hi], None), target[lo:hi]).backward()
    opt.step()
    torch.cuda.synchronize()
    import torch.distributed as dist

    out_q.put((rank, {n: q.detach().cpu().numpy() for n, q in model.named_parameters()},
               {n: b.cpu().numpy() for n, b in model.named_buffers() if "running_" in n}, sent, int(model.train_flat_grad().numel()),
               model._engine.sync_bn_calls(), {n for n, q in model.named_parameters() if not torch.equal(q.detach(), w0[n])}))
    dist.barrier()
    dist.destroy_process_group()


def test_a_data_parallel_adam_step_is_the_one_process_step():
    """optim.Adam(model, data_parallel=True, sync_bn=True, grad_reduce="mean") on 2 ranks x 3 pairs against the engine's own step on
    the 6 pairs in one process: the gradient bounds above through one Adam step (lr * sign(grad) where the gradient is live: 2e-5),
    and exactly two gradient collectives — the flat buffer, then everything else."""
    from text2loc_amd import optim

    model, objects, texts, target = _whole_batch()
    opt = optim.Adam(model, lr=1e-3)
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(objects, texts, None), target).backward()
    ref_grads = {n: q.grad.detach().cpu().numpy().astype(np.float64) for n, q in model.named_parameters() if q.grad is not None}
    opt.step()
    ref = {n: q.detach().cpu().numpy() for n, q in model.named_parameters()}
    ref_bufs = {n: b.cpu().numpy() for n, b in model.named_buffers() if "running_" in n}
    assert "language_encoder.table" in ref_grads and "cross_objects.1.linear2.weight" in ref_grads
    # the second collective: the text branch's table and what this configuration never differentiates (as zeros: the list is rank-independent)
    n_rest = sum(int(q.numel()) for n, q in model.named_parameters() if q.requires_grad and not model.engine_steps(n, q))
    res = _run(_adam_worker, 2)
    for rank, params, bufs, sent, n_flat, calls, moved in res:
        assert sent == [(n_flat, True), (n_rest, True)], sent
        assert calls == 2 * STAGES
        assert moved <= set(ref_grads) and "language_encoder.table" in moved  # never differentiated: never stepped
        for n in ref_grads:  # (what this configuration never runs keeps the fixture's per-process random initialisation)
            v = params[n]
            if n.startswith("object_encoder.") and n.endswith(NOISE):
                continue
            gr = np.abs(ref_grads[n])
            live = gr > 1e-2 * max(np.sqrt((gr ** 2).mean()), 1e-12)
            assert np.abs(v - ref[n])[live].max(initial=0.0) < 2e-5, n
        for n, v in bufs.items():
            assert np.allclose(v, ref_bufs[n], rtol=2e-4, atol=2e-5), n
    for n in ref_grads:  # the ranks stay in step, bit for bit
        assert np.array_equal(res[0][1][n], res[1][1][n]), n
