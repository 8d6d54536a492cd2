"""GPU tier: the pairwise and hardest ranking losses on the engine (t2l_ranking_loss: one launch up to 128 rows, six beyond) against
the float64 reference of tests/ranking_loss_ref.py on conditioned inputs — the loss to 3e-5 relative, every gradient element to
RANK_T * rms(reference tensor) + 1e-9, the bar derived there from the float32 CPU evaluation of the torch mirror — then the modules,
the refusals, ``coarse.train_epoch`` under ``--ranking_loss pairwise`` and the global batch of two ranks."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import ranking_loss_ref as R

pytestmark = pytest.mark.gpu

M = 0.35


@pytest.fixture(scope="module")
def eng():
    from text2loc_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()  # a copy: the shared inputs are read-only


def run(eng, im, s, kind, margin, need_grad=True):
    loss, g_im, g_s = eng.ranking_loss(dev(im), dev(s), kind, margin, R.SCALES[kind], need_grad=need_grad)
    torch.cuda.synchronize()
    if not need_grad:
        assert g_im is None and g_s is None
        return float(loss.item()), None, None
    return float(loss.item()), g_im.cpu().numpy(), g_s.cpu().numpy()


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_golden(eng, golden, kind):
    """The imported reference's own value and autograd gradients at B = 24 (tests/golden/loss_ranking.npz), and the float64
    reference on the same rows (min |hinge| 3e-4, min gap 1e-3 there: decidable in float32)."""
    g = golden("loss_ranking")
    m = float(g["margin"])
    loss, g_im, g_s = run(eng, g["im"], g["s"], kind, m)
    R.assert_loss(loss, float(g[kind + "_loss"]), "golden")
    R.assert_grad(g_im, g[kind + "_grad_im"].astype(np.float64), kind, "golden d im")
    R.assert_grad(g_s, g[kind + "_grad_s"].astype(np.float64), kind, "golden d s")
    rl, rgi, rgs = R.ranking_loss_ref(g["im"], g["s"], kind, m)
    R.assert_loss(loss, rl, "float64")
    R.assert_grad(g_im, rgi, kind, "d im")
    R.assert_grad(g_s, rgs, kind, "d s")


@pytest.mark.parametrize("B,a,m", R.CASES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_conditioned_batches(eng, kind, B, a, m):
    """1..128 rows: the fused kernel and its 32-row tile edges; 129, 300, 1024: the chain. With gradients and forward only."""
    im, s, _ = R.conditioned_inputs(B, a, m)
    rl, rgi, rgs = R.conditioned_reference(B, a, m, kind)
    loss, g_im, g_s = run(eng, im, s, kind, m)
    print(f"{kind} B={B} a={a} m={m}: loss rel err {abs(loss - rl) / abs(rl) if rl else abs(loss):.2e}, "
          f"d im {R.grad_errors(g_im, rgi):.2e} rms, d s {R.grad_errors(g_s, rgs):.2e} rms (T = {R.RANK_T[kind]:.1e})")
    R.assert_loss(loss, rl, "loss")
    R.assert_grad(g_im, rgi, kind, "d im")
    R.assert_grad(g_s, rgs, kind, "d s")
    forward, _, _ = run(eng, im, s, kind, m, need_grad=False)
    assert abs(forward - loss) <= 1e-7 * abs(loss)
    if B == 1:
        assert loss == 0.0 and not g_im.any() and not g_s.any()


@pytest.mark.parametrize("B", [33, 128, 300])
@pytest.mark.parametrize("kind", R.KINDS)
def test_same_bits_every_run(eng, kind, B):
    im, s, _ = R.conditioned_inputs(B, 0.9, M)
    d_im, d_s = dev(im), dev(s)
    first = [t.clone() for t in eng.ranking_loss(d_im, d_s, kind, M, R.SCALES[kind])]
    again = eng.ranking_loss(d_im, d_s, kind, M, R.SCALES[kind])
    torch.cuda.synchronize()
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ modules
def _crit(kind, **kw):
    from text2loc_amd.losses import HardestRankingLoss, PairwiseRankingLoss

    return PairwiseRankingLoss(M, **kw) if kind == "pairwise" else HardestRankingLoss(M, **kw)


@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("kind", R.KINDS)
def test_modules_take_the_engine_path_and_plug_into_autograd(kind, B):
    im, s, _ = R.conditioned_inputs(B, 0.9, M)
    rl, rgi, rgs = R.conditioned_reference(B, 0.9, M, kind)
    crit = _crit(kind)
    cls = type(crit)
    e0, t0 = cls.engine_calls, cls.torch_calls
    x, y = dev(im).requires_grad_(), dev(s).requires_grad_()
    loss = crit(x, y)
    (2.0 * loss).backward()
    assert (cls.engine_calls, cls.torch_calls) == (e0 + 1, t0)
    R.assert_loss(float(loss.detach()), rl, "module loss")
    R.assert_grad(x.grad.cpu().numpy() / 2, rgi, kind, "module d im (upstream factor 2)")
    R.assert_grad(y.grad.cpu().numpy() / 2, rgs, kind, "module d s (upstream factor 2)")
    with torch.no_grad():  # nothing requires a gradient: the forward-only call
        assert abs(float(crit(dev(im), dev(s))) - float(loss.detach())) <= 1e-7 * abs(rl)
    # the torch formulation on the same device, switched by the instance attribute
    off = _crit(kind)
    off.use_engine = False
    x2, y2 = dev(im).requires_grad_(), dev(s).requires_grad_()
    loss2 = off(x2, y2)
    loss2.backward()
    assert (cls.engine_calls, cls.torch_calls) == (e0 + 2, t0 + 1)
    R.assert_loss(float(loss2.detach()), rl, "torch formulation")
    R.assert_grad(x2.grad.cpu().numpy(), rgi, kind, "torch formulation d im")
    R.assert_grad(x.grad.cpu().numpy() / 2, x2.grad.double().cpu().numpy(), kind, "engine vs torch d im")
    R.assert_grad(y.grad.cpu().numpy() / 2, y2.grad.double().cpu().numpy(), kind, "engine vs torch d s")


@pytest.mark.parametrize("kind", R.KINDS)
def test_modules_keep_other_inputs_on_torch(kind):
    crit = _crit(kind)
    cls = type(crit)
    e0, t0 = cls.engine_calls, cls.torch_calls
    im, s, _ = R.conditioned_inputs(33, 0.9, M)
    cpu = crit(torch.from_numpy(im.copy()), torch.from_numpy(s.copy()))
    R.assert_loss(float(cpu), R.conditioned_reference(33, 0.9, M, kind)[0], "CPU tensors")
    crit(dev(im[:, :128]), dev(s[:, :128]))  # another width
    crit(dev(im).double(), dev(s).double())  # another dtype
    assert (cls.engine_calls, cls.torch_calls) == (e0, t0 + 3)
    cls.use_engine = False  # the class attribute switches every instance
    try:
        crit(dev(im), dev(s))
        assert (cls.engine_calls, cls.torch_calls) == (e0, t0 + 4)
    finally:
        cls.use_engine = True
    crit(dev(im), dev(s))
    assert (cls.engine_calls, cls.torch_calls) == (e0 + 1, t0 + 4)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(eng):
    from text2loc_amd.engine import T2LError, _stream_ptr

    im, s = torch.randn(8, 256, device="cuda"), torch.randn(8, 256, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    g_im, g_s = torch.full_like(im, 7.0), torch.full_like(s, 7.0)
    call = eng.lib.t2l_ranking_loss
    st = _stream_ptr(eng.device)

    def refused(match, *a):
        assert call(eng._h, *a, st) == -1  # T2L_EINVAL
        assert match in eng.lib.t2l_last_error(eng._h).decode()

    p = (im.data_ptr(), s.data_ptr())
    out = (loss.data_ptr(), g_im.data_ptr(), g_s.data_ptr())
    refused("batch", *p, 0, 0, M, 1.0, *out)
    refused("batch", *p, -3, 0, M, 1.0, *out)
    refused("1024", *p, 1025, 0, M, 1.0, *out)
    refused("kind", *p, 8, 2, M, 1.0, *out)
    refused("kind", *p, 8, -1, M, 1.0, *out)
    refused("margin", *p, 8, 0, -0.1, 1.0, *out)
    refused("margin", *p, 8, 1, float("nan"), 1.0, *out)
    refused("margin", *p, 8, 1, float("inf"), 1.0, *out)
    refused("scale", *p, 8, 1, M, float("nan"), *out)
    refused("null", None, s.data_ptr(), 8, 0, M, 1.0, *out)
    refused("null", *p, 8, 0, M, 1.0, None, out[1], out[2])
    refused("both gradients", *p, 8, 0, M, 1.0, out[0], out[1], None)
    refused("both gradients", *p, 8, 0, M, 1.0, out[0], None, out[2])
    refused("16-byte", im.data_ptr() + 4, s.data_ptr(), 7, 0, M, 1.0, *out)
    refused("16-byte", im.data_ptr(), s.data_ptr() + 8, 7, 0, M, 1.0, *out)
    refused("4-byte", *p, 8, 0, M, 1.0, out[0] + 2, out[1], out[2])
    refused("4-byte", *p, 8, 0, M, 1.0, out[0], out[1] + 1, out[2])
    assert call(None, *p, 8, 0, M, 1.0, *out, st) == -1
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((g_im == 7.0).all()) and bool((g_s == 7.0).all())  # nothing ran
    # a row slice is a legal argument: rows are 1 KiB
    l1 = eng.ranking_loss(im[3:], s[3:], "pairwise", M)[0]
    l2 = eng.ranking_loss(im[3:].clone(), s[3:].clone(), "pairwise", M)[0]
    assert torch.equal(l1, l2)
    with pytest.raises(T2LError, match="1024"):
        eng.ranking_loss(torch.zeros(1025, 256, device="cuda"), torch.zeros(1025, 256, device="cuda"), "hardest", M)
    with pytest.raises(T2LError, match="kind"):
        eng.ranking_loss(im, s, "triplet", M)
    with pytest.raises(T2LError, match="CUDA"):
        eng.ranking_loss(im.cpu(), s, "pairwise", M)


# ------------------------------------------------------------------------------------------------------------------ training loop
def test_train_epoch_under_pairwise_tracks_the_torch_formulation():
    """``coarse.train_epoch`` on the synthetic model of tests/test_gpu_train_loop.py with ``make_criterion(args)`` at the reference's
    default (pairwise, margin 0.35), two batches of 16, twice from identical state: engine loss vs ``use_engine = False``."""
    from tests.test_gpu_train_loop import TableText, _args
    from tests.test_host_logic import make_objects
    from text2loc_amd import losses, synth
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork
    from text2loc_amd.coarse import collate_fn, train_epoch
    from text2loc_amd.optim import Adam

    B = 16
    args = _args(ranking_loss="pairwise", margin=0.35)
    cells = synth.make_cells(2 * B, seed=40)
    objects = make_objects(cells, 40)
    weights = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_object_branch_weights(6).items()}

    class Ds(torch.utils.data.Dataset):
        def __len__(self):
            return 2 * B

        def __getitem__(self, i):
            return {"texts": i, "objects": objects[i], "object_points": None}

    def epoch(use_engine):
        model = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=TableText(2 * B, 5))
        model.load_state_dict(weights, strict=False)
        for layer in model.obj_inter_module:  # no dropout: both runs see the same graph
            layer.dropout.p = layer.dropout1.p = layer.dropout2.p = 0.0
            layer.self_attn.dropout = 0.0
        model = model.to("cuda")
        crit = losses.make_criterion(args)
        assert type(crit) is losses.PairwiseRankingLoss and crit.margin == 0.35
        crit.use_engine = use_engine
        seen = []
        crit.register_forward_hook(lambda mod, inp, out: seen.append(float(out.detach())))
        calls = (losses.PairwiseRankingLoss.engine_calls, losses.PairwiseRankingLoss.torch_calls)
        dl = torch.utils.data.DataLoader(Ds(), batch_size=B, collate_fn=collate_fn, shuffle=False)
        torch.manual_seed(0)
        mean, _ = train_epoch(model, dl, args, Adam(model, lr=1e-3), crit)
        after = (losses.PairwiseRankingLoss.engine_calls, losses.PairwiseRankingLoss.torch_calls)
        assert (after[0] - calls[0], after[1] - calls[1]) == ((2, 0) if use_engine else (0, 2))
        assert len(seen) == 2 and abs(mean - np.mean(seen)) < 1e-6 * abs(mean)
        return seen

    on, off = epoch(True), epoch(False)
    print("per-batch losses, engine:", on, "torch:", off)
    for x, y in zip(on, off):
        assert np.isfinite(x) and x > 0 and abs(x - y) <= 1e-5 * abs(y)


# ------------------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, b_local, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    im, s, _ = R.conditioned_inputs(world * b_local, 0.45, M)
    lo = rank * b_local
    out = {}
    for kind in R.KINDS:
        crit = _crit(kind, gather=True)
        x, y = dev(im[lo:lo + b_local]).requires_grad_(), dev(s[lo:lo + b_local]).requires_grad_()
        loss = crit(x, y)
        loss.backward()
        torch.cuda.synchronize()
        assert type(crit).engine_calls == 1 and type(crit).torch_calls == 0
        out[kind] = (float(loss.detach()), x.grad.cpu().numpy(), y.grad.cpu().numpy())
    out_q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_evaluate_the_global_batch(eng):
    """gloo, both ranks on GPU 0 (as tests/test_gpu_dp_train.py): 2 x 16 rows with ``gather=True`` — every rank's loss is the
    single-process loss of the 32 rows, its gradients the corresponding 16 rows."""
    import torch.multiprocessing as mp

    world, b_local, limit = 2, 16, 240
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, b_local, port, out_q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(out_q.get(timeout=limit) for _ in range(world))
        for p in procs:
            p.join(timeout=limit)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    im, s, _ = R.conditioned_inputs(world * b_local, 0.45, M)
    for kind in R.KINDS:
        rl, rgi, rgs = R.conditioned_reference(world * b_local, 0.45, M, kind)
        one, one_gi, one_gs = run(eng, im, s, kind, M)
        for rank in range(world):
            loss, g_im, g_s = res[rank][kind]
            rows = slice(rank * b_local, (rank + 1) * b_local)
            assert abs(loss - one) <= 1e-7 * abs(one)
            R.assert_loss(loss, rl, f"rank {rank}")
            bound_i, bound_s = R.RANK_T[kind] * R.rms(rgi) + 1e-9, R.RANK_T[kind] * R.rms(rgs) + 1e-9  # the bars of the 32-row tensors
            assert np.abs(g_im - rgi[rows]).max() <= bound_i and np.abs(g_s - rgs[rows]).max() <= bound_s
            assert np.array_equal(g_im, one_gi[rows]) and np.array_equal(g_s, one_gs[rows])  # the same kernel on the same rows
