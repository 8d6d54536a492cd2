"""The coarse stage's criteria with the reference's constructor/forward signatures: ContrastiveLoss (training/losses.py:255-283;
libt2l.so: t2l_contrastive_loss), PairwiseRankingLoss and HardestRankingLoss (:179-217, :286-355; t2l_ranking_loss), each one
fused HIP forward+backward call, and ``make_criterion(args)``, the selection of training/coarse.py:263-270."""
from __future__ import annotations

import torch

from .engine import Engine
from .plumbing import device_index

_engines = {}  # device index -> the losses' own engine context (one per device, shared by every criterion)


def _engine_for(device: torch.device) -> Engine:
    idx = device_index(device, "the loss")
    if idx not in _engines:
        _engines[idx] = Engine(idx)
    return _engines[idx]


class _ContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, temperature):
        eng = _engine_for(im.device)
        need = im.requires_grad or s.requires_grad
        loss, ga, gp = eng.contrastive_loss(im.detach().contiguous().float(), s.detach().contiguous().float(),
                                            temperature, need_grad=need)
        if need:
            ctx.save_for_backward(ga, gp)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        ga, gp = ctx.saved_tensors
        return grad_out * ga, grad_out * gp, None


class _GatherRowsFn(torch.autograd.Function):
    """all_gather of the ranks' [B,D] rows into [W*B,D] (rank-major), differentiable: the backward hands every rank the slice
    of the incoming gradient that belongs to ITS rows — no communication. With a loss every rank evaluates identically on the
    gathered rows, that slice is d(global loss)/d(local rows); parameter gradients then only need a SUM over the ranks
    (``optim.Adam(group=..., grad_reduce="sum")``)."""

    @staticmethod
    def forward(ctx, x, group):
        import torch.distributed as dist

        from .sharded import _all_gather

        world, rank = dist.get_world_size(group), dist.get_rank(group)
        ctx.lo, ctx.n = rank * x.shape[0], x.shape[0]
        out = x.new_empty((world * x.shape[0],) + tuple(x.shape[1:]))
        _all_gather(dist, out, x.detach().contiguous(), group)
        return out

    @staticmethod
    def backward(ctx, grad):
        return grad[ctx.lo:ctx.lo + ctx.n].contiguous(), None


def gather_rows_with_grad(x, group=None):
    """[B,D] per rank -> [W*B,D] on every rank, gradients flowing back to the local rows (every rank must hold B rows)."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return x
    return _GatherRowsFn.apply(x, group)


class ContrastiveLoss(torch.nn.Module):
    """Symmetric InfoNCE; ``forward(im, s)`` as in the reference (both inputs are re-normalised inside).

    Data-parallel training (not in the reference, which is single-process): with ``group`` (or
    ``gather=True`` for the default process group) every rank all-gathers the [B,256] text and cell embeddings of ALL ranks
    — two collectives of W*B*1 KiB — and evaluates the loss of the GLOBAL W*B batch (every cell of every rank is a negative
    for every text), exactly the value one process would compute on the concatenated batch; the backward returns
    d(global loss)/d(local rows). Sum the parameter gradients over the ranks (``optim.Adam(model, group=...)``) and the step
    equals the single-process step on the W*B batch, except that BatchNorm statistics stay per rank."""

    def __init__(self, temperature: float = 1.0, group=None, gather: bool = False):
        super().__init__()
        self.temperature = temperature
        self.group = group
        self.gather = bool(gather) or group is not None

    def forward(self, im, s):
        if self.gather:
            im, s = gather_rows_with_grad(im, self.group), gather_rows_with_grad(s, self.group)
        return _ContrastiveFn.apply(im, s, float(self.temperature))


def _cosine_scores(im, s):
    im = im / torch.norm(im, dim=1, keepdim=True)
    s = s / torch.norm(s, dim=1, keepdim=True)
    return im @ s.t()


class _RankingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, kind, margin, scale):
        eng = _engine_for(im.device)
        need = im.requires_grad or s.requires_grad
        loss, g_im, g_s = eng.ranking_loss(im.detach().contiguous(), s.detach().contiguous(), kind, margin, scale, need_grad=need)
        if need:
            ctx.save_for_backward(g_im, g_s)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_im, g_s = ctx.saved_tensors
        return grad_out * g_im, grad_out * g_s, None, None, None


class _RankingLoss(torch.nn.Module):
    """What the two in-batch hinge losses share: the optional all-gather of the global batch (as ``ContrastiveLoss``: the loss of the
    W*B rows, the backward returning the local rows' slice) and the choice of path. CUDA float32 ``[B,256]`` inputs with
    1 <= B <= ``ENGINE_MAX_BATCH`` go to the engine (``t2l_ranking_loss``: one launch up to 128 rows, six beyond); anything else —
    CPU tensors, other widths or dtypes, larger batches — runs ``torch_forward``, the plain torch formulation. ``use_engine = False``
    (class or instance) switches the engine off; ``engine_calls`` / ``torch_calls`` count, per class, which path ran."""

    use_engine = True
    ENGINE_MAX_BATCH = 1024  # T2L_MAX_LOSS_BATCH
    engine_calls = 0
    torch_calls = 0
    kind = None
    scale = 1.0

    def _setup(self, margin, group, gather):
        self.margin = margin
        self.group = group
        self.gather = bool(gather) or group is not None

    def _on_engine(self, im, s):
        return (self.use_engine and im.is_cuda and s.is_cuda and im.dtype == torch.float32 and s.dtype == torch.float32
                and im.dim() == 2 and im.shape == s.shape and im.shape[1] == 256 and 1 <= im.shape[0] <= self.ENGINE_MAX_BATCH)

    def forward(self, im, s):
        if self.gather:
            im, s = gather_rows_with_grad(im, self.group), gather_rows_with_grad(s, self.group)
        if self._on_engine(im, s):
            type(self).engine_calls += 1
            return _RankingFn.apply(im, s, self.kind, float(self.margin), float(self.scale))
        type(self).torch_calls += 1
        return self.torch_forward(im, s)


class PairwiseRankingLoss(_RankingLoss):
    """--ranking_loss pairwise (training/losses.py:178-216, the reference's args default): sum of all in-batch hinge
    violations in both directions, divided by the batch size. ``group`` / ``gather``: the loss of the global batch, as
    ``ContrastiveLoss``."""

    kind = "pairwise"
    engine_calls = 0
    torch_calls = 0

    def __init__(self, margin: float = 1.0, group=None, gather: bool = False):
        super().__init__()
        self._setup(margin, group, gather)

    def torch_forward(self, im, s):
        scores = _cosine_scores(im, s)
        diag = scores.diag()
        off = ~torch.eye(len(im), dtype=torch.bool, device=scores.device)
        cost_s = torch.clamp(self.margin - diag[:, None] + scores, min=0) * off   # vs the other cells of each text
        cost_im = torch.clamp(self.margin - diag[None, :] + scores, min=0) * off  # vs the other texts of each cell
        return (cost_s.sum() + cost_im.sum()) / len(im)


class HardestRankingLoss(_RankingLoss):
    """--ranking_loss hardest, the definition in force (the module's SECOND HardestRankingLoss, training/losses.py:286-355,
    shadows the first): the pairwise hinge costs, but only the largest violation of every row counts, times ``scale``. Both
    maxima run along dim=1, as the reference's do."""

    kind = "hardest"
    engine_calls = 0
    torch_calls = 0

    def __init__(self, margin: float = 1.0, scale: float = 64.0, group=None, gather: bool = False):
        super().__init__()
        self._setup(margin, group, gather)
        self.scale = scale

    def torch_forward(self, images, captions):
        scores = _cosine_scores(images, captions)
        diag = scores.diag()
        off = ~torch.eye(len(images), dtype=torch.bool, device=scores.device)
        cost_s = torch.clamp(self.margin - diag[None, :] + scores, min=0) * off   # [i][j]: text j's own cell vs cell i
        cost_im = torch.clamp(self.margin - diag[:, None] + scores, min=0) * off  # [i][j]: cell i's own text vs text j
        return (cost_im.max(dim=1)[0].mean() + cost_s.max(dim=1)[0].mean()) * self.scale


def make_criterion(args, group=None, gather: bool = False):
    """The criterion ``args.ranking_loss`` selects, as training/coarse.py:263-270 builds it (``group`` / ``gather``: its global-batch
    form). ``triplet`` raises, as ``coarse.train_epoch`` does: the reference's own triplet branch cannot run."""
    name = args.ranking_loss
    if name == "pairwise":
        return PairwiseRankingLoss(margin=args.margin, group=group, gather=gather)
    if name == "hardest":
        return HardestRankingLoss(margin=args.margin, group=group, gather=gather)
    if name == "contrastive":
        return ContrastiveLoss(temperature=args.temperature, group=group, gather=gather)
    if name == "triplet":
        raise NotImplementedError("ranking_loss='triplet' is not runnable in the reference either (training/coarse.py:47-50)")
    raise ValueError(f"unknown ranking_loss {name!r} (pairwise, hardest, contrastive)")
