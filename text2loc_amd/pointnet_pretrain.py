"""Pretraining the PointNet++ object backbone as an object classifier: what produces the reference's ``--pointnet_path`` file
(models/object_encoder.py:50 loads it unconditionally; its published name records a classification accuracy).

The snapshot of the reference has no script for this step, so it is defined by what the snapshot does fix: ``PointNet2``'s two
``Linear(256, .)`` heads over ``features2`` (models/pointcloud/pointnet2.py:64-65, 91-92), the key layout of its ``state_dict``,
the transforms its training scripts hand the backbone (training/coarse.py:182-193) and the plain softmax cross-entropy. Like the
rest of PointNet++ here, it is self-consistent only.

``PointNet2`` runs on the engine in both modes: t2l_pointnet_cls_forward / _heads / _backward under ``model.train()``,
t2l_pointnet_features + the forward-only heads call under ``model.eval()``. There is no CPU path for the model; ``ClassifierLoss``
on CPU tensors is ``F.cross_entropy`` per head.
"""
from __future__ import annotations

import os.path as osp
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .cell_retrieval import PointNet2Params
from .engine import Engine, T2LError
from .kitti360pose import _checked_batch_size, draw_salts, load_pickle
from .packing import POINT_TRANSFORMS, PackedCellSet
from .plumbing import _point_field, bump_batches_tracked, check_token, engine_for, hook_leaf, new_token, rebind, tensors_version
from .tables import COLORS, KNOWN_CLASS

PREFIX = "object_encoder.pointnet."  # the keys the engine knows the backbone by (as it sits in CellRetrievalNetwork / CrossMatch)
_HEADS = ("class_classifier.", "color_classifier.")


# ---- the model ---------------------------------------------------------------------------------------------------------------------
class PointNet2Output:
    """What ``PointNet2.forward`` returns (the reference's EasyDict, pointnet2.py:94-100, without features0 / features1, which stay in
    the engine): ``features2`` [n,256], and ``class_pred`` [n,C1] / ``color_pred`` [n,C2], computed by the heads kernel on first use
    (the training loop never reads them: ``ClassifierLoss`` takes the loss and the counts from the same kernel). Under
    ``model.train()`` the logits are detached: gradients flow through ``ClassifierLoss`` only."""

    def __init__(self, model, features2):
        self.model, self.features2, self._logits = model, features2, None

    def _pred(self):
        if self._logits is None:
            n = int(self.features2.shape[0])
            zeros = np.zeros(n, np.int32)  # (the kernel wants labels; the logits do not depend on them)
            self._logits = self.model._engine.pointnet_cls_heads(self.features2.detach(), zeros, zeros, need_grad=False)[0]
        return self._logits

    @property
    def class_pred(self):
        return self._pred()[:, :self.model.class_classifier.out_features]

    @property
    def color_pred(self):
        return self._pred()[:, self.model.class_classifier.out_features:]


def _sync_grads(live):
    """The engine ADDS into the bound buffers: give them the value ``.grad`` has now (``plumbing.adopt_grad``, first half)."""
    for t, g in live:
        if t.grad is None:
            g.zero_()
        elif t.grad.data_ptr() != g.data_ptr():
            g.copy_(t.grad)


def _hand_out(live):
    for t, g in live:
        t.grad = g


class _BackboneFn(torch.autograd.Function):
    """Training-mode backbone up to features2 (t2l_pointnet_cls_forward / _backward). Parameter gradients do not flow through
    autograd: the engine adds them into the bound ``.grad`` buffers (``hook`` is a dummy leaf that makes autograd call ``backward``)."""

    @staticmethod
    def forward(ctx, hook, model, pos, rgb):
        out = model._engine.pointnet_cls_forward(pos, rgb)
        ctx.model = model
        ctx.token = new_token(model, "_cls_token")
        ctx.live = list(model._cls_live[0])
        return out

    @staticmethod
    def backward(ctx, grad_f2):
        model = ctx.model
        check_token(model, "_cls_token", ctx.token, "PointNet2 training forward")
        if ctx.live:  # (a frozen backbone has no backward: the heads' gradients were written by the loss)
            _sync_grads(ctx.live)
            model._engine.pointnet_cls_backward(grad_f2.contiguous().float())
            _hand_out(ctx.live)
        return None, None, None, None


class _HeadsLossFn(torch.autograd.Function):
    """``w_class CE(class) + w_color CE(color)`` over features2 (t2l_pointnet_cls_heads): the forward is the forward-only form, the
    backward the full one, scaled by the incoming gradient — read back once, the step's one readback."""

    @staticmethod
    def forward(ctx, features2, model, class_labels, color_labels, w_class, w_color):
        f2 = features2.detach().contiguous()
        _, loss2, correct, _ = model._engine.pointnet_cls_heads(f2, class_labels, color_labels, need_grad=False, need_logits=False)
        ctx.model, ctx.f2, ctx.labels, ctx.w = model, f2, (class_labels, color_labels), (w_class, w_color)
        ctx.live = list(model._cls_live[1])
        ctx.mark_non_differentiable(loss2, correct)
        return w_class * loss2[0] + w_color * loss2[1], loss2, correct

    @staticmethod
    def backward(ctx, grad_out, _g2, _g3):
        g = float(grad_out)
        _sync_grads(ctx.live)
        grad = ctx.model._engine.pointnet_cls_heads(ctx.f2, ctx.labels[0], ctx.labels[1], ctx.w[0] * g, ctx.w[1] * g, need_grad=True,
                                                    need_logits=False)[3]
        _hand_out(ctx.live)
        return grad, None, None, None, None, None


class PointNet2(PointNet2Params):
    """The reference's ``PointNet2(num_classes, num_colors, args)`` (pointnet2.py:52-100) on the engine. ``state_dict()`` has the
    reference's keys and shapes, so ``torch.save(model.state_dict(), path)`` is a ``pointnet_path`` file and loads into
    ``CellRetrievalNetwork(...).object_encoder.pointnet`` and ``CrossMatch(...).object_encoder.pointnet``.

    ``forward(batch)``: one batch of objects as the reference's dataloader builds it — ``.pos`` / ``.x`` [n*256,3] (or [n,256,3]),
    or a dict with those keys. The whole batch is ONE BatchNorm segment, as a single PyG batch is. Under ``model.train()`` with
    gradients enabled the gradients land in the live ``.grad`` tensors (``torch.optim.Adam`` steps them); one forward per backward."""

    def __init__(self, num_classes: int, num_colors: int, args=None):
        super().__init__(num_classes, num_colors)
        if args is not None:  # pointnet2.py:55
            assert getattr(args, "pointnet_layers", 3) == 3 and getattr(args, "pointnet_variation", 0) == 0
        self.args = args
        self._engine: Optional[Engine] = None
        self._weights_version = None
        self._generation = 0   # bumped whenever the engine changes buffers (running statistics) behind torch's back
        self._cls_bound = None
        self._cls_grads = {}
        self._cls_live = ([], [])  # (backbone, heads): (parameter, its bound gradient buffer) of the last bind
        self._cls_token = None
        self._cls_hook = None

    @property
    def device(self):
        return self.lin2.weight.device

    def _device_engine(self) -> Engine:
        eng, is_new = engine_for(self._engine, self.device, "PointNet2")
        if is_new:
            self._engine, self._weights_version, self._cls_bound = eng, None, None
        return eng

    def _cls_tensors(self):
        """engine key -> (live tensor, persistent gradient buffer | None): the backbone with buffers exactly when it trains
        (``requires_grad``), the heads always, the BatchNorm running statistics without."""
        out, backbone, heads = {}, [], []
        for n, t in self.named_parameters():
            if not t.requires_grad:
                out[PREFIX + n] = (t.data, None)
                continue
            g = self._cls_grads.get(n)
            if g is None or g.shape != t.shape or g.device != t.device:
                g = self._cls_grads[n] = torch.zeros_like(t.data)
            (heads if n.startswith(_HEADS) else backbone).append((t, g))
            out[PREFIX + n] = (t.data, g)
        for n, b in self.named_buffers():
            if n.endswith(("running_mean", "running_var")):
                out[PREFIX + n] = (b, None)
        self._cls_live = (backbone, heads)
        return out

    def _bound_engine(self) -> Engine:
        eng = self._device_engine()
        self._cls_bound = rebind(eng, self._cls_tensors(), self._cls_bound, eng.pointnet_cls_bind)
        return eng

    def _read(self, batch):
        pos, x = _point_field(batch, "pos"), _point_field(batch, "x")
        if isinstance(batch, (torch.Tensor, np.ndarray)) or pos is None or x is None:
            raise T2LError("PointNet2: the batch must carry .pos and .x [n*256,3] (a PyG Batch, or a dict with those keys)")
        if self.device.type != "cuda":
            raise T2LError("PointNet2 runs on the MI355X only (model.to('cuda')); there is no CPU fallback")
        pos = torch.as_tensor(pos).reshape(-1, 256, 3).to(self.device, torch.float32).contiguous()
        x = torch.as_tensor(x).reshape(-1, 256, 3).to(self.device, torch.float32).contiguous()
        if pos.shape != x.shape or pos.shape[0] == 0:
            raise T2LError(f"PointNet2: .pos and .x must hold the same n >= 1 objects of 256 points, got {tuple(pos.shape)}, {tuple(x.shape)}")
        return pos, x

    def forward(self, batch) -> PointNet2Output:
        pos, rgb = self._read(batch)
        eng = self._bound_engine()  # (the heads call reads the live head tensors in both modes)
        if self.training and torch.is_grad_enabled():
            self._cls_hook = hook_leaf(self._cls_hook, self.device)
            f2 = _BackboneFn.apply(self._cls_hook, self, pos, rgb)
            bump_batches_tracked(self.named_modules(), lambda name: True)
            self._generation += 1  # running statistics moved: the eval path must re-load its weights
            return PointNet2Output(self, f2)
        if self.training:
            raise T2LError("PointNet2 under model.train() needs gradients enabled (the training-mode forward keeps its activations for "
                           "one backward); call model.eval() for inference")
        with torch.no_grad():
            version = (tensors_version(list(self.state_dict(keep_vars=True).values())), self._generation)
            if version != self._weights_version:
                eng.pointnet_load_weights({PREFIX + k: v for k, v in self.state_dict().items()})
                self._weights_version = version
            n = int(pos.shape[0])
            return PointNet2Output(self, eng.pointnet_features(pos, rgb, np.array([0, n], dtype=np.int32)))


class ClassifierLoss:
    """``w_class * CE(class_pred, class_labels) + w_color * CE(color_pred, color_labels)``, mean over the batch, no ignore index, no
    class weights. On a ``PointNet2Output`` the heads, the loss and its backward are one engine kernel (labels are HOST int arrays);
    on anything with CPU ``class_pred`` / ``color_pred`` tensors it is ``F.cross_entropy`` per head. ``last`` holds the last call's
    ``loss2`` (per head, f32[2]) and ``correct`` (first arg-max == label, i32[2] / i64[2]) on the device of the inputs."""

    def __init__(self, w_class: float = 1.0, w_color: float = 1.0):
        self.w_class, self.w_color = float(w_class), float(w_color)
        self.last = None

    def __call__(self, out, class_labels, color_labels):
        if isinstance(out, PointNet2Output):
            lc = np.ascontiguousarray(class_labels.cpu().numpy() if isinstance(class_labels, torch.Tensor) else class_labels, dtype=np.int32)
            lk = np.ascontiguousarray(color_labels.cpu().numpy() if isinstance(color_labels, torch.Tensor) else color_labels, dtype=np.int32)
            if out.features2.requires_grad:
                loss, loss2, correct = _HeadsLossFn.apply(out.features2, out.model, lc, lk, self.w_class, self.w_color)
            else:
                _, loss2, correct, _ = out.model._engine.pointnet_cls_heads(out.features2, lc, lk, need_grad=False, need_logits=False)
                loss = self.w_class * loss2[0] + self.w_color * loss2[1]
            self.last = SimpleNamespace(loss2=loss2, correct=correct)
            return loss
        cp, kp = out.class_pred, out.color_pred
        if cp.is_cuda:
            raise T2LError("ClassifierLoss on the GPU takes PointNet2's own output (the heads run in the engine); there is no eager path")
        lc, lk = torch.as_tensor(np.asarray(class_labels), dtype=torch.long), torch.as_tensor(np.asarray(color_labels), dtype=torch.long)
        l1, l2 = F.cross_entropy(cp, lc), F.cross_entropy(kp, lk)
        self.last = SimpleNamespace(loss2=torch.stack([l1, l2]).detach(),
                                    correct=torch.stack([(cp.argmax(1) == lc).sum(), (kp.argmax(1) == lk).sum()]))
        return self.w_class * l1 + self.w_color * l2


# ---- the dataset -------------------------------------------------------------------------------------------------------------------
def nearest_color(rgb_mean) -> np.ndarray:
    """Index of the nearest of the 8 centres of ``tables.COLORS`` (Euclidean, lowest index on ties) per row of ``rgb_mean`` [n,3]."""
    d = np.linalg.norm(np.asarray(rgb_mean, dtype=np.float64)[:, None, :] - COLORS[None], axis=2)
    return np.argmin(d, axis=1).astype(np.int32)


class Kitti360ObjectDataset:
    """One item per distinct (scene, object id) of the scenes' cells; the first occurrence in cell order wins (a cell holds its
    clipped view of an object). Objects whose label is not in ``KNOWN_CLASS`` and objects with fewer than ``min_points`` points are
    dropped (25: the reference's own floor for an object). Class label: the index in ``KNOWN_CLASS``; colour label:
    the nearest of the 8 ``COLORS`` centres to the object's mean colour. The raw points stay resident through ``cell_set``
    (``PackedCellSet``: one pseudo-cell per scene), item i = object row i."""

    def __init__(self, base_path: str, scene_names: Sequence[str], min_points: int = 25):
        self._build([(scene, load_pickle(osp.join(base_path, "cells", f"{scene}.pkl"))) for scene in scene_names], min_points)

    @classmethod
    def from_cells(cls, scene_cells, min_points: int = 25):
        """The same dataset over cells already in memory: ``scene_cells`` = [(scene name, its cells in order), ...]."""
        self = cls.__new__(cls)
        self._build(list(scene_cells), min_points)
        return self

    def _build(self, scene_cells, min_points):
        self.keys, self.dropped_label, self.dropped_small = [], 0, 0
        groups, seen = [], set()
        for scene, cells in scene_cells:
            kept = []
            for cell in cells:
                for o in cell.objects:
                    if (scene, o.id) in seen:
                        continue
                    seen.add((scene, o.id))
                    if o.label not in KNOWN_CLASS:
                        self.dropped_label += 1
                    elif len(o.xyz) < int(min_points):
                        self.dropped_small += 1
                    else:
                        kept.append(o)
                        self.keys.append((scene, o.id))
            groups.append(SimpleNamespace(id=scene, objects=kept))
        self.cell_set = PackedCellSet(groups)
        self.class_labels = np.array([KNOWN_CLASS.index(lb) for lb in self.cell_set.labels], dtype=np.int32)
        self._color_labels = None
        self._sampler_engine = None

    def __len__(self):
        return len(self.keys)

    def color_labels_host(self) -> np.ndarray:
        """The colour labels by numpy on the host (float64 means of the float32 colours)."""
        cs = self.cell_set
        po = cs.point_offsets
        means = np.array([cs.rgb[po[i]:po[i + 1]].mean(axis=0, dtype=np.float64) for i in range(len(self))]).reshape(-1, 3)
        return nearest_color(means)

    def color_labels(self, engine: Engine, device) -> np.ndarray:
        """The colour labels as HOST i32[n], from ONE t2l_reduce_objects over the resident set (identity ``color_rows``), cached."""
        if self._color_labels is None:
            d = self.cell_set.on_device(device)
            red = engine.reduce_objects(d["xyz"], d["rgb"], self.cell_set.point_offsets, COLORS, np.arange(len(COLORS), dtype=np.int32))
            self._color_labels = red["color_idx"].cpu().numpy().astype(np.int32)
        return self._color_labels


def epoch_permutation(n: int, seed: int, epoch: int) -> np.ndarray:
    """The order of an epoch's items: a function of (seed, epoch) only."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(int(n))


def object_batches(dataset: Kitti360ObjectDataset, batch_size: int, seed: int = 0, transform: str = "rotate_normalize", device="cuda",
                   epoch: int = 0, shuffle: bool = True, drop_last: bool = False, engine: Optional[Engine] = None):
    """One epoch of ``(pos f32[B,256,3], rgb f32[B,256,3], class_labels i32[B], color_labels i32[B])``: the points on ``device``,
    the labels HOST arrays. The order is ``epoch_permutation(len(dataset), seed, epoch)`` (drawn on the host); a batch's rows are
    sampled from the resident set in ONE launch of t2l_sample_object_points_indexed — item i under ``seed ^ draw_salts(epoch, i, 1)[0]``
    — with ``transform`` (``packing.POINT_TRANSFORMS``; the default is what the reference's training scripts give the backbone,
    training/coarse.py:182-193: FixedPoints + RandomRotate(120, axis=2) + NormalizeScale; ``packing.point_transform_from_args``
    names the others). GPU work belongs to the process that owns the engine: inside a DataLoader worker this raises."""
    batch_size = _checked_batch_size("object_batches", batch_size)
    if transform not in POINT_TRANSFORMS:
        raise T2LError(f"object_batches: transform must be one of {sorted(POINT_TRANSFORMS)}, got {transform!r}")
    if engine is None:
        engine, _ = engine_for(dataset._sampler_engine, torch.device(device), "object_batches")
        dataset._sampler_engine = engine
    order = epoch_permutation(len(dataset), seed, epoch) if shuffle else np.arange(len(dataset))
    d = dataset.cell_set.on_device(device)
    color = dataset.color_labels(engine, device)
    for lo in range(0, len(order), batch_size):
        chunk = order[lo:lo + batch_size]
        if drop_last and len(chunk) < batch_size:
            return
        rows = chunk.astype(np.int32)
        salts = np.array([draw_salts(epoch, int(i), 1)[0] for i in chunk], dtype=np.uint32)
        pos, rgb = engine.sample_object_points_indexed(d["xyz"], d["rgb"], d["point_offsets"], rows, salts, seed=int(seed),
                                                       transform=transform)
        yield pos, rgb, dataset.class_labels[chunk], color[chunk]


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def _epoch(model, batches, criterion, optimizer):
    tot, ok, n_all = None, None, 0
    for pos, rgb, class_labels, color_labels in batches:
        if optimizer is not None:
            optimizer.zero_grad()
        loss = criterion(model({"pos": pos, "x": rgb}), class_labels, color_labels)
        if optimizer is not None:
            loss.backward()
            optimizer.step()
        n = int(len(class_labels))
        part = torch.cat([loss.detach().reshape(1), criterion.last.loss2.reshape(2)]).double() * n
        cnt = criterion.last.correct.reshape(2).double()
        tot, ok, n_all = (part, cnt, n) if tot is None else (tot + part, ok + cnt, n_all + n)
    if tot is None:
        raise ValueError("no batches")
    v = (torch.cat([tot, ok]) / n_all).cpu().tolist()  # the epoch's one readback of the metrics
    return dict(loss=v[0], loss_class=v[1], loss_color=v[2], acc_class=v[3], acc_color=v[4])


def train_epoch(model, batches, optimizer, criterion) -> dict:
    """zero_grad, forward, loss, backward, ``optimizer.step()`` per batch of ``object_batches``; -> the epoch's sample-weighted
    ``{loss, loss_class, loss_color, acc_class, acc_color}``. The metrics stay on the device until the epoch ends."""
    model.train()
    return _epoch(model, batches, criterion, optimizer)


@torch.no_grad()
def eval_epoch(model, batches, criterion) -> dict:
    """The same metrics under ``model.eval()`` (t2l_pointnet_features + the forward-only heads call)."""
    model.eval()
    return _epoch(model, batches, criterion, None)
