"""Host plumbing between the nn.Modules (``CellRetrievalNetwork``, ``LanguageEncoder``, ``CrossMatch``, the losses) and the engine:
one copy of what each of them needs around an engine call. Plain functions over the caller's own attributes; no state here."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import packing
from .engine import Engine, T2LError


# ---- the engine of a device, and whether what it holds is still current ------------------------------------------------------------
def device_index(device, what: str) -> int:
    if device.type != "cuda":
        raise T2LError(f"{what} runs on the MI355X only (model.to('cuda')); there is no CPU fallback")
    return device.index if device.index is not None else torch.cuda.current_device()


def engine_for(current, device, what: str):
    """-> (engine on ``device``, is_new): ``current`` when it already sits there; after a new one the caller resets whatever it
    cached about the old one's contents (versions, bind keys)."""
    idx = device_index(device, what)
    if current is not None and current.device == idx:
        return current, False
    return Engine(idx), True


def tensors_version(tensors) -> tuple:
    """Changes when a tensor of the list was replaced or written in place (not when the engine wrote behind torch's back: the
    callers keep a generation counter for that)."""
    return tuple([(t.data_ptr(), t._version) for t in tensors])


def bind_key(tensors) -> tuple:
    """name -> (data, gradient buffer | None): changes when, and only when, a data or gradient pointer does."""
    return tuple((n, d.data_ptr(), None if g is None else g.data_ptr()) for n, (d, g) in tensors.items())


def rebind(eng, tensors, bound, bind):
    """``bind(tensors)`` unless ``bound`` is already their key; -> the key to remember. The same module on moved storage
    (model.to(), a re-assigned .grad) keeps the engine-side Adam moments; the first bind of an engine starts them."""
    key = bind_key(tensors)
    if key != bound:
        eng.set_option("train_keep_adam_state", 1 if bound is not None else 0)
        bind(tensors)
    return key


def adopt_grad(param, buf):
    """Make the persistent buffer ``buf`` (what the engine is bound to and ADDS into) ``param.grad``, with the value .grad has now."""
    if param.grad is None:
        param.grad = buf  # zero_grad(set_to_none=True) only dropped the reference
        buf.zero_()
    elif param.grad.data_ptr() != buf.data_ptr():
        buf.copy_(param.grad)  # a gradient assigned from outside keeps its VALUE; the storage stays the bound buffer's
        param.grad = buf


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def pack_objects(eng, objects, object_encoder, dev):
    """Packed cells on ``dev``. Raw points not reduced yet: one HBM pass on the GPU (t2l_reduce_objects) instead of three numpy
    reductions per object on the host (what the reference redoes on every call); reduced before: the cached values, packed on the host.
    ``objects`` from ``kitti360pose.coarse_batches`` (a list that carries ``cell_set``, ``object_rows`` and ``mirror``): the rows of the
    set's resident reductions in one launch (``PackedCellSet.gather_rows``); nothing is walked or uploaded but the row list."""
    oe = object_encoder
    cell_set, rows, mirror = (getattr(objects, n, None) for n in ("cell_set", "object_rows", "mirror"))
    if cell_set is not None and rows is not None and mirror is not None:
        counts = [len(r) for r in rows]
        flat = np.concatenate(rows) if counts else np.zeros(0, np.int32)
        return cell_set.gather_rows(eng, dev, flat, np.repeat(np.asarray(mirror, dtype=np.uint8), counts), counts, oe.known_classes,
                                    oe.known_colors)
    if any(getattr(o, "_t2l_feat", None) is None for objs in objects for o in objs):
        return packing.pack_cells_gpu(eng, objects, oe.known_classes, oe.known_colors, dev)
    return packing.to_device(packing.pack_cells(objects, oe.known_classes, oe.known_colors), dev)


def _point_field(p, name):
    return p[name] if isinstance(p, dict) else getattr(p, name, None)


def is_point_batch(p) -> bool:
    """A cell's point batch as the reference's dataloader builds it: a PyG ``Batch`` or anything with ``.pos`` / ``.x``
    [n*256,3], or a dict with those keys (anything else in ``object_points`` is a precomputed features2 array / tensor)."""
    return not isinstance(p, (torch.Tensor, np.ndarray)) and _point_field(p, "pos") is not None


def point_batch_tensors(object_points, use_color: bool, dev):
    """Per-cell point batches -> (pos f32[n,256,3], rgb f32[n,256,3], objects per cell) on ``dev``. Without ``use_color`` the
    colours are voided, as the reference's ObjectEncoder does (object_encoder.py:87-90); the caller's arrays are not touched."""
    if use_color:
        xs = [torch.as_tensor(_point_field(p, "x")) for p in object_points]
    else:  # ablation of the reference: void all colours (object_encoder.py:87-90)
        xs = [torch.zeros_like(torch.as_tensor(_point_field(p, "x"))) for p in object_points]
    pos = torch.cat([torch.as_tensor(_point_field(p, "pos")).reshape(-1, 256, 3) for p in object_points]).to(dev, torch.float32)
    rgb = torch.cat([x.reshape(-1, 256, 3) for x in xs]).to(dev, torch.float32)
    counts = [int(torch.as_tensor(_point_field(p, "pos")).shape[0]) // 256 for p in object_points]
    return pos.contiguous(), rgb.contiguous(), counts


def read_object_points(object_points, use_color: bool, dev, per_cell=None):
    """``object_points`` of the published feature mode (class_embed off): per cell EITHER precomputed PointNet++ features2 [n_i,256]
    (array / tensor) -> f32[n,256] on ``dev``, OR the cell's point batch -> ``point_batch_tensors``' (pos, rgb, counts) for the
    engine's backbone. ``per_cell``: the object count every cell must have (the fine stage's pad_size)."""
    if object_points is None or any(p is None for p in object_points):
        raise T2LError("class_embed is off: object_points must hold, per cell, PointNet++ features2 [n_i,256] or the cell's point "
                       "batch (.pos/.x [n_i*256,3])")
    kinds = {is_point_batch(p) for p in object_points}
    if len(kinds) > 1:
        raise T2LError("object_points mixes point batches and features2 tensors: pass one kind for every cell")
    if kinds == {True}:
        for p in object_points if per_cell is not None else ():
            shapes = [None if _point_field(p, n) is None else tuple(np.shape(_point_field(p, n))) for n in ("pos", "x")]
            if any(sh != (per_cell * 256, 3) for sh in shapes):
                raise T2LError(f"a point batch must hold {per_cell}*256 points per cell (.pos and .x [{per_cell * 256},3]), got {shapes}")
        return point_batch_tensors(object_points, use_color, dev)
    pn = torch.cat([p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p)) for p in object_points], dim=0).to(dev, torch.float32)
    if per_cell is not None and tuple(pn.shape) != (len(object_points) * per_cell, 256):
        raise T2LError(f"features2 must be [{per_cell},256] per cell, got {tuple(pn.shape)} in all")
    return pn.reshape(-1, 256)


# ---- around a training-mode forward ------------------------------------------------------------------------------------------------
def hook_leaf(current, dev):
    """The dummy leaf that makes autograd call an engine function's ``backward`` (no real input requires grad)."""
    if current is None or current.device != dev:
        return torch.zeros(1, device=dev, requires_grad=True)
    return current


def new_token(owner, attr: str):
    """Marks the forward whose activations the engine now holds (it keeps those of the LAST training-mode forward only)."""
    token = object()
    setattr(owner, attr, token)
    return token


def check_token(owner, attr: str, token, what: str):
    if getattr(owner, attr) is not token:
        raise T2LError(f"backward of a stale {what}: the engine keeps the activations of the LAST training-mode forward only "
                       "(the reference's loop does one forward per backward too)")


def bump_batches_tracked(named_modules, is_used, backbone_prefix=(), backbone_calls: int = 0):
    """``BatchNorm1d.train()``'s int64 side effect, which the engine does not see: +1 on every BatchNorm the step ran (``is_used(name)``),
    + ``backbone_calls`` on the PointNet++ backbone's, which the reference calls once per cell (object_encoder.py:92-95)."""
    for name, m in named_modules:
        if isinstance(m, nn.BatchNorm1d) and m.num_batches_tracked is not None and is_used(name):
            n = backbone_calls if name.startswith(backbone_prefix) else 1
            if n:
                m.num_batches_tracked += n
