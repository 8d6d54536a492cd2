"""Drop-in for the reference's fine stage: ``models.cross_matcher.CrossMatch`` (models/cross_matcher.py:39-141) and
``evaluation.pipeline.run_fine`` (evaluation/pipeline.py:88-204).

    CrossMatch(known_classes, known_colors, args)
        .forward(objects, hints, object_points) -> Tensor[B,2]   offsets = pose estimate inside each cell, in [0,1]^2
        .state_dict() / .load_state_dict()    same key names as the reference's fine checkpoint
        .encode_cells(objects, object_points) -> Tensor[B,16,128]   (new: the query-independent half, cacheable per cell)
        .match(cell_desc, hint_desc, cell_index, hint_index) -> Tensor[P,2]

Of the text branch (``LanguageEncoder(is_fine=True)``: T5 + one Transformer layer over tokens + Linear/BN) only T5 stays on
PyTorch-ROCm: the head behind it runs in the engine, in eval mode (t2l_text_head) and under ``model.train()``
(t2l_text_head_train / _backward in their fine layout, out [B, n_hints, 128]; ``LanguageEncoder.head`` keeps the PyTorch modules
for what the engine does not take: site-specific dropout probabilities, a trainable T5, ``use_engine_train_head = False``). The
3D-submap branch (ObjectEncoder at fine_embed_dim incl. PointNet++ in the published mode), the cascaded cross-attention decoder
layers and the offset head run in the engine (t2l_fine_*). The nn.Modules below are PARAMETER CONTAINERS for the engine-side
tensors.

Under ``model.train()``, ``forward`` is one training step's forward in the engine (t2l_fine_train_*): BatchNorm over the
batch's objects, the decoder layers' dropout, and a backward that adds every parameter gradient straight into the live
``.grad`` tensors and hands d loss / d hint encodings (and d features2) back to autograd, so ``loss.backward()`` continues into
the text branch — the engine's text-head backward, which adds the head's gradients into its ``.grad`` tensors the same way — and
``torch.optim.Adam(model.parameters())`` steps everything (training/fine.py:38-91) — or ``text2loc_amd.optim.Adam(model)``, which
zeroes and steps the engine-side parameters with one launch each (t2l_fine_zero_grad / t2l_fine_adam_step, the moments inside the
library), the hint encoder's head through t2l_text_adam_step, and leaves only what remains to a torch optimizer. ``encode_cells`` /
``match`` stay eval-only.

With class_embed off (the published fine command) ``object_points`` holds per cell EITHER features2 [16,256] as tensors OR the
cell's point batch (``.pos`` / ``.x`` [16*256,3], or a dict with those keys, as ``CellRetrievalNetwork`` takes them). Point
batches run the PointNet++ backbone in the engine in training mode, one call per cell as in the reference (per-cell BatchNorm
statistics; its running statistics move once per cell and ``num_batches_tracked`` by B), and the backward continues into it:
trained jointly unless ``--pointnet_freeze``, in which case only its forward runs. Backbone parameters get their ``.grad`` only
from a backward that went through the backbone; a step fed features2 tensors leaves them at None, so optimizers skip them.
Parity of the backbone with torch_geometric stays unpinned (self-consistent with the build's own restatement only), as for
the coarse stage's backbone.
"""
from __future__ import annotations

from copy import copy
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import packing
from .cell_retrieval import LanguageEncoder, ObjectEncoderParams, _apply_sync_bn
from .engine import Engine, T2LError
from .plumbing import (adopt_grad, bump_batches_tracked, check_token, engine_for, hook_leaf, new_token, pack_objects, read_object_points,
                       rebind, tensors_version)

FINE_DIM, PAD_SIZE = 128, 16
BACKBONE = "object_encoder.pointnet."
_HEADS = (BACKBONE + "class_classifier.", BACKBONE + "color_classifier.")  # PointNet2's classifiers: not on the features2 path


def get_mlp_offset(dims: List[int]) -> nn.Sequential:
    """Linear/ReLU stack without trailing activation; key layout ``{0,2,...}`` (models/cross_matcher.py:17-36)."""
    mods: list = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


class PadObject:
    """``Object3d.create_padding()`` (datapreparation/kitti360pose/imports.py:75-83): label 'pad', 8 points within 1 mm of
    the origin, black. The reference draws the 8 points with the global numpy RNG on every call; here they are fixed."""

    label = "pad"
    _xyz = np.random.default_rng(0xBAD).random((8, 3)) * 0.001
    _rgb = np.zeros((8, 3), dtype=np.float32)

    def __init__(self):
        self.xyz, self.rgb = PadObject._xyz, PadObject._rgb


def pad_objects(objects: list, pad_size: int = PAD_SIZE) -> list:
    """Cut to / pad to ``pad_size`` objects (dataloading/kitti360pose/eval.py:147-156)."""
    objs = list(objects)[:pad_size]
    while len(objs) < pad_size:
        objs.append(PadObject())
    return objs


def create_hint_description(pose) -> List[str]:
    """dataloading/kitti360pose/base.py:60-68."""
    return [f"The pose is {d.direction} of a {d.object_color_text} {d.object_label}." for d in pose.descriptions]


class CrossMatch(nn.Module):
    def __init__(self, known_classes: List[str], known_colors: List[str], args, language_encoder: Optional[nn.Module] = None):
        super().__init__()
        self.args = args
        self.embed_dim = args.fine_embed_dim
        if self.embed_dim != FINE_DIM:
            raise T2LError(f"the engine's fine stage is built for fine_embed_dim={FINE_DIM}, got {self.embed_dim}")
        if getattr(args, "pad_size", PAD_SIZE) != PAD_SIZE:
            raise T2LError(f"the engine's fine stage is built for pad_size={PAD_SIZE}")
        n_layers = int(args.fine_num_decoder_layers)
        if not 0 <= n_layers <= 4:
            raise T2LError(f"the engine's fine stage holds 0..4 decoder layers, got fine_num_decoder_layers={n_layers}")
        self.object_encoder = ObjectEncoderParams(FINE_DIM, known_classes, args, known_colors)
        self.language_encoder = language_encoder if language_encoder is not None else LanguageEncoder(
            FINE_DIM, hungging_model=args.hungging_model, fixed_embedding=args.fixed_embedding,
            intra_module_num_layers=args.fine_intra_module_num_layers, intra_module_num_heads=args.fine_intra_module_num_heads,
            is_fine=True)
        self.mlp_offsets = get_mlp_offset([FINE_DIM, FINE_DIM // 2, 2])
        mk = lambda: nn.TransformerDecoderLayer(d_model=FINE_DIM, nhead=args.fine_num_decoder_heads, dim_feedforward=4 * FINE_DIM)
        if n_layers > 0:
            self.cross_hints = nn.ModuleList([mk() for _ in range(n_layers)])
            self.cross_objects = nn.ModuleList([mk() for _ in range(n_layers)])
        else:  # cross_matcher.py:75-79: ONE layer (state_dict keys "cross_hints.*", no index), the hints attend the raw objects once
            self.cross_hints = mk()
            self.cross_objects = None
        self._engine: Optional[Engine] = None
        self._weights_version = None
        self._train_generation = 0  # bumped by every training-mode forward (running statistics move outside torch's _version)
        self._fine_train_bound = None
        self._fine_train_grads = {}  # name -> persistent gradient buffer (kept when .grad is set to None): views of _fine_train_flat
        self._fine_train_flat = None
        self._fine_train_flat_layout = None
        self._sync_bn_cfg = None
        self._fine_train_token = None
        self._fine_train_hook = None
        self._fine_train_pn_live = []  # (backbone parameter, its bound gradient buffer) of the last bind that trains the backbone

    @property
    def device(self):
        return next(self.mlp_offsets.parameters()).device

    def get_device(self):
        return self.device

    # ---- engine plumbing ----------------------------------------------------------------------------------
    def _device_engine(self) -> Engine:
        eng, is_new = engine_for(self._engine, self.device, "the fine stage")
        if is_new:
            self._engine, self._weights_version, self._fine_train_bound = eng, None, None
        return eng

    def engine(self) -> Engine:
        self._device_engine()
        params = [p for n, p in self.state_dict(keep_vars=True).items() if not n.startswith("language_encoder.")]
        version = (tensors_version(params), self._train_generation)
        if version != self._weights_version:
            a = self.args
            sd = {k: v for k, v in self.state_dict().items() if not k.startswith("language_encoder.")}
            self._engine.fine_load_weights(sd, class_embed=bool(getattr(a, "class_embed", False)),
                                           color_embed=bool(getattr(a, "color_embed", False)), use_features=tuple(a.use_features),
                                           num_layers=a.fine_num_decoder_layers, num_heads=a.fine_num_decoder_heads)
            self._weights_version = version
        return self._engine

    def _read_points(self, objects, object_points):
        """``read_object_points`` for exactly the cells of ``objects`` (the engine takes the cell count from ``objects`` and reads
        ``pad_size`` rows per cell): -> features2 f32[B*16,256], or the point batches' (pos, rgb, counts)."""
        got = read_object_points(object_points, "color" in self.args.use_features, self.device, PAD_SIZE)
        rows = int((got[0] if isinstance(got, tuple) else got).shape[0])
        if rows != len(objects) * PAD_SIZE:
            raise T2LError(f"object_points must describe exactly the objects of each cell: {len(objects)} cells of {PAD_SIZE}, "
                           f"got {rows} objects in all")
        return got

    # ---- the two halves -----------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_cells(self, objects, object_points=None) -> torch.Tensor:
        """[B,16,128] unit-row object descriptors of B padded cells (cross_matcher.py:97-104)."""
        if self.training:
            raise T2LError("the fine stage is eval-only here (call model.eval()); its training step is not built")
        if any(len(o) != PAD_SIZE for o in objects):
            raise T2LError(f"every cell must hold exactly pad_size={PAD_SIZE} objects (cross_matcher.pad_objects pads / cuts)")
        eng, a = self.engine(), self.args
        packed = pack_objects(eng, objects, self.object_encoder, self.device)
        if "class" in a.use_features and not bool(getattr(a, "class_embed", False)):
            pn = self._read_points(objects, object_points)
            if isinstance(pn, tuple):  # point batches: the backbone in the engine
                pn = eng.pointnet_features(pn[0], pn[1], np.arange(0, len(objects) * PAD_SIZE + 1, PAD_SIZE, dtype=np.int32))
            packed["pn_feat"] = pn.contiguous()
        return eng.fine_encode_objects(packed)

    @torch.no_grad()
    def match(self, cell_desc: torch.Tensor, hint_desc: torch.Tensor, cell_index=None, hint_index=None) -> torch.Tensor:
        ci = None if cell_index is None else torch.as_tensor(cell_index, dtype=torch.int32, device=cell_desc.device).contiguous()
        hi = None if hint_index is None else torch.as_tensor(hint_index, dtype=torch.int32, device=cell_desc.device).contiguous()
        return self.engine().fine_match(cell_desc.contiguous(), hint_desc.detach().float().contiguous(), ci, hi)

    def forward(self, objects, hints, object_points=None) -> torch.Tensor:
        """One (pose, cell) pair per batch entry, as ``run_fine`` calls it (evaluation/pipeline.py:113-116) and as the
        reference's fine train_epoch batches them (training/fine.py:51-55)."""
        if self.training:
            return self._forward_train(objects, hints, object_points)
        with torch.no_grad():
            hint_enc = self.language_encoder(hints)  # [B, n_hints, 128]  (cross_matcher.py:95)
            return self.match(self.encode_cells(objects, object_points), hint_enc)

    # ---- training mode ------------------------------------------------------------------------------------
    def _fine_train_modules(self):
        """(prefixes of the modules the engine step runs, prefixes of those whose parameters receive a gradient) — the
        ObjectEncoder branches of args.use_features (object_encoder.py:102-149), plus mlp_pointnet and the PointNet++ backbone
        whenever class_embed is off: the reference runs them then even without "class" (object_encoder.py:86-99), which moves
        their BatchNorm statistics only. (The backbone runs only on point batches; its classifier heads never do.)"""
        a = self.args
        ce, co = bool(getattr(a, "class_embed", False)), bool(getattr(a, "color_embed", False))
        oe = "object_encoder."
        grad = ["cross_hints.", "cross_objects.", "mlp_offsets."]
        if "class" in a.use_features:
            grad.append(oe + ("class_embedding." if ce else "mlp_pointnet."))
            if not ce:
                grad.append(BACKBONE)
        if "color" in a.use_features:
            grad.append(oe + ("color_embedding." if co else "color_encoder."))
        if "position" in a.use_features:
            grad.append(oe + "pos_encoder.")
        if "num" in a.use_features:
            grad.append(oe + "num_encoder.")
        if len(a.use_features) > 1:
            grad.append(oe + "mlp_merge.")
        run = grad + ([oe + "mlp_pointnet.", BACKBONE] if not ce else [])
        return tuple(run), tuple(grad)

    def _fine_train_tensors(self):
        """state_dict key -> (live tensor, persistent .grad buffer or None) for everything the engine step reads. Only the
        parameters the step differentiates get a .grad (the others stay None, as in the reference, and optimizers skip them).
        The backbone's buffers are handed out as .grad by the backward that goes through the backbone (_FineTrainFn), not here."""
        run, with_grad = self._fine_train_modules()
        out = {}
        self._fine_train_pn_live = []
        live = [(n, t) for n, t in self.named_parameters() if n.startswith(run) and not n.startswith(_HEADS)]
        # The gradient buffers are views into ONE flat tensor (64-float aligned), as CellRetrievalNetwork._train_tensors makes them:
        # data-parallel training all-reduces it as a single collective (optim.Adam(group=...)), and zero_grad(set_to_none=True) /
        # model.to() only drop or move references, never the buffers the engine is bound to.
        steps = lambda n, t: bool(t.requires_grad) and n.startswith(with_grad)  # (engine_steps with the module lists at hand)
        want = [(n, t) for n, t in live if steps(n, t)]
        layout = tuple((n, int(t.numel())) for n, t in want)
        dev = want[0][1].device if want else None
        if want and (self._fine_train_flat is None or self._fine_train_flat_layout != layout or self._fine_train_flat.device != dev):
            offs, total = [], 0
            for _, t in want:
                offs.append(total)
                total += (int(t.numel()) + 63) // 64 * 64
            self._fine_train_flat = torch.zeros(total, dtype=torch.float32, device=dev)
            self._fine_train_flat_layout = layout
            self._fine_train_grads = {n: self._fine_train_flat[o:o + t.numel()].view(t.shape) for (n, t), o in zip(want, offs)}
        for n, t in live:
            if not steps(n, t):
                out[n] = (t.data, None)  # frozen: no gradient
                continue
            g = self._fine_train_grads[n]
            if n.startswith(BACKBONE):
                self._fine_train_pn_live.append((t, g))
            else:
                adopt_grad(t, g)
            out[n] = (t.data, g)
        for n, b in self.named_buffers():
            if n.startswith(run) and n.endswith(("running_mean", "running_var")):
                out[n] = (b, None)
        return out

    def engine_steps(self, name: str, param) -> bool:
        """Does the engine step differentiate (and ``optim.Adam`` step on the engine) this parameter? The modules of
        ``_fine_train_modules`` that receive a gradient, minus the backbone's classifier heads and whatever is frozen."""
        _, with_grad = self._fine_train_modules()
        return bool(param.requires_grad) and name.startswith(with_grad) and not name.startswith(_HEADS)

    def engine_adam_order(self):
        """[(name, parameter)] in the order of t2l_fine_adam_state's moments: bind order, the backbone's group behind the rest."""
        own = [(n, p) for n, p in self.named_parameters() if self.engine_steps(n, p)]
        return [x for x in own if not x[0].startswith(BACKBONE)] + [x for x in own if x[0].startswith(BACKBONE)]

    def train_flat_grad(self) -> Optional[torch.Tensor]:
        """The flat buffer every engine-stepped parameter's ``.grad`` is a view of (None before the first bind)."""
        return self._fine_train_flat

    def _fine_train_dropout(self) -> float:
        """The one dropout probability the engine applies at all six sites of every decoder layer; layers (or sites) that
        disagree are refused rather than trained with the wrong p."""
        layers = list(self.cross_hints) + list(self.cross_objects) if self.cross_objects is not None else [self.cross_hints]
        ps = set()
        for l in layers:
            ps |= {float(l.dropout.p), float(l.dropout1.p), float(l.dropout2.p), float(l.dropout3.p),
                   float(l.self_attn.dropout), float(l.multihead_attn.dropout)}
        if len(ps) != 1:
            raise T2LError(f"the engine applies one dropout probability to every decoder layer; these layers use {sorted(ps)}")
        return ps.pop()

    def _fine_train_engine(self) -> Engine:
        """The engine with t2l_fine_train_bind pointing at the CURRENT parameter / gradient / buffer storage (no re-packing:
        the step reads the live tensors). Every call walks the module's parameters as they are now: a replaced Parameter re-binds."""
        eng, a = self._device_engine(), self.args
        # (rebind: the same model on moved storage — model.to(), a re-assigned .grad — keeps the engine-side Adam moments)
        self._fine_train_bound = rebind(eng, self._fine_train_tensors(), self._fine_train_bound, lambda tensors: eng.fine_train_bind(
            tensors, class_embed=bool(getattr(a, "class_embed", False)), color_embed=bool(getattr(a, "color_embed", False)),
            use_features=tuple(a.use_features), num_layers=a.fine_num_decoder_layers, num_heads=a.fine_num_decoder_heads))
        _apply_sync_bn(eng, self._sync_bn_cfg)
        return eng

    def sync_batchnorm(self, group=None, enable: bool = True):
        """Data-parallel training with the reference's batch statistics: every BatchNorm1d of the ObjectEncoder's branches and
        mlp_merge (object_encoder.py:41-52,121-149) and the hint encoder's inter_mlp (language_encoder.py:99) normalises over the
        objects / hints of ALL ranks' pairs — W ranks x B/W pairs then take the step the reference takes on its one batch of B
        (training/fine.py:38-91). The PointNet++ backbone is not part of this: its BatchNorms use per-cell statistics and a cell lives
        on one rank. Needs an initialised process group; ``optim.Adam(model, data_parallel=True, grad_reduce="mean")`` completes the
        step (the fine loss is a mean over the local rows)."""
        cfg = (group,) if enable else None
        self._sync_bn_cfg = cfg
        if hasattr(self.language_encoder, "_bind_text_train"):
            self.language_encoder._sync_bn_cfg = cfg

    def _forward_train(self, objects, hints, object_points):
        if any(len(o) != PAD_SIZE for o in objects):
            raise T2LError(f"every cell must hold exactly pad_size={PAD_SIZE} objects (cross_matcher.pad_objects pads / cuts)")
        a, dev = self.args, self.device
        pn = pts = None
        if not bool(getattr(a, "class_embed", False)):  # object_encoder.py:86-99: features2 whenever class_embed is off
            pn = self._read_points(objects, object_points)
            if isinstance(pn, tuple):
                pn, pts = None, pn[:2]
                if dev.type != "cuda":
                    raise T2LError("training the fine stage on point batches needs the jointly trained PointNet++ backbone, which is not "
                                   "built for the fine stage on the host: it runs on the MI355X only (model.to('cuda')); there is no CPU fallback")
        p_drop = self._fine_train_dropout()                         # nn.TransformerDecoderLayer default 0.1
        eng = self._fine_train_engine()
        packed = pack_objects(eng, objects, self.object_encoder, dev)
        hint_enc = self.language_encoder(hints)  # [B, n_hints, 128]  (cross_matcher.py:95): the engine's training head behind T5
        if hint_enc.dim() != 3 or hint_enc.shape[0] != len(objects) or not 1 <= hint_enc.shape[1] <= 8 or hint_enc.shape[2] != FINE_DIM:
            raise T2LError(f"hint encodings must be [B={len(objects)}, 1..8, 128], got {tuple(hint_enc.shape)}")
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())        # torch.manual_seed governs the masks
        self._fine_train_hook = hook_leaf(self._fine_train_hook, dev)
        out = _FineTrainFn.apply(self._fine_train_hook, hint_enc, pn, self, packed, p_drop, seed, pts)
        run, _ = self._fine_train_modules()
        bump_batches_tracked(self.named_modules(), lambda name: (name + ".").startswith(run), BACKBONE, len(objects) if pts is not None else 0)
        self._train_generation += 1  # running statistics moved: the eval path must re-load its weights
        return out


class _FineTrainFn(torch.autograd.Function):
    """Training-mode CrossMatch downstream of the text branch: forward and backward are HIP (t2l_fine_train_forward /
    _backward). Parameter gradients do not flow through autograd: the engine adds them straight into the bound ``.grad``
    buffers; the differentiable inputs are the hint encodings and features2 (``hook`` is a dummy leaf that makes autograd call
    ``backward`` even when neither requires grad). ``pts`` = (pos, rgb): features2 comes from the backbone's training-mode
    forward instead, and the backward continues into it when it trains."""

    @staticmethod
    def forward(ctx, hook, hint_enc, pn, model, packed, p_drop, seed, pts=None):
        hint_c = hint_enc.detach().float().contiguous()
        pn_c = None if pn is None else pn.detach().contiguous()
        if pts is not None:
            out = model._engine.fine_train_forward_points(packed, pts[0], pts[1], hint_c, dropout_p=p_drop, seed=seed)
        else:
            out = model._engine.fine_train_forward(packed, pn_c, hint_c, dropout_p=p_drop, seed=seed)
        ctx.model = model
        ctx.token = new_token(model, "_fine_train_token")
        ctx.hint_shape, ctx.hint_dtype = hint_c.shape, hint_enc.dtype
        ctx.pn_shape = None if pn is None else pn_c.shape
        ctx.pn_live = list(model._fine_train_pn_live) if pts is not None else []  # the backbone's backward will run
        return out

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        check_token(model, "_fine_train_token", ctx.token, "CrossMatch training forward")
        need_hint, need_pn = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gh = torch.empty(ctx.hint_shape, dtype=torch.float32, device=grad_out.device) if need_hint else None
        gp = torch.empty(ctx.pn_shape, dtype=torch.float32, device=grad_out.device) if need_pn else None
        for t, g in ctx.pn_live:  # the engine ADDS into the bound buffers: give them the value .grad has now ...
            if t.grad is None:
                g.zero_()
            elif t.grad.data_ptr() != g.data_ptr():
                g.copy_(t.grad)
        model._engine.fine_train_backward(grad_out.contiguous().float(), gh, gp)
        for t, g in ctx.pn_live:  # ... and hand them out only once the backward went through the backbone (adopt_grad in two halves)
            t.grad = g
        return None, (gh.to(ctx.hint_dtype) if gh is not None else None), gp, None, None, None, None, None


@torch.no_grad()
def encode_pose_hints(language_encoder, texts: List[str], max_batch: int = 256) -> torch.Tensor:
    """Hint encodings [n_poses, n_hints, 128] of one text per pose, equal to what the reference's per-pose call produces.

    The reference runs the model once per pose on ``max(top_k)`` copies of that pose's text (evaluation/pipeline.py:113-116,
    dataloading/kitti360pose/eval.py:181-186), so ``padding='longest'`` pads to THAT pose's longest hint — and the
    intra-module TransformerEncoderLayers have no padding mask and max-pool over every token position
    (language_encoder.py:127-134), i.e. the pad length is part of the result. Poses are therefore batched only with
    poses of the same (hint count, padded token length): inside such a group a joint call pads exactly like the
    per-pose call. One tokenizer pass per pose decides the groups; the model runs once per group chunk."""
    tok = getattr(language_encoder, "tokenizer", None)
    split = getattr(language_encoder, "split_sentences", None)
    if tok is None or split is None:  # injected encoders without a tokenizer (tests with a table): one call per pose
        return torch.cat([language_encoder([t]) for t in texts]) if texts else torch.zeros((0, 0, FINE_DIM))
    groups = {}
    for i, t in enumerate(texts):
        ss = split(t)
        ids = tok(ss, return_tensors="pt", padding="longest")["input_ids"]
        groups.setdefault((len(ss), int(ids.shape[1])), []).append(i)
    if len({k[0] for k in groups}) > 1:
        raise T2LError(f"poses carry different numbers of hints: {sorted({k[0] for k in groups})}")
    out = None
    for _, members in sorted(groups.items()):
        for lo in range(0, len(members), max_batch):
            sel = members[lo:lo + max_batch]
            enc = language_encoder([texts[i] for i in sel])
            if out is None:
                out = torch.empty((len(texts),) + tuple(enc.shape[1:]), dtype=enc.dtype, device=enc.device)
            out[torch.as_tensor(sel, device=enc.device)] = enc
    return out if out is not None else torch.zeros((0, 0, FINE_DIM))


@torch.no_grad()
def run_fine(model: CrossMatch, retrievals, dataloader, args, transform_fine=None, object_points_fn=None,
             return_offsets: bool = False):
    """evaluation/pipeline.py:88-204: offsets of every pose against its max(top_k) retrieved cells -> {k: {t: accuracy}}.
    The reference builds a ``Kitti360TopKDataset`` item per pose and runs one forward per pose, re-encoding a cell for
    every pose that retrieved it; here every distinct retrieved cell is padded and encoded ONCE, every pose's hints are
    encoded once, and all poses x max(top_k) pairs are matched in one launch.
    ``object_points_fn(list_of_padded_object_lists) -> object_points`` supplies the PointNet++ inputs in the published
    feature mode. Without one they are sampled here (``packing.sample_object_points``) under ``transform_fine`` — a transform
    name ("fixed" / "normalize"), or, as in the reference's script, chosen from ``args.no_pc_augment_fine``
    (evaluation/pipeline.py:220-223: FixedPoints only under the flag, which the published commands pass)."""
    model.eval()
    a = model.args
    if object_points_fn is None and "class" in a.use_features and not bool(getattr(a, "class_embed", False)):
        name = transform_fine if isinstance(transform_fine, str) else packing.point_transform_from_args(args, fine=True)
        pts_rng = np.random.default_rng(int(getattr(args, "seed", 0) or 0))

        def object_points_fn(chunk):
            return packing.sample_object_points(chunk, 256, pts_rng, transform=name)
    ds = dataloader.dataset
    poses, cells = ds.all_poses, ds.all_cells
    K = max(args.top_k)
    assert len(poses) == len(retrievals) and all(len(r) == K for r in retrievals), "retrievals must be trimmed to max(top_k)"
    cells_dict = {c.id: c for c in cells}
    uniq = sorted({str(cid) for r in retrievals for cid in r})
    row = {cid: i for i, cid in enumerate(uniq)}
    # OPT-IN, like coarse.eval_epoch (args.shard_layout set to anything but None / "none"): with more than one process (one per GPU)
    # the distinct cells and the (pose, cell) pairs are split across the ranks in contiguous blocks — no exchange inside either
    # stage — and all-gathered once each. Every rank must then call run_fine with the same retrievals (proven by one small
    # all_reduce); without the option an initialised process group changes nothing (rank-0-only validation stays local).
    from .sharded import assert_replicated, gather_rows, shard_bounds, world_rank

    layout = getattr(args, "shard_layout", None) or getattr(a, "shard_layout", None)
    world, rank = world_rank() if layout not in (None, "", "none", "off") else (1, 0)
    if world > 1:
        assert_replicated([torch.tensor([row[str(cid)] for r in retrievals for cid in r], dtype=torch.float64)], None, "retrievals")
    c_lo, c_hi = shard_bounds(len(uniq), world, rank)
    padded = [pad_objects(cells_dict[cid].objects) for cid in uniq[c_lo:c_hi]]
    descs = []
    for lo in range(0, len(padded), 2048):
        chunk = padded[lo:lo + 2048]
        descs.append(model.encode_cells(chunk, object_points_fn(chunk) if object_points_fn is not None else None))
    cell_desc = torch.cat(descs) if descs else torch.zeros((0, PAD_SIZE, FINE_DIM), device=model.device)
    cell_desc = gather_rows(cell_desc, len(uniq)) if world > 1 else cell_desc
    hint_desc = encode_pose_hints(model.language_encoder, [" ".join(create_hint_description(p)) for p in poses])
    ci = np.array([row[str(cid)] for r in retrievals for cid in r], dtype=np.int32)
    hi = np.repeat(np.arange(len(poses), dtype=np.int32), K)
    p_lo, p_hi = shard_bounds(len(ci), world, rank)
    local = model.match(cell_desc, hint_desc, ci[p_lo:p_hi], hi[p_lo:p_hi]) if p_hi > p_lo else \
        torch.zeros((0, 2), device=model.device)
    offsets = (gather_rows(local, len(ci)) if world > 1 else local).cpu().numpy().reshape(len(poses), K, 2)
    from .coarse import _pose_cell_tables, sample_accuracies_batch

    pose_xy, pose_scene, bbox_xy, size, scene = _pose_cell_tables(poses, cells, retrievals)
    ok = sample_accuracies_batch(pose_xy, pose_scene, bbox_xy, size, scene, offsets.astype(np.float64), args.top_k, args.threshs)
    acc = {k: {t: float(np.mean(ok[k][t])) for t in args.threshs} for k in args.top_k}
    return (acc, offsets) if return_offsets else acc  # offsets f32[n_poses, max(top_k), 2]: the per-pair estimates
