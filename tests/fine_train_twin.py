"""TEST INFRASTRUCTURE — a float64 torch twin of one training step of the fine stage downstream of the text branch:
``CrossMatch.forward`` under ``model.train()`` (models/cross_matcher.py:86-135; ObjectEncoder with batch-statistics
BatchNorm1d, the cascaded nn.TransformerDecoderLayers with their six dropout sites, max over the hints, mlp_offsets), written
out op by op so that the dropout masks can be the ABI's counter-based ones (include/t2l.h: t2l_fine_train_forward). Gradients
come from torch autograd.

``module_step`` runs the same step through torch's OWN modules (the package's CrossMatch parameter containers are real
nn.Linear / nn.BatchNorm1d / nn.TransformerDecoderLayer modules) with dropout 0; tests/test_oracle_fine_train.py pins the
twin to it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.t2l_oracle_train import NUM_MEAN, NUM_STD, dropout_keep

F32 = np.float32
FEATURES = ("class", "color", "position", "num")


def _drop(x, seed, site, p):
    if p <= 0.0 or int(p * (1 << 24)) == 0:
        return x
    keep = torch.from_numpy(dropout_keep(seed, site, x.numel(), p).reshape(tuple(x.shape)))
    return x * keep.to(x.dtype) / (1.0 - p)


def _num_input(n_pts):
    return ((np.asarray(n_pts).astype(F32)[:, None] - F32(NUM_MEAN)) / F32(NUM_STD)).astype(F32)


class Twin:
    """Parameters as float64 leaf tensors (every float entry of ``sd``), BatchNorm running buffers updated by ``step``."""

    def __init__(self, sd: dict, class_embed: bool, color_embed: bool, use_features=FEATURES, n_layers: int = 2,
                 dtype=torch.float64):
        self.dtype = dtype
        self.t = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad="running_" not in k)
                  for k, v in sd.items() if np.asarray(v).dtype.kind == "f" and not k.startswith(("language_encoder.", "object_encoder.pointnet."))}
        self.class_embed, self.color_embed = class_embed, color_embed
        self.use = tuple(f for f in FEATURES if f in use_features)
        self.n_layers = n_layers

    # ---- building blocks ----------------------------------------------------------------------------------
    def _mlp(self, x, prefix, n, train):
        for i in range(n):
            w, b = self.t[f"{prefix}.{i}.0.weight"], self.t[f"{prefix}.{i}.0.bias"]
            y = x @ w.T + b
            g, bb = self.t[f"{prefix}.{i}.1.weight"], self.t[f"{prefix}.{i}.1.bias"]
            rm, rv = self.t[f"{prefix}.{i}.1.running_mean"], self.t[f"{prefix}.{i}.1.running_var"]
            if train:
                mean, var = y.mean(0), y.var(0, unbiased=False)
                with torch.no_grad():
                    rm.mul_(0.9).add_(0.1 * mean)
                    rv.mul_(0.9).add_(0.1 * y.var(0, unbiased=True))
            else:
                mean, var = rm, rv
            x = torch.relu((y - mean) / torch.sqrt(var + 1e-5) * g + bb)
        return x

    def encode_objects(self, cells, pn_feat=None, train=True):
        p = "object_encoder."
        emb = []
        T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=self.dtype)
        if "class" in self.use:
            if self.class_embed:
                e = F.embedding(torch.as_tensor(np.asarray(cells["class_idx"], dtype=np.int64)), self.t[p + "class_embedding.weight"], padding_idx=0)
            else:
                e = self._mlp(pn_feat, p + "mlp_pointnet", 1, train)
            emb.append(F.normalize(e, dim=-1))
        elif not self.class_embed:  # object_encoder.py:86-99 runs mlp_pointnet whenever class_embed is off
            self._mlp(pn_feat, p + "mlp_pointnet", 1, train)
        if "color" in self.use:
            if self.color_embed:
                e = F.embedding(torch.as_tensor(np.asarray(cells["color_idx"], dtype=np.int64)), self.t[p + "color_embedding.weight"], padding_idx=0)
            else:
                e = self._mlp(T(cells["rgb"]), p + "color_encoder", 2, train)
            emb.append(F.normalize(e, dim=-1))
        if "position" in self.use:
            emb.append(F.normalize(self._mlp(T(cells["center"]), p + "pos_encoder", 2, train), dim=-1))
        if "num" in self.use:
            emb.append(F.normalize(self._mlp(T(_num_input(cells["n_pts"])), p + "num_encoder", 2, train), dim=-1))
        x = self._mlp(torch.cat(emb, -1), p + "mlp_merge", 1, train) if len(emb) > 1 else emb[0]
        return F.normalize(x, dim=-1)

    def _mha(self, q_in, kv_in, prefix, p, seed, site):
        D, H = 128, 4
        w, b = self.t[prefix + ".in_proj_weight"], self.t[prefix + ".in_proj_bias"]
        q = q_in @ w[:D].T + b[:D]
        k = kv_in @ w[D:2 * D].T + b[D:2 * D]
        v = kv_in @ w[2 * D:].T + b[2 * D:]
        heads = lambda a: a.reshape(a.shape[0], a.shape[1], H, D // H).transpose(1, 2)  # [P,H,T,hd]
        q, k, v = heads(q), heads(k), heads(v)
        a = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(D // H), dim=-1)
        a = _drop(a, seed, site, p)
        o = (a @ v).transpose(1, 2).reshape(q_in.shape)
        return o @ self.t[prefix + ".out_proj.weight"].T + self.t[prefix + ".out_proj.bias"]

    def _ln(self, x, prefix):
        return F.layer_norm(x, (128,), self.t[prefix + ".weight"], self.t[prefix + ".bias"], 1e-5)

    def decoder_layer(self, x, mem, prefix, p, seed, site):
        t = self.t
        x = self._ln(x + _drop(self._mha(x, x, prefix + ".self_attn", p, seed, site), seed, site + 1, p), prefix + ".norm1")
        x = self._ln(x + _drop(self._mha(x, mem, prefix + ".multihead_attn", p, seed, site + 2), seed, site + 3, p), prefix + ".norm2")
        h = _drop(torch.relu(x @ t[prefix + ".linear1.weight"].T + t[prefix + ".linear1.bias"]), seed, site + 4, p)
        f = h @ t[prefix + ".linear2.weight"].T + t[prefix + ".linear2.bias"]
        return self._ln(x + _drop(f, seed, site + 5, p), prefix + ".norm3")

    def forward(self, cells, hints, pn_feat=None, p=0.0, seed=0, train=True):
        """cells: packed numpy arrays of P padded cells (16 objects each); hints, pn_feat: tensors in the twin's dtype."""
        P = hints.shape[0]
        obj = self.encode_objects(cells, pn_feat, train).reshape(P, 16, 128)
        hint = hints
        if self.n_layers == 0:
            hint = self.decoder_layer(hint, obj, "cross_hints", p, seed, 0)
        for i in range(self.n_layers):
            obj = self.decoder_layer(obj, hint, f"cross_objects.{i}", p, seed, 6 * (2 * i))
            hint = self.decoder_layer(hint, obj, f"cross_hints.{i}", p, seed, 6 * (2 * i + 1))
        h = hint.max(dim=1).values
        h = torch.relu(h @ self.t["mlp_offsets.0.weight"].T + self.t["mlp_offsets.0.bias"])
        return h @ self.t["mlp_offsets.2.weight"].T + self.t["mlp_offsets.2.bias"]

    def step(self, cells, hints, grad_offsets, pn_feat=None, p=0.0, seed=0):
        """Training forward + backward with upstream gradient ``grad_offsets``. Returns (offsets, grads, grad_hint, grad_pn)
        as numpy; parameter gradients are fresh per call (the twin does not accumulate)."""
        for v in self.t.values():
            v.grad = None
        h = torch.as_tensor(np.asarray(hints, dtype=np.float64), dtype=self.dtype).requires_grad_(True)
        pn = None if pn_feat is None else torch.as_tensor(np.asarray(pn_feat, dtype=np.float64), dtype=self.dtype).requires_grad_(True)
        off = self.forward(cells, h, pn, p, seed, train=True)
        (off * torch.as_tensor(np.asarray(grad_offsets, dtype=np.float64), dtype=self.dtype)).sum().backward()
        grads = {k: v.grad.numpy() for k, v in self.t.items() if v.grad is not None}
        return off.detach().numpy(), grads, h.grad.numpy(), None if pn is None or pn.grad is None else pn.grad.numpy()

    def running(self):
        return {k: v.detach().numpy().copy() for k, v in self.t.items() if "running_" in k}

    def params(self):
        return {k: v.detach().numpy().copy() for k, v in self.t.items()}


def module_step(model, cells, hints, grad_offsets, pn_feat=None):
    """The same step through torch's own modules of a (CPU, float64, train-mode, dropout-0) ``CrossMatch`` parameter container:
    get_mlp Sequentials, nn.TransformerDecoderLayer(tgt [T,P,D], memory [T,P,D]) as models/cross_matcher.py:109-124 calls them.
    Returns (offsets, {name: grad}, grad_hint, grad_pn)."""
    a = model.args
    oe = model.object_encoder
    use = [f for f in FEATURES if f in a.use_features]
    T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    model.zero_grad(set_to_none=True)
    h = T(hints).requires_grad_(True)
    pn = None if pn_feat is None else T(pn_feat).requires_grad_(True)
    emb = []
    if "class" in use:
        e = oe.class_embedding(torch.as_tensor(np.asarray(cells["class_idx"], dtype=np.int64))) if a.class_embed else oe.mlp_pointnet(pn)
        emb.append(F.normalize(e, dim=-1))
    elif not a.class_embed:
        oe.mlp_pointnet(pn)
    if "color" in use:
        e = oe.color_embedding(torch.as_tensor(np.asarray(cells["color_idx"], dtype=np.int64))) if a.color_embed else oe.color_encoder(T(cells["rgb"]))
        emb.append(F.normalize(e, dim=-1))
    if "position" in use:
        emb.append(F.normalize(oe.pos_encoder(T(cells["center"])), dim=-1))
    if "num" in use:
        emb.append(F.normalize(oe.num_encoder(T(_num_input(cells["n_pts"]))), dim=-1))
    x = oe.mlp_merge(torch.cat(emb, -1)) if len(emb) > 1 else emb[0]
    obj = F.normalize(x, dim=-1).reshape(h.shape[0], 16, 128).transpose(0, 1)
    hint = h.transpose(0, 1)
    if a.fine_num_decoder_layers == 0:
        hint = model.cross_hints(hint, obj)
    for i in range(a.fine_num_decoder_layers):
        obj = model.cross_objects[i](obj, hint)
        hint = model.cross_hints[i](hint, obj)
    off = model.mlp_offsets(hint.max(dim=0).values)
    (off * T(grad_offsets)).sum().backward()
    grads = {n: q.grad.numpy() for n, q in model.named_parameters() if q.grad is not None}
    return off.detach().numpy(), grads, h.grad.numpy(), None if pn is None or pn.grad is None else pn.grad.numpy()
