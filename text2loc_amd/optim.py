"""``optim.Adam(model.parameters(), lr)`` of the reference's training script (training/coarse.py:258) for a
``text2loc_amd.CellRetrievalNetwork``: the object-branch parameters (with the PointNet++ backbone when it trains) are stepped by the engine's multi-tensor Adam kernel
(t2l_adam_step: one launch over every bound tensor, moments kept in HBM by the library), everything else (the language
head) by ``torch.optim.Adam`` with the same hyper-parameters. It is a ``torch.optim.Optimizer``, so the reference's
``ExponentialLR`` / ``StepLR`` schedulers (training/coarse.py:268-273) drive it unchanged through ``param_groups``.

Data-parallel training (one process per GPU; not in the reference — SURVEY.md 8e): ``Adam(model, lr, group=pg)`` all-reduces
the gradients at the top of ``step()``. The engine-stepped parameters' ``.grad`` are views of ONE flat buffer
(``CellRetrievalNetwork.train_flat_grad``), so they travel as a single RCCL all_reduce (16.5 M floats = 66 MB with the
backbone: per-link bound on xGMI, one large collective instead of ~150 small ones); the language head's gradients are
flattened into a second one. ``grad_reduce="sum"`` pairs with ``ContrastiveLoss(group=pg)`` (every rank differentiates the
GLOBAL loss w.r.t. its own rows: the sum over ranks is the exact gradient; the default here); ``"mean"`` is the usual average for
per-rank losses.

``Adam(model)`` with a ``text2loc_amd.CrossMatch`` is the fine stage's optimizer (training/fine.py:57,72,229) and returns a ``FineAdam``:
the decoders, mlp_offsets, the object-encoder branches and the jointly trained backbone on t2l_fine_zero_grad / t2l_fine_adam_step,
the hint encoder's head on t2l_text_adam_step. The fine loss is a MEAN over the local rows (``offset_lambda * MSE``), so its
data-parallel step takes ``grad_reduce="mean"`` (a ``FineAdam``'s default): with equal shards the mean of the ranks' gradients is the gradient of the
one-process batch (the coarse step's ``"sum"`` belongs to its gathered, global loss). Only several processes on one GPU were run; no
scaling curve was measured.
"""
from __future__ import annotations

import torch


def all_reduce_flat(buf: torch.Tensor, group=None, mean: bool = False) -> torch.Tensor:
    """In-place all_reduce (sum, or mean) of one flat gradient buffer: RCCL on the tensor's own device under "nccl"; under gloo a
    device tensor is staged through the host (several processes on one GPU in the tests — RCCL refuses duplicate devices)."""
    import torch.distributed as dist

    if buf.is_cuda and dist.get_backend(group) != "nccl":
        h = buf.cpu()
        dist.all_reduce(h, group=group)
        buf.copy_(h)
    else:
        dist.all_reduce(buf, group=group)
    if mean:
        buf.div_(dist.get_world_size(group))
    return buf


class Adam(torch.optim.Optimizer):
    DEFAULT_GRAD_REDUCE = "sum"  # (the coarse step differentiates a gathered, global loss)

    def __new__(cls, model=None, *args, **kwargs):
        # Adam(model) with a CrossMatch is a FineAdam: the one __init__ below runs for both, through the three hooks FineAdam overrides
        # (which parameters the engine steps, which head parameters, the default reduction)
        return super().__new__(FineAdam if cls is Adam and hasattr(model, "_fine_train_engine") else cls)

    @staticmethod
    def _engine_steps(model, n, p) -> bool:
        """Does the engine's Adam kernel step parameter ``n``? The object branch incl. the PointNet++ backbone unless --pointnet_freeze;
        not the backbone's classifier heads (not on the coarse path — features2 is consumed, they train in pointnet_pretrain: .grad
        stays None and torch skips them as in the reference)."""
        return n.startswith(("object_encoder.", "obj_inter_module.")) and not n.startswith(
            ("object_encoder.pointnet.class_classifier.", "object_encoder.pointnet.color_classifier."))

    @staticmethod
    def _head_params(le):
        return le.engine_optimizer_params() if hasattr(le, "engine_optimizer_params") else []

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, group=None, grad_reduce: str = None,
                 data_parallel: bool = False, sync_bn: bool = False, text_engine: bool = True):
        """``group``: a torch.distributed process group, or ``data_parallel=True`` for the default one — turns the gradient
        all-reduce of ``step()`` on. ``sync_bn``: also ``model.sync_batchnorm(group)`` — BatchNorm statistics over all ranks' batches,
        i.e. the reference's one-process step on the global batch. ``text_engine``: the language head's trained parameters (when the
        engine's training head serves this model: ``LanguageEncoder.engine_optimizer_params``) are stepped by ``t2l_text_adam_step`` — one
        launch, moments inside the library — instead of a torch.optim.Adam beside the engine."""
        grad_reduce = self.DEFAULT_GRAD_REDUCE if grad_reduce is None else grad_reduce
        if grad_reduce not in ("sum", "mean"):
            raise ValueError("grad_reduce must be 'sum' or 'mean'")
        if not getattr(model, "published_shape", True):
            from .engine import TRAIN_SHAPE_MSG, T2LError

            raise T2LError("optim.Adam: " + TRAIN_SHAPE_MSG)
        self._group, self._grad_reduce, self._dp = group, grad_reduce, bool(data_parallel) or group is not None
        obj, rest, text = [], [], []
        le = getattr(model, "language_encoder", None)
        on_gpu = any(p.is_cuda for p in model.parameters())
        head = self._head_params(le) if (text_engine and on_gpu) else []
        text_ids = {id(p) for _, p in head}
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            # the text head's trained parameters: t2l_text_adam_step (one launch, moments inside the library)
            (text if id(p) in text_ids else obj if self._engine_steps(model, n, p) else rest).append(p)
        # names in named_parameters order of everything the object-branch kernel does NOT step, and which optimizer steps each here:
        # a checkpoint written under the other ``text_engine`` setting (or before the head moved into the engine) holds the same
        # moments under the other layout — load_state_dict migrates by these names
        text_set = {id(p) for p in text}
        obj_set = {id(p) for p in obj}
        self._non_obj = [(n, p, "text" if id(p) in text_set else "rest") for n, p in model.named_parameters()
                         if p.requires_grad and id(p) not in obj_set]
        groups = [{"params": obj, "t2l_engine": True}]
        if rest:
            groups.append({"params": rest, "t2l_engine": False})
        if text:
            groups.append({"params": text, "t2l_engine": "text_head"})
        super().__init__(groups, dict(lr=lr, betas=tuple(betas), eps=eps))
        self._model = model
        self._text = bool(text)
        self._head = [("language_encoder." + n, p) for n, p in head]
        self._rest = rest
        if sync_bn:
            model.sync_batchnorm(group)
        self._torch = torch.optim.Adam(rest, lr=lr, betas=tuple(betas), eps=eps) if rest else None

    def zero_grad(self, set_to_none: bool = False):
        """Object-branch gradients are zeroed IN PLACE by one kernel (the engine accumulates into fixed buffers)."""
        if self._model.device.type == "cuda":
            self._model.train_engine().zero_grad()
            if self._text:
                self._model.language_encoder.engine_zero_grad()  # in place: the engine accumulates into the bound buffers
        if self._torch is not None:
            self._torch.zero_grad(set_to_none=set_to_none)

    def _bound_engine(self):
        return self._model.train_engine()

    # ---- data parallel ------------------------------------------------------------------------------------------------
    def _world(self) -> int:
        import torch.distributed as dist

        if not self._dp:
            return 1
        return dist.get_world_size(self._group) if dist.is_available() and dist.is_initialized() else 1

    @torch.no_grad()
    def all_reduce_grads(self):
        """ONE all_reduce over the engine-owned flat gradient buffer + one over the flattened torch-side gradients."""
        world = self._world()
        if world == 1:
            return
        self._bound_engine()  # binds (and so allocates) the flat buffer if nothing has yet
        bufs = []
        flat = self._model.train_flat_grad()
        if flat is not None:
            bufs.append((flat, None))
        # a rank-INDEPENDENT list: every torch-side parameter, a missing gradient (a branch this rank's batch skipped, set_to_none) as
        # zeros — ranks that disagreed on which gradients exist would issue all_reduces of different sizes (a hang, or silent garbage)
        rest = [p for g in self.param_groups[1:] for p in g["params"]]
        if rest:
            bufs.append((torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in rest]), rest))
        for buf, params in bufs:
            all_reduce_flat(buf, self._group, mean=self._grad_reduce == "mean")
            if params is not None:
                off = 0
                for p in params:
                    g = buf[off:off + p.numel()].view_as(p)
                    if p.grad is None:
                        p.grad = g.clone()  # (another rank may have contributed: every rank steps the same set)
                    else:
                        p.grad.copy_(g)
                    off += p.numel()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.all_reduce_grads()
        g = self.param_groups[0]
        eng = self._model.train_engine()
        eng.adam_step(g["lr"], g["betas"][0], g["betas"][1], g["eps"])
        self._model._train_generation += 1  # parameters changed behind torch's back: eval weights must be re-folded
        if self._torch is not None:
            for src, dst in zip([g_ for g_ in self.param_groups[1:] if g_["t2l_engine"] is False], self._torch.param_groups):
                dst["lr"], dst["betas"], dst["eps"] = src["lr"], src["betas"], src["eps"]
            self._torch.step()
        if self._text:
            gt = self.param_groups[-1]
            self._model.language_encoder.engine_adam_step(gt["lr"], gt["betas"], gt["eps"])
        return loss

    # ---- checkpoint / resume: the engine-side moments are part of the optimizer state -------------------------------
    def state_dict(self):
        sd = {"param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
              "torch": self._torch.state_dict() if self._torch is not None else None, "t2l_engine": None, "t2l_text_engine": None}
        if self._model.device.type == "cuda":
            m, v, step = self._model.train_engine().adam_state()
            # the engine keeps one bias-correction step for the object branch and one for the PointNet++ backbone (which only steps
            # when its backward ran): two explicit fields (round 3 leaked the packed word step | step_pn << 32 into "step")
            sd["t2l_engine"] = {"exp_avg": m.cpu(), "exp_avg_sq": v.cpu(), "step": int(step) & 0xFFFFFFFF, "step_pn": int(step) >> 32}
            if self._text:
                le = self._model.language_encoder
                le._bind_text_train(self._model.device)
                m, v, step = le._th_train_engine.text_adam_state()
                sd["t2l_text_engine"] = {"exp_avg": m.cpu(), "exp_avg_sq": v.cpu(), "step": int(step)}
        return sd

    def _saved_moments(self, sd):
        """{parameter name: (exp_avg, exp_avg_sq, step)} of every non-object-branch parameter a checkpoint holds moments for, whichever
        layout wrote it: (i) head inside ``sd["torch"]`` (``text_engine=False``, CPU models, checkpoints older than the engine-side head);
        (ii) head as the engine's flat moments ``sd["t2l_text_engine"]`` (bind order = named_parameters order) + the rest in ``sd["torch"]``.
        A checkpoint that fits neither raises, naming the sizes — never a silent restart of Adam."""
        names_all = [n for n, _, _ in self._non_obj]
        names_rest = [n for n, _, k in self._non_obj if k == "rest"]
        text = [(n, p) for n, p, k in self._non_obj if k == "text"]
        ts, te = sd.get("torch"), sd.get("t2l_text_engine")
        n_saved = sum(len(g["params"]) for g in ts["param_groups"]) if ts is not None else 0
        out = {}
        if te is None:
            if n_saved == len(names_all):
                order = names_all                      # layout (i): the head's moments sit in the torch optimizer's state
            elif n_saved == len(names_rest) and not text:
                order = names_rest
            else:
                raise ValueError(f"optimizer checkpoint holds {n_saved} torch-side parameters; this model has {len(names_all)} outside the "
                                 f"object branch ({len(text)} of them in the text head): not a checkpoint of this model")
        else:
            head = [(n, p) for n, p in (self._model.language_encoder.engine_optimizer_params()
                                        if hasattr(getattr(self._model, "language_encoder", None), "engine_optimizer_params") else [])]
            head = [("language_encoder." + n, p) for n, p in head]
            total = sum(p.numel() for _, p in head)
            if int(te["exp_avg"].numel()) != total:
                raise ValueError(f"optimizer checkpoint holds {int(te['exp_avg'].numel())} text-head moments; this model's engine head has {total}")
            head_names = {n for n, _ in head}
            order = [n for n in names_all if n not in head_names]
            if n_saved != len(order):
                raise ValueError(f"optimizer checkpoint holds {n_saved} torch-side parameters beside the engine's text head; this model has {len(order)}")
            off = 0
            for n, p_ in head:
                k = p_.numel()
                out[n] = (te["exp_avg"][off:off + k].view_as(p_), te["exp_avg_sq"][off:off + k].view_as(p_), int(te["step"]))
                off += k
        if ts is not None:
            saved_ids = [i for g in ts["param_groups"] for i in g["params"]]
            for i, n in zip(saved_ids, order):
                st = ts["state"].get(i)
                if st:
                    out[n] = (st["exp_avg"], st["exp_avg_sq"], int(st["step"]))
        return out

    def load_state_dict(self, sd):
        # hyper-parameters go back by the group's MARKER, not its position: the two head layouts have different group lists
        # ([obj, rest] against [obj, rest, text] or [obj, text]). A group with no counterpart in the checkpoint is the text head
        # under the other layout: it takes lr / betas / eps of the group that held the head there (text <-> rest); the marker
        # itself is never taken from the checkpoint.
        by_kind = {}
        for sg in sd["param_groups"]:
            by_kind.setdefault(sg.get("t2l_engine", None), sg)
        for g in self.param_groups:
            kind = g["t2l_engine"]
            src = by_kind.get(kind)
            if src is None and kind == "text_head":
                src = by_kind.get(False)
            if src is None and kind is False:
                src = by_kind.get("text_head")
            if src is None:
                continue
            g.update({k: v for k, v in src.items() if k not in ("params", "t2l_engine")})
        saved = self._saved_moments(sd)
        if self._torch is not None:
            rest = [(n, p) for n, p, k in self._non_obj if k == "rest"]
            ref_group = (sd.get("torch") or {}).get("param_groups", [None])[0] or self._torch.state_dict()["param_groups"][0]
            state = {}
            for i, (n, p) in enumerate(rest):
                if n in saved:
                    m, v, step = saved[n]
                    state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.detach().clone().view_as(p), "exp_avg_sq": v.detach().clone().view_as(p)}
            self._torch.load_state_dict({"state": state, "param_groups": [dict(ref_group, params=list(range(len(rest))))]})
        e = sd.get("t2l_engine")
        if e is not None:
            step = int(e["step"])
            step_pn = int(e["step_pn"]) if "step_pn" in e else (step >> 32 if step >> 32 else step & 0xFFFFFFFF)  # older checkpoints:
            self._model.train_engine().set_adam_state(e["exp_avg"], e["exp_avg_sq"], (step & 0xFFFFFFFF) | (step_pn << 32))  # packed, or one step for both
        if self._text:  # the head's moments go into the engine whichever layout the checkpoint used (flat, bind order)
            le = self._model.language_encoder
            le._bind_text_train(self._model.device)
            text = [(n, p) for n, p, k in self._non_obj if k == "text"]
            have = [n for n, _ in text if n in saved]
            if have and len(have) != len(text):
                raise ValueError(f"optimizer checkpoint holds moments for {len(have)} of the {len(text)} text-head tensors")
            if have:
                steps = {saved[n][2] for n, _ in text}
                if len(steps) != 1:
                    raise ValueError(f"text-head tensors of the checkpoint disagree on the Adam step ({sorted(steps)}): the engine keeps one")
                dev = self._model.device
                m = torch.cat([saved[n][0].detach().to(dev, torch.float32).reshape(-1) for n, _ in text])
                v = torch.cat([saved[n][1].detach().to(dev, torch.float32).reshape(-1) for n, _ in text])
                le._th_train_engine.set_text_adam_state(m, v, steps.pop())


class FineAdam(Adam):
    """``Adam(model)`` for a ``CrossMatch`` (constructed through ``Adam``; same keywords and the same ``__init__``, except that
    ``grad_reduce`` defaults to ``"mean"``). Three parameter groups at most: the
    engine's (``CrossMatch.engine_steps``: one zeroing launch, one Adam launch, moments inside the library, ``.grad`` views of
    ``CrossMatch.train_flat_grad()``), whatever is left (``torch.optim.Adam``: a text branch on its PyTorch modules, parameters the
    configuration never differentiates — their ``.grad`` stays None and torch skips them), and the hint encoder's engine head
    (``LanguageEncoder.engine_head_params``: t2l_text_adam_step in its fine layout). Data parallel: ``all_reduce_grads`` sends the flat
    buffer as one collective and every other gradient, the hint encoder's included, as a second.

    ``state_dict()`` is ``torch.optim.Adam(model.parameters())``'s own: one group over every parameter in ``model.parameters()``
    order, exp_avg / exp_avg_sq / step per stepped parameter — a checkpoint written by either optimizer loads into the other."""

    DEFAULT_GRAD_REDUCE = "mean"  # the fine loss is a mean over the local rows: the ranks' gradients are averaged

    @staticmethod
    def _engine_steps(model, n, p) -> bool:
        return model.engine_steps(n, p)

    @staticmethod
    def _head_params(le):
        return le.engine_head_params() if hasattr(le, "engine_head_params") else []

    def _bound_engine(self):
        return self._model._fine_train_engine()

    def zero_grad(self, set_to_none: bool = False):
        """The engine's gradients are zeroed IN PLACE by one kernel (it accumulates into fixed buffers); the backbone then sits out the
        next step unless a backward goes through it again, as a ``.grad`` of None would make it under torch."""
        if self._model.device.type == "cuda":
            self._bound_engine().fine_zero_grad()
            if self._text:
                self._model.language_encoder.engine_zero_grad()
        if self._torch is not None:
            self._torch.zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.all_reduce_grads()
        g = self.param_groups[0]
        self._bound_engine().fine_adam_step(g["lr"], g["betas"][0], g["betas"][1], g["eps"])
        self._model._train_generation += 1  # parameters changed behind torch's back: the eval path must re-load its weights
        if self._torch is not None:
            for src, dst in zip([g_ for g_ in self.param_groups[1:] if g_["t2l_engine"] is False], self._torch.param_groups):
                dst["lr"], dst["betas"], dst["eps"] = src["lr"], src["betas"], src["eps"]
            self._torch.step()
        if self._text:
            gt = self.param_groups[-1]
            self._model.language_encoder.engine_adam_step(gt["lr"], gt["betas"], gt["eps"])
        return loss

    # ---- checkpoint / resume in torch.optim.Adam(model.parameters())'s layout -----------------------------------------------
    def _torch_group(self, n_params: int):
        g = self.param_groups[0]
        ref = torch.optim.Adam([torch.zeros(1)], lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"]).state_dict()["param_groups"][0]
        return dict(ref, params=list(range(n_params)))

    @staticmethod
    def _flat_entries(order, m, v, steps):
        """{id(parameter): state entry} of the tensors of ``order`` = [(name, parameter, which step)] whose step is > 0."""
        out, off = {}, 0
        for _, p, k in order:
            n = p.numel()
            if steps[k] > 0:
                out[id(p)] = {"step": torch.tensor(float(steps[k])), "exp_avg": m[off:off + n].view_as(p).clone(),
                              "exp_avg_sq": v[off:off + n].view_as(p).clone()}
            off += n
        return out

    def _engine_order(self):
        from .cross_matcher import BACKBONE

        return [(n, p, 1 if n.startswith(BACKBONE) else 0) for n, p in self._model.engine_adam_order()]

    def state_dict(self):
        model = self._model
        params = list(model.parameters())
        entries = {}
        if model.device.type == "cuda":
            m, v, step = self._bound_engine().fine_adam_state()
            entries.update(self._flat_entries(self._engine_order(), m, v, (step & 0xFFFFFFFF, step >> 32)))
            if self._text:
                le = model.language_encoder
                le._bind_text_train(model.device)
                m, v, step = le._th_train_engine.text_adam_state()
                entries.update(self._flat_entries([(n, p, 0) for n, p in self._head], m, v, (int(step),)))
        if self._torch is not None:
            ts = self._torch.state_dict()["state"]
            for i, p in enumerate(self._rest):
                if i in ts:
                    entries[id(p)] = ts[i]
        return {"state": {i: entries[id(p)] for i, p in enumerate(params) if id(p) in entries},
                "param_groups": [self._torch_group(len(params))]}

    def _flat_from(self, order, saved, what):
        """(m, v, steps) for the engine from the checkpoint's entries: zeros for a tensor it holds nothing for (never stepped), one step
        count per group — the engine keeps one."""
        dev = self._model.device
        ms, vs, steps = [], [], {}
        for n, p, k in order:
            e = saved.get(id(p))
            if e is None:
                ms.append(torch.zeros(p.numel(), dtype=torch.float32, device=dev))
                vs.append(torch.zeros(p.numel(), dtype=torch.float32, device=dev))
                continue
            if tuple(e["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer checkpoint: moments of {n} are {tuple(e['exp_avg'].shape)}, the parameter is {tuple(p.shape)}")
            ms.append(e["exp_avg"].detach().to(dev, torch.float32).reshape(-1))
            vs.append(e["exp_avg_sq"].detach().to(dev, torch.float32).reshape(-1))
            steps.setdefault(k, set()).add(int(e["step"]))
        for k, st in steps.items():
            if len(st) != 1:
                raise ValueError(f"{what} tensors of the checkpoint disagree on the Adam step ({sorted(st)}): the engine keeps one per group")
        return torch.cat(ms), torch.cat(vs), {k: st.pop() for k, st in steps.items()}

    def load_state_dict(self, sd):
        model = self._model
        params = list(model.parameters())
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        if len(ids) != len(params):
            raise ValueError(f"optimizer checkpoint holds {len(ids)} parameters; this model has {len(params)}: not a checkpoint of "
                             f"torch.optim.Adam(model.parameters()) for this model")
        src = sd["param_groups"][0]
        for g in self.param_groups:
            g.update({k: src[k] for k in ("lr", "betas", "eps") if k in src})
            g["betas"] = tuple(g["betas"])
        saved = {id(p): sd["state"][i] for i, p in zip(ids, params) if i in sd["state"]}
        if self._torch is not None:
            state = {i: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in saved[id(p)].items()}
                     for i, p in enumerate(self._rest) if id(p) in saved}
            self._torch.load_state_dict({"state": state, "param_groups": [self._torch_group(len(self._rest))]})
        order = self._engine_order()
        if order:
            m, v, steps = self._flat_from(order, saved, "engine-stepped")
            self._bound_engine().set_fine_adam_state(m, v, steps.get(0, 0) | (steps.get(1, 0) << 32))
        if self._text:
            le = model.language_encoder
            le._bind_text_train(model.device)
            m, v, steps = self._flat_from([(n, p, 0) for n, p in self._head], saved, "text-head")
            le._th_train_engine.set_text_adam_state(m, v, steps.get(0, 0))
