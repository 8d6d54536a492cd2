"""TEST INFRASTRUCTURE — float64 reference, derived bounds and the committed cases of the backbone's pretraining step
(tests/test_pointnet_pretrain_cpu.py, tests/test_gpu_pointnet_pretrain.py, tests/test_gpu_pointnet_cls_safety.py).

The step: two Linear(256, C) heads over features2 and the softmax cross-entropy of each (models/pointcloud/pointnet2.py:64-65,
91-92; the plain definition of the loss). numpy only, never the product. U = 2^-24 (one float32 rounding), as tests/train_blocks.py.

Bounds, in the order the kernel computes (x = features2 [n,256], l = logits, C = classes of a head, y = one-hot label):

  logits.   tol_l[r,c] = (256 + 2) U (sum_k |x_rk||W_ck| + |b_c|): the first-order worst case of ANY summation order of the 256
            products plus the bias add (what the issue states).  d_r = max_c tol_l[r,c] over BOTH heads' columns of row r.

  loss.     CE_r = logsumexp(l_r) - l_r[label].  Lipschitz step: the gradient of logsumexp is the softmax, whose entries are >= 0
            and sum to 1, so |logsumexp(l + e) - logsumexp(l)| <= max_c |e_c|; the label term adds another max_c |e_c|:
                |CE_r(l~) - CE_r(l)| <= 2 d_r.
            Evaluating it in float32 at the perturbed logits, with R_r = max_c (max l_r - l_rc) + 2 d_r the range of the exponents:
            l - m rounds once (<= U R_r absolute, i.e. relative on its exponential), expf is good to 2 U relative, the C-term sum
            adds (C - 1) U, logf 2 U |log z| + its argument's relative error with 0 <= log z <= log C, and (m - l[label]) and the
            final add one rounding each of magnitudes <= R_r and <= log C + R_r:
                eval_r = U (C + 1 + R_r + 2 log C + R_r + log C + R_r) = U (C + 1 + 3 log C + 3 R_r).
            tol_CE_r = 2 (2 d_r + eval_r) (the 2: second order, as train_blocks' FACTOR).  The mean runs in float64; 1/n is a float32
            and the result rounds to float32 once:  tol_loss = mean_r tol_CE_r + 3 U |loss|.

  G.        G_rc = w (p_rc - y_rc) / n,  p = softmax.  d log p_c / d l = y_c - p, of 1-norm <= 2, so to first order
            |p~_c - p_c| <= 2 d_r p_c.  In float32: the exponential carries (R_r + 2) U relative, 1 / z the sum's (C - 1 + R_r + 2) U
            plus one rounding, their product one more: (C + 2 R_r + 5) U relative on p_c; then the subtraction, w / n (two roundings)
            and the product: 4 U |p_c - y_c|:
                tol_G[r,c] = 2 (|w| / n) (p_rc (2 d_r + (C + 2 R_r + 5) U) + 4 U |p_rc - y_rc|).

  d x.      dx_rk = sum_c G_rc W_ck over the kernel's 64 column slots:  tol = sum_c tol_G[r,c] |W_ck| + 2 (64 + 2) U sum_c |G_rc||W_ck|.
  dW, db.   dW_ck = sum_r G_rc x_rk (rows of a workgroup in registers, workgroups through float atomics: n + 8 roundings cover both):
            tol = sum_r tol_G[r,c] |x_rk| + 2 (n + 8) U sum_r |G_rc||x_rk|;  db likewise with x = 1.

  counts.   The kernel's arg-max equals float64's whenever the top-two gap of the row exceeds 2 d_r; the committed cases keep every
            row's gap above 100 d_r (``heads_case`` asserts nothing: tests/test_pointnet_pretrain_cpu.py does, for every case).
"""
import functools

import numpy as np

from text2loc_amd import synth

U = 2.0 ** -24
P = "object_encoder.pointnet."
HEADS = ("class_classifier", "color_classifier")
ROWS_PER_WG = 32  # pointnet_cls.hip: kClsRows
# n: one row | a partial workgroup | two whole workgroups and a ragged third (2 * 32 + 6)
HEAD_ROWS = (1, 5, 70)
HEAD_CLASSES = ((22, 8), (2, 32))
# seed of every (n, (C1, C2)) case: the first for which every row's top-two gap exceeds 100 x its logit bound (searched on the
# float64 reference alone, tests/test_pointnet_pretrain_cpu.py asserts it)
HEAD_SEEDS = {(1, (22, 8)): 0, (5, (22, 8)): 1, (70, (22, 8)): 3, (1, (2, 32)): 0, (5, (2, 32)): 0, (70, (2, 32)): 20}
W_CLASS, W_COLOR = 1.0, 0.5  # (unequal, so that a swapped weight shows)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def heads_forward(x, sd, class_labels, color_labels):
    """float64: per head (logits [n,C], softmax p, CE per row, first arg-max)."""
    x = f64(x)
    out = []
    for name, lab in zip(HEADS, (class_labels, color_labels)):
        W, b = f64(sd[P + name + ".weight"]), f64(sd[P + name + ".bias"])
        l = x @ W.T + b
        m = l.max(axis=1, keepdims=True)
        e = np.exp(l - m)
        z = e.sum(axis=1, keepdims=True)
        ce = (np.log(z) + m)[:, 0] - l[np.arange(len(l)), lab]
        out.append(dict(W=W, b=b, logits=l, p=e / z, ce=ce, argmax=l.argmax(axis=1), labels=np.asarray(lab)))
    return out


def heads_ref(x, sd, class_labels, color_labels, w_class=W_CLASS, w_color=W_COLOR):
    """float64 reference of t2l_pointnet_cls_heads: dict(logits [n,C1+C2], loss [2], correct [2], dx [n,256], grads name -> array,
    G per head, heads = heads_forward's list)."""
    x = f64(x)
    n = len(x)
    heads = heads_forward(x, sd, class_labels, color_labels)
    dx = np.zeros_like(x)
    grads, Gs = {}, []
    for h, w, name in zip(heads, (w_class, w_color), HEADS):
        y = np.zeros_like(h["p"])
        y[np.arange(n), h["labels"]] = 1.0
        G = w * (h["p"] - y) / n
        Gs.append(G)
        dx += G @ h["W"]
        grads[P + name + ".weight"] = G.T @ x
        grads[P + name + ".bias"] = G.sum(axis=0)
    return dict(logits=np.concatenate([h["logits"] for h in heads], axis=1), loss=np.array([h["ce"].mean() for h in heads]),
                correct=np.array([(h["argmax"] == h["labels"]).sum() for h in heads]), dx=dx, grads=grads, G=Gs, heads=heads)


def heads_bounds(x, ref, w_class=W_CLASS, w_color=W_COLOR):
    """The module docstring's bounds for ``ref = heads_ref(x, ...)``: dict(logits, loss [2], dx, grads name -> array, d [n], gap [n,2])."""
    x = np.abs(f64(x))
    n = len(x)
    heads = ref["heads"]
    tol_l = [(256 + 2) * U * (x @ np.abs(h["W"]).T + np.abs(h["b"])) for h in heads]
    d = np.maximum(tol_l[0].max(axis=1), tol_l[1].max(axis=1))
    tol_loss, tol_dx, tol_g, gaps = [], np.zeros_like(x), {}, []
    for h, w, name, G in zip(heads, (w_class, w_color), HEADS, ref["G"]):
        C = h["logits"].shape[1]
        R = (h["logits"].max(axis=1, keepdims=True) - h["logits"]).max(axis=1) + 2 * d
        ev = U * (C + 1 + 3 * np.log(C) + 3 * R)
        tol_ce = 2 * (2 * d + ev)
        tol_loss.append(tol_ce.mean() + 3 * U * abs(h["ce"].mean()))
        y = np.zeros_like(h["p"])
        y[np.arange(n), h["labels"]] = 1.0
        tol_G = 2 * abs(w) / n * (h["p"] * (2 * d + (C + 2 * R + 5) * U)[:, None] + 4 * U * np.abs(h["p"] - y))
        aW, aG = np.abs(h["W"]), np.abs(G)
        tol_dx += tol_G @ aW + 2 * (64 + 2) * U * (aG @ aW)
        tol_g[P + name + ".weight"] = tol_G.T @ x + 2 * (n + 8) * U * (aG.T @ x)
        tol_g[P + name + ".bias"] = tol_G.sum(axis=0) + 2 * (n + 8) * U * aG.sum(axis=0)
        top = np.sort(h["logits"], axis=1)
        gaps.append(top[:, -1] - top[:, -2])
    return dict(logits=np.concatenate(tol_l, axis=1), loss=np.array(tol_loss), dx=tol_dx, grads=tol_g, d=d, gap=np.stack(gaps, axis=1))


def make_heads_inputs(n, classes, seed):
    """features2 = |N(0,1)| (post-ReLU-like, float32), head weights from synth.make_pointnet_weights, uniform labels."""
    c1, c2 = classes
    rng = np.random.default_rng([seed, n, c1, c2])
    x = np.abs(rng.standard_normal((n, 256))).astype(np.float32)
    sd = synth.make_pointnet_weights(seed, n_classes=c1, n_colors=c2)
    return x, sd, rng.integers(0, c1, n).astype(np.int32), rng.integers(0, c2, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def heads_case(n, classes):
    """(x f32[n,256], sd, class_labels, color_labels, ref, bounds) of a committed case: computed once, shared, never modified."""
    x, sd, lc, lk = make_heads_inputs(n, classes, HEAD_SEEDS[(n, classes)])
    ref = heads_ref(x, sd, lc, lk)
    return x, sd, lc, lk, ref, heads_bounds(x, ref)


def gaps_hold(n, classes, seed):
    x, sd, lc, lk = make_heads_inputs(n, classes, seed)
    b = heads_bounds(x, heads_ref(x, sd, lc, lk))
    return bool((b["gap"] > 100 * b["d"][:, None]).all())


# ---- the short trajectory ----------------------------------------------------------------------------------------------------------
TRAJ_OBJECTS, TRAJ_STEPS, TRAJ_LR, TRAJ_SEED = 4, 3, 1e-3, 0


def make_trajectory_inputs(seed=TRAJ_SEED, n_obj=TRAJ_OBJECTS):
    """(pos, rgb f32[n,256,3], sd numpy, class_labels, color_labels) of the trajectory case: one segment of n_obj objects."""
    cells = synth.make_cells(1, seed=seed + 40, min_obj=n_obj, max_obj=n_obj)
    pos, rgb = synth.make_sampled_points(cells, seed + 41)
    sd = synth.make_pointnet_weights(seed + 42)
    rng = np.random.default_rng([seed, 0xC15])
    return pos, rgb, sd, rng.integers(0, 22, n_obj).astype(np.int32), rng.integers(0, 8, n_obj).astype(np.int32)


def step_ref(pos, rgb, sd, class_labels, color_labels, w_class=1.0, w_color=1.0, backward=True):
    """One float64 forward (+ backward) of the whole step, the batch as ONE segment: (features2, heads_ref dict, backbone info)."""
    from oracle import t2l_oracle_pointnet_train as OPT

    offs = np.array([0, len(pos)], dtype=np.int32)
    f2, info = OPT.forward_backward(pos, rgb, offs, sd)
    ref = heads_ref(f2, sd, class_labels, color_labels, w_class, w_color)
    if backward:
        _, info = OPT.forward_backward(pos, rgb, offs, sd, grad_f2=ref["dx"])
    return f2, ref, info


def trajectory_ref(steps=TRAJ_STEPS, lr=TRAJ_LR, seed=TRAJ_SEED, n_obj=TRAJ_OBJECTS):
    """The weighted loss before each of ``steps`` float64 Adam steps (oracle.t2l_oracle_train.adam_step) on one fixed batch, and the
    loss after the last: ``steps + 1`` values. Running statistics move as the training-mode forward moves them."""
    from oracle import t2l_oracle_train as OT

    pos, rgb, sd, lc, lk = make_trajectory_inputs(seed, n_obj)
    sd = {k: f64(v) if np.asarray(v).dtype.kind == "f" else v for k, v in sd.items()}
    m, v, losses = {}, {}, []
    for step in range(1, steps + 2):
        last = step == steps + 1
        _, ref, info = step_ref(pos, rgb, sd, lc, lk, backward=not last)
        losses.append(float(ref["loss"].sum()))
        if last:
            break
        grads = dict(info["grads"])
        grads.update(ref["grads"])
        for k, g in grads.items():
            sd[k], m[k], v[k] = OT.adam_step(sd[k], g, m.get(k, 0.0), v.get(k, 0.0), step, lr)
        sd.update(info["running"])
    return losses
