"""TEST INFRASTRUCTURE — float64 oracle of the PointNet++ object backbone in TRAINING mode: forward with batch-statistics
BatchNorm, analytic backward, running-statistics update (SURVEY.md §8 rows a3 + a9).

PARITY UNPINNED, like the eval-mode restatement it extends (oracle/t2l_oracle_pointnet.py: FPS start / tie rule, ball query,
PyG's bipartite self-loop edge are this build's reading of absent third-party packages). What the reference's own code fixes
and this module follows:

* the backbone is called ONCE PER CELL (models/object_encoder.py:92-95: ``[self.pointnet(pyg_batch) for pyg_batch in
  object_points]``), so under ``model.train()`` every BatchNorm1d of it normalises with the statistics of THAT cell's rows
  (the edges of all its objects for the SetAbstraction MLPs, its objects' 32 remaining points for the global MLP) and updates
  its running statistics once per cell, in cell order (momentum 0.1, unbiased variance);
* structure: models/pointcloud/pointnet2.py:18-100 — SA(0.5, r) x3 with get_mlp([cin+3, h1, h2]) (Linear, BatchNorm, ReLU
  twice), max aggregation; global MLP on cat[x, pos] + max over the points; lin1 / lin2 with ReLU; ``features2`` is consumed.

The index structure (FPS order, neighbour lists, the extra self-loop source) comes from the eval oracle's own functions, so
both oracles see identical edges. Gradients: d loss / d every ``object_encoder.pointnet.*`` parameter the path uses, given
d loss / d features2 (the classifier heads are not on the path: object_encoder.py:60-61 uses features2).
Checked against central differences of its own forward in tests/test_oracle_train.py.

Reduced-precision arithmetic (``arith``, oracle/arith.py; the engine's option ``train_bf16``, text2loc_amd/csrc/pointnet_train.h):
every product of the path runs on a bf16-capable GEMM and takes the operand arithmetic here —
* edge MLPs: rows2_kernel (gemm_rows2.h:118-306, operands converted in rows2_fill / step) for y1 = X W1^T and y2 = a1 W2^T
  (pn_block_fwd, pointnet_train.h:858, 1078-1079), dA1 = dA2 W2 (:1152) and the input gradient dA1 W1 (:1168 / :1174); tn2_kernel
  (gemm_rows2.h:330-490, conversion at :420-443) for dW2 = dA2^T a1 (:1147) and dW1 = dA1^T X (:1156);
* lin1 / lin2: gemm_f32.h (gemm_nt :1094-1095, gemm_tn / gemm_nn :1134-1138).
In mode 1 the edge-row tensors are also STORED as bf16, rounded once when written (gemm_rows2.h:26-32, pn_store_t; ``store`` here):
X (pt_gather_kernel), y1, y2, a1 (stored at the global level, rebuilt from the stored y1 and rounded as an operand at the SA levels —
the same value), dA2 and dA1 (each the gradient w.r.t. the Linear output after the BatchNorm backward) and the global level's input
gradient. The BatchNorm statistics of the forward come from the float32 accumulators BEFORE the rounding (rows2_kernel's epilogue,
gemm_rows2.h:252, 277-299); everything after them — normalisation, ReLU, the first-maximum arg-max of a group, the BatchNorm
backward's sums and closed form — reads the rounded values. Float32 (exact here): the SA levels' input gradient (scattered by
rows2_kernel's epilogue), the per-group tensors (xout, arg, ysel, dxout), lin1 / lin2 activations, the bias gradients (column sums of
the stored dY).
"""
from __future__ import annotations

import numpy as np

from . import arith as A
from . import t2l_oracle_pointnet as OP

BN_EPS = 1e-5
MOMENTUM = 0.1
P = "object_encoder.pointnet."


def _bn_train(h, gamma, beta, hs):
    """Statistics of h; the normalisation reads hs (h as stored: bf16 in mode 1)."""
    n = h.shape[0]
    mean = h.mean(axis=0)
    var = h.var(axis=0)  # biased
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (hs - mean) * rstd
    return xhat * gamma + beta, (xhat, rstd, n, mean, var)


def _bn_bwd(dy, cache, gamma):
    xhat, rstd, n, _, _ = cache
    dgamma = (dy * xhat).sum(axis=0)
    dbeta = dy.sum(axis=0)
    dxhat = dy * gamma
    dx = rstd * (dxhat - dxhat.mean(axis=0) - xhat * (dxhat * xhat).mean(axis=0))
    return dx, dgamma, dbeta


class _Mlp:
    """get_mlp([cin, h1, h2]) in training mode over ONE BatchNorm domain (the rows of one cell)."""

    def __init__(self, sd, prefix, arith=0):
        self.prefix = prefix
        self.arith = arith
        self.w = [sd[f"{prefix}.{i}.0.weight"].astype(np.float64) for i in range(2)]
        self.b = [sd[f"{prefix}.{i}.0.bias"].astype(np.float64) for i in range(2)]
        self.g = [sd[f"{prefix}.{i}.1.weight"].astype(np.float64) for i in range(2)]
        self.be = [sd[f"{prefix}.{i}.1.bias"].astype(np.float64) for i in range(2)]

    def forward(self, x):
        cache = []
        for i in range(2):
            h = A.product(x, self.w[i].T, self.arith) + self.b[i]
            y, bn = _bn_train(h, self.g[i], self.be[i], A.store(h, self.arith))
            a = np.maximum(y, 0.0)
            cache.append((x, bn, a))
            x = a
        return x, cache

    def backward(self, da, cache, grads, need_dx=True, store_dx=False):
        """store_dx: the input gradient is an edge-row tensor too (the global level's; the SA levels scatter theirs in float32)."""
        for i in (1, 0):
            x, bn, a = cache[i]
            dy = da * (a > 0)
            dh, dg, db = _bn_bwd(dy, bn, self.g[i])
            dh = A.store(dh, self.arith)
            grads[f"{self.prefix}.{i}.1.weight"] = grads.get(f"{self.prefix}.{i}.1.weight", 0) + dg
            grads[f"{self.prefix}.{i}.1.bias"] = grads.get(f"{self.prefix}.{i}.1.bias", 0) + db
            grads[f"{self.prefix}.{i}.0.weight"] = grads.get(f"{self.prefix}.{i}.0.weight", 0) + A.product(dh.T, x, self.arith)
            grads[f"{self.prefix}.{i}.0.bias"] = grads.get(f"{self.prefix}.{i}.0.bias", 0) + dh.sum(axis=0)
            da = A.product(dh, self.w[i], self.arith) if (need_dx or i == 1) else None
            if i == 1 or store_dx:
                da = A.store(da, self.arith)
        return da


def build_edges(pos, cell_offsets, pyg_self_loops=True):
    """Index structure of the three SetAbstraction levels (shared by forward and backward): per level
    (sel [n_obj, nd], per object the list over centres of source-row indices into the CELL's flattened source array)."""
    n_obj = pos.shape[0]
    cur_pos = pos.astype(np.float32)
    levels = []
    for radius, _ in OP.LEVELS:
        ns = cur_pos.shape[1]
        nd = (ns + 1) // 2
        sel = np.zeros((n_obj, nd), dtype=np.int64)
        new_pos = np.zeros((n_obj, nd, 3), dtype=np.float32)
        src = [[None] * nd for _ in range(n_obj)]
        for c in range(len(cell_offsets) - 1):
            lo, hi = int(cell_offsets[c]), int(cell_offsets[c + 1])
            for o in range(lo, hi):
                sel[o] = OP.fps(cur_pos[o], nd)
                new_pos[o] = cur_pos[o][sel[o]]
                for t in range(nd):
                    nb = OP.ball_query(cur_pos[o], new_pos[o, t], radius) + (o - lo) * ns  # rows of the cell's source array
                    if pyg_self_loops:
                        nb = np.concatenate([nb, [(o - lo) * nd + t]])
                    src[o][t] = nb
        levels.append((sel, src, cur_pos, new_pos))
        cur_pos = new_pos
    return levels


def forward_backward(pos, rgb, cell_offsets, sd, grad_f2=None, pyg_self_loops=True, arith=0):
    """pos, rgb f32[n_obj,256,3]. Returns (features2 f64[n_obj,256], info) with info["grads"] (when grad_f2 is given),
    info["running"] = name -> value after the per-cell sequential updates, info["features0"]. ``arith``: module docstring."""
    sd64 = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    n_obj = pos.shape[0]
    n_cells = len(cell_offsets) - 1
    levels = build_edges(pos, cell_offsets, pyg_self_loops)
    running = {k: v.copy() for k, v in sd64.items() if k.startswith(P) and "running_" in k}

    def update_running(prefix, caches):  # caches: the two BatchNorm caches of one cell's call
        for i in range(2):
            _, _, n, mean, var = caches[i][1]
            running[f"{prefix}.{i}.1.running_mean"] = (1 - MOMENTUM) * running[f"{prefix}.{i}.1.running_mean"] + MOMENTUM * mean
            running[f"{prefix}.{i}.1.running_var"] = (1 - MOMENTUM) * running[f"{prefix}.{i}.1.running_var"] + MOMENTUM * var * n / max(n - 1, 1)

    x_levels = [rgb.astype(np.float64)]
    fwd = []  # per level, per cell: (mlp cache, row -> (object, centre), argmax rows)
    for li, (radius, name) in enumerate(OP.LEVELS):
        sel, src, src_pos, new_pos = levels[li]
        mlp = _Mlp(sd64, f"{P}{name}.point_conv.local_nn", arith)
        x_prev = x_levels[-1]
        nd = sel.shape[1]
        h2 = mlp.w[1].shape[0]
        new_x = np.zeros((n_obj, nd, h2))
        per_cell = []
        for c in range(n_cells):
            lo, hi = int(cell_offsets[c]), int(cell_offsets[c + 1])
            xs = x_prev[lo:hi].reshape(-1, x_prev.shape[2])
            ps = src_pos[lo:hi].reshape(-1, 3).astype(np.float64)
            rows_src, rows_ctr = [], []
            for o in range(lo, hi):
                for t in range(nd):
                    rows_src.extend(src[o][t].tolist())
                    rows_ctr.extend([(o, t)] * len(src[o][t]))
            rows_src = np.array(rows_src, dtype=np.int64)
            ctr = np.array(rows_ctr, dtype=np.int64)
            xin = A.store(np.concatenate([xs[rows_src], ps[rows_src] - new_pos[ctr[:, 0], ctr[:, 1]].astype(np.float64)], axis=1), arith)
            a, cache = mlp.forward(xin)
            update_running(mlp.prefix, cache)
            amax = {}
            start = 0
            for o in range(lo, hi):
                for t in range(nd):
                    k = len(src[o][t])
                    blk = a[start:start + k]
                    arg = blk.argmax(axis=0)  # first maximum
                    new_x[o, t] = blk[arg, np.arange(h2)]
                    amax[(o, t)] = start + arg
                    start += k
            per_cell.append((cache, rows_src, amax, lo, hi))
        fwd.append((mlp, per_cell))
        x_levels.append(new_x)
    # global abstraction, per cell
    ga = _Mlp(sd64, P + "ga.mlp", arith)
    pos3 = levels[-1][3].astype(np.float64)
    x3 = x_levels[-1]
    f0 = np.zeros((n_obj, ga.w[1].shape[0]))
    ga_cells = []
    for c in range(n_cells):
        lo, hi = int(cell_offsets[c]), int(cell_offsets[c + 1])
        xin = A.store(np.concatenate([x3[lo:hi], pos3[lo:hi]], axis=2).reshape(-1, x3.shape[2] + 3), arith)
        a, cache = ga.forward(xin)
        update_running(ga.prefix, cache)
        a3 = a.reshape(hi - lo, pos3.shape[1], -1)
        arg = a3.argmax(axis=1)
        f0[lo:hi] = np.take_along_axis(a3, arg[:, None, :], axis=1)[:, 0, :]
        ga_cells.append((cache, arg, lo, hi))
    w1, b1 = sd64[P + "lin1.weight"], sd64[P + "lin1.bias"]
    w2, b2 = sd64[P + "lin2.weight"], sd64[P + "lin2.bias"]
    f1 = np.maximum(A.product(f0, w1.T, arith) + b1, 0.0)
    f2 = np.maximum(A.product(f1, w2.T, arith) + b2, 0.0)
    info = {"running": running, "features0": f0, "features1": f1}
    if grad_f2 is None:
        return f2, info

    grads = {}
    d2 = np.asarray(grad_f2, dtype=np.float64) * (f2 > 0)
    grads[P + "lin2.weight"], grads[P + "lin2.bias"] = A.product(d2.T, f1, arith), d2.sum(axis=0)
    d1 = A.product(d2, w2, arith) * (f1 > 0)
    grads[P + "lin1.weight"], grads[P + "lin1.bias"] = A.product(d1.T, f0, arith), d1.sum(axis=0)
    df0 = A.product(d1, w1, arith)
    dx = np.zeros_like(x3)
    for cache, arg, lo, hi in ga_cells:
        npts = pos3.shape[1]
        da = np.zeros((hi - lo, npts, f0.shape[1]))
        np.put_along_axis(da, arg[:, None, :], df0[lo:hi][:, None, :], axis=1)
        dxin = ga.backward(da.reshape(-1, f0.shape[1]), cache, grads, store_dx=True)
        dx[lo:hi] = dxin.reshape(hi - lo, npts, -1)[:, :, : x3.shape[2]]
    for li in (2, 1, 0):
        mlp, per_cell = fwd[li]
        x_prev = x_levels[li]
        dprev = np.zeros_like(x_prev)
        h2 = mlp.w[1].shape[0]
        for cache, rows_src, amax, lo, hi in per_cell:
            n_rows = cache[1][2].shape[0]
            da = np.zeros((n_rows, h2))
            for (o, t), rows in amax.items():
                np.add.at(da, (rows, np.arange(h2)), dx[o, t])
            dxin = mlp.backward(da, cache, grads, need_dx=li > 0)
            if li > 0:
                flat = dprev[lo:hi].reshape(-1, x_prev.shape[2])
                np.add.at(flat, rows_src, dxin[:, : x_prev.shape[2]])
                dprev[lo:hi] = flat.reshape(hi - lo, x_prev.shape[1], -1)
        dx = dprev
    info["grads"] = grads
    return f2, info
