"""TEST INFRASTRUCTURE — a float64 restatement of the TRAINING step of the fine stage's hint encoder: ``LanguageEncoder(is_fine=True)``
downstream of the frozen T5's hidden states under ``model.train()`` (models/language_encoder.py:127-141): TransformerEncoderLayer(1024,
4 heads, 4096) over the tokens of every hint (:130-134, dropout sites 0-3) -> max over the tokens (:135) -> inter_mlp = Linear(1024 -> D)
+ BatchNorm1d in batch-statistics mode, no ReLU (:137) -> one vector per hint (:138-141 views them [B, n_hints, D]).

Built from the blocks of oracle/t2l_oracle_train.py — ``_layer_fwd`` / ``_layer_bwd`` at layer index 0, ``_bn_fwd`` / ``_bn_bwd`` and
``_Tape.mm`` for the operand arithmetic ``arith`` (oracle/arith.py; the engine's option ``text_train_bf16``) — i.e. the coarse head's
oracle (oracle/t2l_oracle_text_train.py) cut off behind the BatchNorm. tests/test_oracle_fine_text.py pins it to the imported
reference's own step (tests/golden/fine_train_text.npz) and to central differences of its own forward.
"""
from __future__ import annotations

import numpy as np

from oracle import t2l_oracle_train as OT
from text2loc_amd import synth

P = "language_encoder."


def fine_head_weights(seed: int, embed_dim: int = 128) -> dict:
    """state_dict (numpy) of the fine head: ``synth.make_language_head_weights`` without the inter_module it does not have."""
    return {k: v for k, v in synth.make_language_head_weights(seed, embed_dim=embed_dim).items() if ".inter_module." not in k}


def fine_text_head_train(hidden: np.ndarray, sd: dict, grad_out=None, p_drop: float = 0.0, seed: int = 0, dtype=np.float64,
                         prefix: str = P, arith=0):
    """hidden [n_sent, L, 1024] -> (out [n_sent, D], info). With ``grad_out`` [n_sent, D]: info["grads"][name] = dLoss/dparameter;
    info["bn_stats"]["<prefix>inter_mlp.0.1"] = (mean, biased var, n) always."""
    t = OT._Tape(sd, dtype, arith)
    w = t.w
    x = np.asarray(hidden).astype(dtype)
    x2, c1 = OT._layer_fwd(t, x, prefix + "intra_module.0", 4, p_drop, seed, 0)
    tok_arg = x2.argmax(axis=1)  # first maximal token wins, as torch.max
    pooled = np.take_along_axis(x2, tok_arg[:, None, :], axis=1)[:, 0]
    mp = prefix + "inter_mlp.0"
    y = t.mm(pooled, w[mp + ".0.weight"].T) + w[mp + ".0.bias"]
    z, bc = OT._bn_fwd(y, w[mp + ".1.weight"], w[mp + ".1.bias"])
    t.bn_stats[mp + ".1"] = (bc[2], bc[3], y.shape[0])
    info = {"pooled": pooled, "bn_stats": t.bn_stats}
    if grad_out is None:
        return z, info
    dz = np.asarray(grad_out).astype(dtype).reshape(z.shape)
    dy, dg, db = OT._bn_bwd(dz, w[mp + ".1.weight"], bc)
    t.add(mp + ".1.weight", dg)
    t.add(mp + ".1.bias", db)
    t.add(mp + ".0.weight", t.mm(dy.T, pooled))
    t.add(mp + ".0.bias", dy.sum(0))
    dpooled = t.mm(dy, w[mp + ".0.weight"])
    dx2 = np.zeros_like(x2)
    np.put_along_axis(dx2, tok_arg[:, None, :], dpooled[:, None, :], axis=1)
    OT._layer_bwd(t, dx2, prefix + "intra_module.0", 4, c1)
    info["grads"] = t.grads
    return z, info
