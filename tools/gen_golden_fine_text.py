"""TEST INFRASTRUCTURE — build-container only (needs the reference tree).

Golden vectors for one training step of the fine stage WITH its text branch: imports the upstream reference through
oracle/ref_harness.py and runs its own ``CrossMatch`` (models/cross_matcher.py:39-129) in embedding mode with 2 decoder layers
under ``model.train()``, every dropout site at p = 0, and the real ``LanguageEncoder(is_fine=True)`` (models/language_encoder.py:76-141)
behind a stub T5 that returns ``synth.make_t5_hidden`` (T5 is frozen by --fixed_embedding and its weights do not exist here).
Weights: ``synth.make_fine_weights`` plus ``synth.make_language_head_weights(embed_dim=128)`` without its inter_module (the fine head
has none). Then ``offset_lambda * nn.MSELoss()`` against seeded targets and ``backward()`` — the body of training/fine.py:38-91.

Writes ``tests/golden/fine_train_text.npz`` (DATA only): seeds and shapes, the hint encodings the text branch produced and
d loss / d hint encodings, offsets, targets and loss, the gradient of every language_encoder head parameter and of a few decoder
parameters (pack_tensor: sampled beyond 1,024 elements, with norm and sum), and inter_mlp's BatchNorm running buffers after the step.
"""
from __future__ import annotations

import os
import os.path as osp
import sys
import tempfile

import numpy as np

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(REPO, "oracle"))
sys.path.insert(0, REPO)
import ref_harness as H  # noqa: E402

H.setup_reference_imports()

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from gen_golden import to_torch_sd  # noqa: E402
from gen_golden_train import pack_tensor  # noqa: E402
from text2loc_amd import synth  # noqa: E402

OUT = osp.join(REPO, "tests", "golden")
torch.set_num_threads(4)
B, NH, PAD, LAMBDA = 8, 6, 16, 5.0  # offset_lambda: training/args.py:29 default
DECODER_GRADS = ("cross_hints.0.self_attn.in_proj_weight", "cross_hints.1.linear2.weight", "cross_objects.0.multihead_attn.out_proj.weight",
                 "cross_objects.1.norm3.weight", "mlp_offsets.0.weight", "mlp_offsets.2.bias")


def run(hf_dir, pn_path, w_seed, h_seed, hidden_seed, c_seed, n_tokens):
    from datapreparation.kitti360pose.utils import COLOR_NAMES, KNOWN_CLASS
    from models.cross_matcher import CrossMatch

    args = H.make_args(hf_dir, pn_path, class_embed=True, color_embed=True, fine_embed_dim=128, fine_num_decoder_heads=4,
                       fine_num_decoder_layers=2, fine_intra_module_num_layers=1, fine_intra_module_num_heads=4,
                       pad_size=PAD, num_mentioned=NH, offset_lambda=LAMBDA)
    torch.manual_seed(0)
    model = CrossMatch(KNOWN_CLASS, COLOR_NAMES, args)
    sd = synth.make_fine_weights(w_seed, num_layers=2)
    sd.update({k: v for k, v in synth.make_language_head_weights(h_seed, embed_dim=128).items() if ".inter_module." not in k})
    missing, unexpected = model.load_state_dict(to_torch_sd(sd), strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(("language_encoder.llm_model.", "object_encoder.pointnet")) for k in missing), missing
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
    hidden = synth.make_t5_hidden(B * NH, n_tokens, seed=hidden_seed)

    class StubT5(nn.Module):
        def forward(self, input_ids=None, attention_mask=None, output_attentions=False):
            from easydict import EasyDict

            assert input_ids.shape[0] == B * NH
            return EasyDict(last_hidden_state=torch.from_numpy(hidden))

    model.language_encoder.llm_model = StubT5()
    cells = synth.make_cells(B, seed=c_seed, with_pn_feat=True, min_obj=PAD, max_obj=PAD)
    objects = [list(o) for o in H.build_objects(cells, seed=c_seed)]
    target = np.random.default_rng([c_seed, 0xF7]).random((B, 2)).astype(np.float32)
    model.train()
    kept = {}

    def keep_hints(mod, i, o):
        o.retain_grad()
        kept["hints"] = o

    h = model.language_encoder.register_forward_hook(keep_hints)
    texts = [" ".join(["The pose is north of a gray pole."] * NH)] * B
    out = model(objects, texts, [None] * B)                              # training/fine.py:48
    h.remove()
    loss = LAMBDA * nn.MSELoss()(out, torch.from_numpy(target))          # :51-53
    loss.backward()                                                      # :55
    res = {"weight_seed": w_seed, "head_seed": h_seed, "hidden_seed": hidden_seed, "cell_seed": c_seed, "batch": B, "n_hints": NH,
           "n_tokens": n_tokens, "n_layers": 2, "offset_lambda": LAMBDA, "hint_encodings": kept["hints"].detach().numpy(),
           "grad_hint": kept["hints"].grad.numpy(), "targets": target, "offsets_out": out.detach().numpy(), "loss": float(loss)}
    params = dict(model.named_parameters())
    used = []
    for n, p in params.items():
        if n.startswith("language_encoder.") and ".llm_model." not in n and p.grad is not None:
            used.append(n)
            pack_tensor(res, "grad", n, p.grad.numpy())
    for n in DECODER_GRADS:
        pack_tensor(res, "grad", n, params[n].grad.numpy())
    res["used_params"] = np.array(used)
    res["decoder_params"] = np.array(DECODER_GRADS)
    for n, b in model.named_buffers():
        if n.startswith("language_encoder.inter_mlp") and "running" in n:
            res["buf/" + n] = b.numpy().copy()
    return res


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="t2l_golden_")
    hf_dir = H.make_tiny_t5(osp.join(tmp, "t5tiny"))
    pn_path = H.make_pointnet_ckpt(osp.join(tmp, "pointnet.pth"))
    # seeds frozen after the split-bf16 twin (tests/fine_text_twin.py, arith = 2) was run against this file on the CPU:
    # tests/test_oracle_fine_text.py keeps that check and records the measured share of entries inside the tolerance
    r = run(hf_dir, pn_path, w_seed=0, h_seed=4, hidden_seed=21, c_seed=40, n_tokens=9)
    np.savez_compressed(osp.join(OUT, "fine_train_text.npz"), **r)
    print("fine_train_text loss", r["loss"], "head params with grad", len(r["used_params"]))


if __name__ == "__main__":
    main()
