"""TEST INFRASTRUCTURE — build-container only (needs the reference tree).

Golden vectors for the text head at the (coarse_embed_dim, inter_module_num_heads) pairs other than the published (256, 4) that
``t2l_text_inter`` is compiled for: imports the upstream reference through oracle/ref_harness.py
(``make_args(coarse_embed_dim=D, inter_module_num_heads=h)``), loads ``synth.make_language_head_weights(seed, embed_dim=D)`` (and
the matching object branch) into its own ``CellRetrievalNetwork``, puts ``synth.make_t5_hidden(6 B, L, seed)`` in place of T5's
output (the ``StubT5`` of oracle/gen_golden.py) and calls ``encode_text`` in eval mode.

Writes DATA only under tests/golden/ (seeds, shape integers, ``text_embeddings`` [B, D]):

    text_head_d128_h4.npz   (128, 4 heads)   what --coarse_embed_dim 128 builds
    text_head_d128_h2.npz   (128, 2 heads)
    text_head_d256_h8.npz   (256, 8 heads)
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

from gen_golden import to_torch_sd  # noqa: E402
from text2loc_amd import synth  # noqa: E402

OUT = osp.join(REPO, "tests", "golden")
torch.set_num_threads(4)
B, L, W_SEED, H_SEED = 5, 9, 1, 4
GOLDENS = {"text_head_d128_h4": (128, 4), "text_head_d128_h2": (128, 2), "text_head_d256_h8": (256, 8)}


def text_golden(name, hf_dir, pn_path):
    from datapreparation.kitti360pose.utils import COLOR_NAMES, KNOWN_CLASS
    from models.cell_retrieval import CellRetrievalNetwork

    D, heads = GOLDENS[name]
    args = H.make_args(hf_dir, pn_path, class_embed=True, color_embed=True, coarse_embed_dim=D, inter_module_num_heads=heads)
    model = CellRetrievalNetwork(KNOWN_CLASS, COLOR_NAMES, args)
    sd = synth.make_object_branch_weights(W_SEED, embed_dim=D)
    sd.update(synth.make_language_head_weights(W_SEED, embed_dim=D))
    missing, unexpected = model.load_state_dict(to_torch_sd(sd), strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(("language_encoder.llm_model", "object_encoder.pointnet")) for k in missing), missing
    model.eval()
    layer = model.language_encoder.inter_module[0]
    assert len(model.language_encoder.inter_module) == 1 and layer.self_attn.num_heads == heads and layer.linear1.out_features == 4 * D
    hidden = synth.make_t5_hidden(6 * B, L, seed=H_SEED)

    class StubT5(torch.nn.Module):
        def forward(self, input_ids=None, attention_mask=None, output_attentions=False):
            from easydict import EasyDict

            assert input_ids.shape[0] == 6 * B
            return EasyDict(last_hidden_state=torch.from_numpy(hidden))

    model.language_encoder.llm_model = StubT5()
    texts = [" ".join(["The pose is north of a gray pole."] * 6)] * B
    with torch.no_grad():
        out = model.encode_text(texts)
    assert out.shape == (B, D)
    np.savez_compressed(osp.join(OUT, name + ".npz"), weight_seed=W_SEED, hidden_seed=H_SEED, batch=B, n_tokens=L, embed_dim=D,
                        num_heads=heads, text_embeddings=out.numpy())
    print(name, out.shape, osp.getsize(osp.join(OUT, name + ".npz")))


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="t2l_golden_text_shapes_")
    hf_dir = H.make_tiny_t5(osp.join(tmp, "t5tiny"))
    pn_path = H.make_pointnet_ckpt(osp.join(tmp, "pointnet.pth"))
    for name in GOLDENS:
        text_golden(name, hf_dir, pn_path)


if __name__ == "__main__":
    main()
