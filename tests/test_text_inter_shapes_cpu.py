"""The inter-sentence layer at the compiled shapes other than the published (256, 4 heads), without a GPU:
(a) the numpy restatement against the reference's goldens (tools/gen_golden_text_shapes.py) at (128, 4), (128, 2), (256, 8);
(b) LanguageEncoder._inter_gate: true exactly for the compiled set;
(c) the launch plan (text2loc_amd/csrc/text_inter_plan.h) walked by a stand-alone host program, tests/text_inter_plan_check.cpp, also
    under the host compiler's address + undefined-behaviour sanitizers when it has them."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from text2loc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "text2loc_amd", "csrc")
SHAPES = [(128, 4), (128, 2), (256, 8)]


@pytest.mark.parametrize("D,heads", SHAPES)
def test_restatement_matches_the_reference_golden(golden, D, heads):
    """oracle.t2l_oracle.text_head with the shape's head count vs the reference's encode_text: the CPU tier's text-head bound, 2e-5 on
    unit-norm embeddings (test_host_logic.py)."""
    g = golden(f"text_head_d{D}_h{heads}")
    assert int(g["embed_dim"]) == D and int(g["num_heads"]) == heads
    B, L = int(g["batch"]), int(g["n_tokens"])
    hidden = synth.make_t5_hidden(6 * B, L, seed=int(g["hidden_seed"]))
    sd = synth.make_language_head_weights(int(g["weight_seed"]), embed_dim=D)
    out = O.text_head(hidden, sd, B, 4, heads)
    assert out.shape == g["text_embeddings"].shape == (B, D)
    err = np.abs(out - g["text_embeddings"]).max()
    print(f"restatement vs reference at ({D}, {heads}): {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("D,heads", SHAPES)
def test_pytorch_modules_match_the_reference_golden(golden, D, heads):
    """The port's LanguageEncoder on its PyTorch modules (CPU) reproduces the golden: the modules the engine path is compared with."""
    from text2loc_amd.cell_retrieval import LanguageEncoder

    g = golden(f"text_head_d{D}_h{heads}")
    B, L = int(g["batch"]), int(g["n_tokens"])
    enc = _encoder(D, heads, weight_seed=int(g["weight_seed"]))
    hidden = torch.from_numpy(synth.make_t5_hidden(6 * B, L, seed=int(g["hidden_seed"])))
    t0 = LanguageEncoder.inter_torch_calls
    with torch.no_grad():
        out = torch.nn.functional.normalize(enc.head(hidden, B)).numpy()
    assert LanguageEncoder.inter_torch_calls == t0 + 1  # (no GPU: the gate is never consulted for an engine call)
    assert np.abs(out - g["text_embeddings"]).max() < 2e-5


def _encoder(D, heads, layers=1, is_fine=False, weight_seed=None, **layer_kw):
    from text2loc_amd.cell_retrieval import LanguageEncoder

    enc = LanguageEncoder(D, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=layers, inter_module_num_heads=heads,
                          is_fine=is_fine, llm_model=object(), tokenizer=None, input_dim=1024)
    if layer_kw:
        enc.inter_module[0] = torch.nn.TransformerEncoderLayer(D, heads, dim_feedforward=4 * D, **layer_kw)
    if weight_seed is not None:
        sd = {k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(weight_seed, embed_dim=D).items()}
        missing, unexpected = enc.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
    return enc.eval()


@pytest.mark.parametrize("D,heads", [(256, 4)] + SHAPES)
def test_inter_gate_is_true_for_the_compiled_shapes(D, heads):
    enc = _encoder(D, heads)
    assert all(enc._inter_gate(S) for S in (1, 6, 17, 32))
    assert not enc._inter_gate(0) and not enc._inter_gate(33)


@pytest.mark.parametrize("D,heads", [(128, 8), (256, 2), (64, 2), (192, 6), (192, 3), (128, 1), (256, 16)])
def test_inter_gate_is_false_for_other_widths_and_head_counts(D, heads):
    assert not _encoder(D, heads)._inter_gate(6)


@pytest.mark.parametrize("D,heads", [(128, 4), (256, 4)])
def test_inter_gate_is_false_for_other_layer_flavours(D, heads):
    assert _encoder(D, heads)._inter_gate(6)
    assert not _encoder(D, heads, layers=2)._inter_gate(6)
    assert not _encoder(D, heads, is_fine=True)._inter_gate(6)
    assert not _encoder(D, heads, norm_first=True)._inter_gate(6)
    assert not _encoder(D, heads, activation="gelu")._inter_gate(6)
    wide = _encoder(D, heads)
    wide.inter_module[0] = torch.nn.TransformerEncoderLayer(D, heads, dim_feedforward=2 * D)  # (not the reference's 4 D)
    assert not wide._inter_gate(6)


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    return "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None


@pytest.mark.skipif(_host_compiler() is None, reason="needs a C++17 host compiler")
def test_launch_plan(tmp_path):
    """Every description exactly once, no tile above 32 rows, LDS <= 160 KiB, for n_desc in {0, 1, 2 dpt - 1, 2 dpt, 2 dpt + 1} and S in
    {1, 5, 6, 11, 16, 17, 32} at both widths. A second build with -fsanitize=address,undefined runs too where the host compiler links
    one (a stand-alone program: nothing is loaded into Python)."""
    src = os.path.join(ROOT, "tests", "text_inter_plan_check.cpp")
    base = [_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o"]
    exe = str(tmp_path / "text_inter_plan_check")
    subprocess.run(base + [exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "text_inter_plan_check: ok" in run.stdout
    san = str(tmp_path / "text_inter_plan_check_san")
    built = subprocess.run(base + [san, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if built.returncode == 0:  # (a host compiler without the sanitizer runtimes: the plain run above stands)
        run = subprocess.run([san], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "text_inter_plan_check: ok" in run.stdout
