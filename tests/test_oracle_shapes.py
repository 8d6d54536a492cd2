"""CPU tier: the cell encoder at shapes other than the published one (coarse_embed_dim, head count, layer count, object_size).

* the numpy oracle, unchanged, reproduces the reference goldens of tools/gen_golden_shapes.py within the bars
  test_oracle_golden.py holds it to for encoder_embed (object_features 2e-5, cell_embeddings 1e-5);
* ``CellRetrievalNetwork`` accepts every compiled shape and refuses the rest with a message that names the compiled set.
"""
import types

import numpy as np
import pytest
import torch

from oracle import t2l_oracle as O
from text2loc_amd import synth

ENCODER_GOLDENS = ("shapes_d128_h4", "shapes_d128_h2_l3_s20", "shapes_d256_h8_l1_s32", "shapes_d256_s24")


def golden_cells(g, with_pn=False):
    cells = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    if with_pn:  # the features2 table regenerates from the seed, as for encoder_pn.npz
        cells["pn_feat"] = synth.make_cells(int(g["n_cells"]), seed=int(g["cell_seed"]), with_pn_feat=True)["pn_feat"]
    return cells


def golden_cases(g):
    """(mode, field suffix) of every mode a golden holds."""
    modes = [str(m) for m in g["modes"]]
    return [(m, "_pn" if (m == "pn" and len(modes) > 1) else "") for m in modes]


def golden_shape(g):
    return int(g["embed_dim"]), int(g["num_heads"]), int(g["num_layers"]), int(g["object_size"])


@pytest.mark.parametrize("name", ENCODER_GOLDENS)
def test_oracle_reproduces_the_shape_goldens(golden, name):
    g = golden(name)
    D, heads, layers, osz = golden_shape(g)
    counts = g["in_counts"]
    assert counts.max() > osz and counts.min() < osz, "the golden must cut one cell and pad another"
    sd = synth.make_object_branch_weights(int(g["weight_seed"]), embed_dim=D, num_layers=layers)
    for mode, sfx in golden_cases(g):
        embed = mode == "embed"
        cells = golden_cells(g, with_pn=not embed)
        emb, feats, _ = O.encode_cells(cells, sd, embed, embed, object_size=osz, n_heads=heads, n_layers=layers, return_stages=True)
        assert emb.shape == (len(counts), D)
        e_feat = np.abs(feats - g["object_features" + sfx]).max()
        e_emb = np.abs(emb - g["cell_embeddings" + sfx]).max()
        print(f"{name} {mode}: object_features {e_feat:.2e} cell_embeddings {e_emb:.2e}")
        assert e_feat < 2e-5
        assert e_emb < 1e-5


def test_e2e_golden_is_the_d128_model(golden):
    g = golden("retrieval_e2e_d128")
    assert g["cell_encodings"].shape == (64, 128) and g["text_encodings"].shape == (64, 128)
    sd = synth.make_object_branch_weights(int(g["weight_seed"]), embed_dim=128, num_layers=int(g["num_layers"]))
    cells = golden_cells(g)
    emb = O.encode_cells(cells, sd, True, True, object_size=int(g["object_size"]), n_heads=int(g["num_heads"]),
                         n_layers=int(g["num_layers"]))
    assert np.abs(emb - g["cell_encodings"]).max() < 1e-5


def make_args(**over):
    a = dict(coarse_embed_dim=256, object_size=28, object_inter_module_num_heads=4, object_inter_module_num_layers=2,
             use_features=["class", "color", "position", "num"], class_embed=True, color_embed=True, hungging_model=None,
             fixed_embedding=True, intra_module_num_layers=1, intra_module_num_heads=4, inter_module_num_layers=1,
             inter_module_num_heads=4)
    a.update(over)
    return types.SimpleNamespace(**a)


class NoText(torch.nn.Module):
    """Stands in for the T5 text branch: the constructor under test is the object branch's."""


def build(**over):
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    return CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, make_args(**over), language_encoder=NoText())


@pytest.mark.parametrize("D,heads,layers,osz", [(128, 4, 2, 28), (128, 2, 3, 20), (256, 8, 1, 32), (256, 4, 2, 24), (128, 4, 4, 1),
                                                (256, 4, 2, 28)])
def test_every_compiled_shape_constructs(D, heads, layers, osz):
    m = build(coarse_embed_dim=D, object_size=osz, object_inter_module_num_heads=heads, object_inter_module_num_layers=layers)
    assert m.embed_dim == D and m.object_size == osz and len(m.obj_inter_module) == layers
    assert m.obj_inter_module[0].linear1.out_features == 2 * D
    assert m.object_encoder.mlp_pointnet[0][0].in_features == 256  # features2 stays 256 wide at every D
    assert m.published_shape == ((D, heads, osz) == (256, 4, 28))


@pytest.mark.parametrize("over", [dict(coarse_embed_dim=192), dict(object_inter_module_num_heads=3), dict(object_size=33),
                                  dict(object_size=0), dict(coarse_embed_dim=128, object_inter_module_num_heads=8),
                                  dict(object_inter_module_num_layers=5)])
def test_shapes_outside_the_compiled_set_are_refused(over):
    from text2loc_amd.engine import T2LError

    with pytest.raises(T2LError) as ei:
        build(**over)
    msg = str(ei.value)
    assert "Compiled set" in msg and "128" in msg and "256" in msg and "head_dim 32 or 64" in msg and "1..32" in msg


def test_the_optimizer_refuses_other_shapes_and_says_why():
    from text2loc_amd import optim
    from text2loc_amd.engine import T2LError

    m = build(coarse_embed_dim=128)
    with pytest.raises(T2LError, match="published shape only"):
        optim.Adam(m, lr=1e-3)
