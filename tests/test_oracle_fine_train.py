"""CPU tier of the fine stage's training step: the float64 twin (tests/fine_train_twin.py) against torch's own modules, its
dropout-mask replay, and the host-side refusals of CrossMatch under model.train()."""
import argparse

import numpy as np
import pytest
import torch

from oracle.t2l_oracle_train import dropout_keep
from tests.fine_train_twin import Twin, module_step
from text2loc_amd import synth
from text2loc_amd.engine import T2LError

CONFIGS = {"embed": (True, 2, ("class", "color", "position", "num")), "pn": (False, 2, ("class", "color", "position", "num")),
           "embed_l0": (True, 0, ("class", "color", "position", "num")), "pn_subset": (False, 1, ("class", "position")),
           "pn_noclass": (False, 1, ("color", "position"))}


def fine_args(embed, n_layers=2, use_features=("class", "color", "position", "num")):
    return argparse.Namespace(fine_embed_dim=128, fine_num_decoder_heads=4, fine_num_decoder_layers=n_layers, pad_size=16, num_mentioned=6,
                              fine_intra_module_num_layers=1, fine_intra_module_num_heads=4, hungging_model=None, fixed_embedding=True,
                              class_embed=embed, color_embed=embed, pointnet_freeze=True, use_features=list(use_features),
                              offset_lambda=1.0)


def problem(embed, n_layers, P=8, H=6, seed=0, use=("class", "color", "position", "num")):
    sd = synth.make_fine_weights(seed, num_layers=n_layers)
    sd["object_encoder.mlp_merge.0.0.weight"] = np.ascontiguousarray(sd["object_encoder.mlp_merge.0.0.weight"][:, :128 * len(use)])
    cells = synth.make_cells(P, seed=seed + 3, min_obj=16, max_obj=16)
    rng = np.random.default_rng(seed + 11)
    hints = rng.standard_normal((P, H, 128)).astype(np.float32)
    pn = None if embed else rng.standard_normal((P * 16, 256)).astype(np.float32)
    gout = rng.standard_normal((P, 2)).astype(np.float32)
    return sd, cells, hints, pn, gout


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.sqrt((b ** 2).mean()), 1e-30))


def torch_model(sd, args):
    from text2loc_amd.cross_matcher import CrossMatch

    m = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=torch.nn.Identity())
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    m = m.double().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return m


@pytest.mark.parametrize("mode", sorted(CONFIGS))
def test_twin_matches_torch_modules_in_train_mode(mode):
    embed, L, use = CONFIGS[mode]
    sd, cells, hints, pn, gout = problem(embed, L, use=use)
    args = fine_args(embed, L, use)
    model = torch_model(sd, args)
    off_m, g_m, gh_m, gp_m = module_step(model, cells, hints, gout, pn)
    twin = Twin(sd, embed, embed, use, L)
    off_t, g_t, gh_t, gp_t = twin.step(cells, hints, gout, pn)
    assert rel(off_t, off_m) < 1e-10
    assert rel(gh_t, gh_m) < 1e-8
    if gp_m is not None or gp_t is not None:
        assert rel(gp_t, gp_m) < 1e-8
    names = {n for n in g_m if not n.startswith("object_encoder.pointnet.")}
    assert names == set(g_t), sorted(names ^ set(g_t))
    for n in names:
        if n.startswith("object_encoder.") and n.endswith(".0.bias") and np.sqrt((g_m[n] ** 2).mean()) < 1e-9:
            assert np.abs(g_t[n]).max() < 1e-12, n  # Linear bias in front of a BatchNorm: true gradient 0
            continue
        assert rel(g_t[n], g_m[n]) < 1e-8, n
    run = twin.running()
    assert run
    for n, v in run.items():
        assert rel(v, model.state_dict()[n].numpy()) < 1e-12, n


def test_twin_replays_the_abi_masks():
    sd, cells, hints, _, gout = problem(True, 1, P=3, H=4)
    twin = Twin(sd, True, True, n_layers=1)
    a, _, _, _ = twin.step(cells, hints, gout, p=0.25, seed=9)
    b, _, _, _ = twin.step(cells, hints, gout, p=0.25, seed=9)
    c, _, _, _ = twin.step(cells, hints, gout, p=0.25, seed=10)
    d, _, _, _ = twin.step(cells, hints, gout, p=0.0, seed=9)
    assert np.array_equal(a, b) and not np.allclose(a, c) and not np.allclose(a, d)
    # the mask rule itself: element i of site j kept iff lowbias32(i*0x9E3779B1 + (seed ^ j*0x85EBCA77)) >> 8 >= p*2^24
    keep = dropout_keep(9, 7, 4096, 0.25)
    assert abs(1 - keep.mean() - 0.25) < 0.03

    def lowbias32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    for i in (0, 1, 77, 4095):
        assert keep[i] == ((lowbias32(i * 0x9E3779B1 + (9 ^ ((7 * 0x85EBCA77) & 0xFFFFFFFF))) >> 8) >= int(0.25 * (1 << 24)))


def test_train_mode_refusals_on_the_host():
    from tests.test_host_logic import make_objects
    from text2loc_amd.cross_matcher import CrossMatch, pad_objects

    cells = synth.make_cells(2, seed=1, min_obj=16, max_obj=16)
    objects = [pad_objects(o) for o in make_objects(cells, 1)]
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, fine_args(False), language_encoder=torch.nn.Identity()).train()
    pts = [{"pos": np.zeros((16 * 256, 3), np.float32), "x": np.zeros((16 * 256, 3), np.float32)} for _ in objects]
    with pytest.raises(T2LError, match="PointNet\\+\\+ backbone, which is not built for the fine stage"):
        model(objects, torch.zeros(2, 6, 128), pts)
    with pytest.raises(T2LError, match="object_points must hold"):
        model(objects, torch.zeros(2, 6, 128), None)
    with pytest.raises(T2LError, match="exactly pad_size"):
        model([o[:5] for o in objects], torch.zeros(2, 6, 128), None)
    with pytest.raises(T2LError, match="MI355X only"):
        model(objects, torch.zeros(2, 6, 128), [torch.zeros(16, 256) for _ in objects])
    model.cross_hints[1].dropout2.p = 0.2
    with pytest.raises(T2LError, match="one dropout probability"):
        model(objects, torch.zeros(2, 6, 128), [torch.zeros(16, 256) for _ in objects])
    with pytest.raises(T2LError, match="eval-only"):
        model.encode_cells(objects, [torch.zeros(16, 256) for _ in objects])


def test_calc_pose_error2():
    from text2loc_amd.fine_training import calc_pose_error2

    class P:
        def __init__(self, xy):
            self.pose = np.array([xy[0], xy[1], 0.0])

    err = calc_pose_error2([[0], [0]], [P((0.5, 0.5)), P((0.0, 1.0))], offsets=np.array([[0.5, 0.2], [0.0, 0.0]]))
    assert abs(err - (0.3 + 1.0) / 2) < 1e-12
    assert calc_pose_error2([[0]], [P((1, 1))], offsets=np.zeros((1, 2)), return_samples=True) == [pytest.approx(np.sqrt(2))]


# ---- the reference's own CrossMatch training step (tests/golden/fine_train_*.npz, tools/gen_golden_fine_train.py) --------
def golden_case(g):
    embed, L = bool(g["embed"]), int(g["n_layers"])
    sd = synth.make_fine_weights(int(g["weight_seed"]), num_layers=L)
    cells = {k[3:]: g[k] for k in g.files if k.startswith("in_") and k != "in_pn_feat"}
    pn = g["in_pn_feat"] if "in_pn_feat" in g.files else None
    return embed, L, sd, cells, pn


def grad_errors(g, name, full):
    """max |error| / rms of one gradient at the fixture's sample positions (the rms from the full tensor's norm)."""
    from tests.test_oracle_train import golden_view

    exp, got = golden_view(g, "grad", name, full)
    rms = float(g[f"grad_norm/{name}"]) / np.sqrt(np.asarray(full).size)
    return float(np.abs(got - exp).max()), rms


@pytest.mark.parametrize("name", ["embed", "pn", "embed_l0"])
def test_twin_reproduces_the_reference_training_step(golden, name):
    g = golden(f"fine_train_{name}")
    embed, L, sd, cells, pn = golden_case(g)
    twin = Twin(sd, embed, embed, n_layers=L)
    h = torch.tensor(g["hint_encodings"], dtype=torch.float64, requires_grad=True)
    p = None if pn is None else torch.tensor(pn, dtype=torch.float64, requires_grad=True)
    out = twin.forward(cells, h, p, train=True)
    loss = float(g["offset_lambda"]) * ((out - torch.tensor(g["targets"], dtype=torch.float64)) ** 2).mean()
    loss.backward()
    assert np.abs(out.detach().numpy() - g["offsets_out"]).max() < 1e-5
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * max(1.0, float(g["loss"]))
    assert rel(h.grad.numpy(), g["grad_hint"]) < 1e-4
    if p is not None:
        assert rel(p.grad.numpy(), g["grad_pn"]) < 1e-4
    used = [str(x) for x in g["used_params"]]
    assert set(used) == {k for k, v in twin.t.items() if v.grad is not None}
    for n in used:
        err, rms = grad_errors(g, n, twin.t[n].grad.numpy())
        if n.startswith("object_encoder.") and n.endswith(".0.bias"):
            assert err < 1e-4, n  # true gradient 0 (a BatchNorm follows): the float32 reference leaves rounding noise
            continue
        if n.endswith("num_encoder.0.0.weight"):
            assert err < 2e-4, n  # [64,1] Linear before a BatchNorm: scale-invariant, only an eps residual (float32 noise)
            continue
        assert err < 1e-4 * rms + 1e-9, (n, err, rms)
    for k in g.files:
        if k.startswith("buf/"):
            assert np.allclose(twin.t[k[4:]].detach().numpy(), g[k], rtol=1e-5, atol=1e-7), k
