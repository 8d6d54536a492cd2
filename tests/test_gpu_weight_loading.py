"""GPU tier: a refused weight load changes nothing. Every eval-mode loader validates and stages the whole state dict on the host before
it touches the context or the device (text2loc_amd/csrc/weight_table.h), so after a load that is refused for a missing or a mis-sized
tensor the context serves exactly what it served before: the previous weights, bit for bit, or — on a fresh context — nothing, which
the entry points refuse on the host before any launch."""
import numpy as np
import pytest
import torch

from text2loc_amd import synth
from text2loc_amd.engine import Engine, T2LError

pytestmark = pytest.mark.gpu

LE = "language_encoder."


def _gpu(cells):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}


# ---- the smallest call(s) behind each load, as eng -> [outputs] ------------------------------------------------------------------
def _object_calls():
    cells = _gpu(synth.make_cells(3, seed=11, with_pn_feat=True))
    pc = synth.make_cells(1, seed=12, min_obj=2, max_obj=2)
    pos, rgb = (torch.from_numpy(a).cuda() for a in synth.make_sampled_points(pc, 12))
    return lambda eng: [eng.encode_cells(cells), eng.pointnet_features(pos, rgb, pc["offsets"])]


def _fine_calls():
    cells = _gpu(synth.make_cells(3, seed=13, min_obj=16, max_obj=16))
    hints = torch.from_numpy(np.random.default_rng(13).standard_normal((3, 6, 128)).astype(np.float32)).cuda()

    def run(eng):
        desc = eng.fine_encode_objects(cells)
        return [desc, eng.fine_match(desc, hints)]

    return run


def _text_calls():
    hid = torch.from_numpy(synth.make_t5_hidden(2, 4, seed=14)).cuda()

    def run(eng):
        sent, bad = eng.text_head(hid)
        desc, bad2 = eng.text_inter(sent, 1)
        assert not bad and not bad2
        return [sent, desc]

    return run


def _object_sd():
    sd = dict(synth.make_object_branch_weights(3))
    sd.update(synth.make_pointnet_weights(3))
    return sd


def _load_object(eng, sd):
    eng.load_weights(sd, class_embed=False, color_embed=False)  # the published mode: PointNet++ features2 -> mlp_pointnet


def _load_fine(eng, sd):
    eng.fine_load_weights(sd, class_embed=True, color_embed=True)


def _load_text(eng, sd):
    eng.text_head_load_weights(sd)


# (state dict, load, calls, the tensor that goes missing / gets one element short, what each call says on a context without weights)
CASES = {
    "object branch, encoder tensor": (_object_sd, _load_object, _object_calls, "obj_inter_module.1.norm2.bias",
                                      ["t2l_encode_cells: weights not loaded", "t2l_pointnet_features: the loaded state_dict carried no"]),
    "object branch, backbone tensor": (_object_sd, _load_object, _object_calls, "object_encoder.pointnet.lin2.bias",
                                       ["t2l_encode_cells: weights not loaded", "t2l_pointnet_features: the loaded state_dict carried no"]),
    "fine stage": (lambda: synth.make_fine_weights(3), _load_fine, _fine_calls, "mlp_offsets.2.weight",
                   ["t2l_fine_encode_objects: fine weights not loaded", "t2l_fine_match: fine weights not loaded"]),
    "text head": (lambda: synth.make_language_head_weights(3), _load_text, _text_calls, LE + "inter_mlp.0.1.running_var",
                  ["text_head: call text_head_load_weights first", "text_inter: call text_head_load_weights first"]),
}


def _broken(sd, key):
    """(what is refused, the message that names it): `key` removed, then `key` one element short"""
    missing = {k: v for k, v in sd.items() if k != key}
    short = dict(sd)
    short[key] = np.ascontiguousarray(sd[key]).reshape(-1)[:-1]
    n = int(np.asarray(sd[key]).size)
    return [(missing, f"missing tensor '{key}'"), (short, rf"wrong size for '{key}' \(has {n - 1} elements, needs {n}\)")]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", list(CASES))
def test_a_refused_load_leaves_the_loaded_weights_serving(eng, case):
    make_sd, load, make_calls, key, _ = CASES[case]
    sd, calls = make_sd(), make_calls()
    load(eng, sd)
    kept = [t.clone() for t in calls(eng)]
    torch.cuda.synchronize()
    for bad_sd, message in _broken(sd, key):
        with pytest.raises(T2LError, match=message):
            load(eng, bad_sd)
    again = calls(eng)
    torch.cuda.synchronize()
    assert len(again) == len(kept) and all(torch.equal(a, k) for a, k in zip(again, kept))


@pytest.mark.parametrize("case", list(CASES))
def test_a_refused_load_on_a_fresh_context_leaves_nothing_to_launch(case):
    make_sd, load, _, key, not_loaded = CASES[case]
    sd = make_sd()
    z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    cells = _gpu(synth.make_cells(3, seed=13, min_obj=16, max_obj=16, with_pn_feat=True))
    attempts = {
        "t2l_encode_cells": lambda e: e.encode_cells(cells),
        "t2l_pointnet_features": lambda e: e.pointnet_features(z(2, 256, 3), z(2, 256, 3), np.array([0, 2])),
        "t2l_fine_encode_objects": lambda e: e.fine_encode_objects(cells),
        "t2l_fine_match": lambda e: e.fine_match(z(3, 16, 128), z(3, 6, 128)),
        "text_head": lambda e: e.text_head(z(2, 4, 1024)),
        "text_inter": lambda e: e.text_inter(z(2, 256), 1),
    }
    e = Engine(0)
    try:
        for bad_sd, message in _broken(sd, key):
            with pytest.raises(T2LError, match=message):
                load(e, bad_sd)
            for text in not_loaded:
                with pytest.raises(T2LError, match=text):
                    attempts[text.split(":")[0]](e)
    finally:
        e.close()
