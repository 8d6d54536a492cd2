"""GPU tier: what a re-bind does to the optimizer state inside the library (train.hip: AdamSet, one for the object branch and one for
the text head). With option train_keep_adam_state the moments and the step carry over exactly when the list of trained tensors is
unchanged; a changed list or a refused bind starts from zero."""
import numpy as np
import pytest
import torch

from tests.fine_text_twin import fine_head_weights
from tests.test_gpu_text_train import P
from tests.test_gpu_train import used_names
from text2loc_amd import synth

pytestmark = pytest.mark.gpu


def _tens(sd):
    return {k: (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda(), None if "running_" in k else torch.zeros(v.shape, device="cuda"))
            for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def _head_tens(seed):
    return _tens({k: v for k, v in synth.make_language_head_weights(seed).items()
                  if k.startswith((P + "intra_module.0.", P + "inter_mlp.0.", P + "inter_module.0."))})


def test_text_head_rebind_keeps_the_state_of_an_unchanged_list_and_drops_it_for_another():
    from text2loc_amd.engine import Engine

    hidden = torch.from_numpy(synth.make_t5_hidden(4, 4, seed=3)).cuda()  # 2 descriptions x 2 sentences x 4 tokens
    G = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 256)).astype(np.float32)).cuda()
    eng, twin = Engine(0), Engine(0)
    try:
        ta, tb = _head_tens(5), _head_tens(5)
        eng.text_train_bind(ta)
        twin.text_train_bind(tb)  # never re-bound; adam_kernel is element-wise, so fed eng's gradients it must stay bit-equal to eng

        def step(i):
            eng.text_zero_grad()
            eng.text_head_train(hidden, 2, dropout_p=0.1, seed=i)
            eng.text_head_backward(G)
            for k, (_, g) in ta.items():
                if g is not None:
                    tb[k][1].copy_(g)
            eng.text_adam_step(1e-3)
            twin.text_adam_step(1e-3)
            torch.cuda.synchronize()
            for k in ta:
                assert torch.equal(ta[k][0], tb[k][0]) or "running_" in k, (i, k)

        step(1)
        step(2)
        m0, v0, s0 = eng.text_adam_state()
        assert s0 == 2 and float(m0.abs().max()) > 0 and float(v0.abs().max()) > 0
        eng.set_option("train_keep_adam_state", 1)
        k = P + "inter_mlp.0.0.weight"
        ta[k] = (ta[k][0], torch.zeros_like(ta[k][1]))  # the same list, one gradient buffer moved
        eng.text_train_bind(ta)
        m1, v1, s1 = eng.text_adam_state()
        assert s1 == 2 and torch.equal(m1, m0) and torch.equal(v1, v0)
        step(3)
        assert eng.text_adam_state()[2] == 3
        # another list on the same context, the option still on: the fine layout (no inter_module tensors) starts from nothing
        eng.text_train_bind(_tens(fine_head_weights(5)))
        m2, v2, s2 = eng.text_adam_state()
        assert s2 == 0 and m2.numel() < m0.numel() and float(m2.abs().max()) == 0.0 and float(v2.abs().max()) == 0.0
    finally:
        eng.close()
        twin.close()


def test_object_branch_rebind_drops_the_state_when_the_list_changes():
    from text2loc_amd.engine import Engine

    eng = Engine(0)
    try:
        tens = _tens(used_names(synth.make_object_branch_weights(2), True))
        eng.train_bind(tens, class_embed=True, color_embed=True)
        m, v, _ = eng.adam_state()
        eng.set_adam_state(torch.full_like(m, 0.5), torch.full_like(v, 0.25), 7)
        eng.set_option("train_keep_adam_state", 1)
        eng.train_bind(tens, class_embed=True, color_embed=True)  # unchanged: kept
        m1, v1, s1 = eng.adam_state()
        assert s1 == 7 and m1.numel() == m.numel() and float(m1.min()) == 0.5 and float(v1.max()) == 0.25
        eng.train_bind(tens, class_embed=True, color_embed=True, num_layers=1)  # obj_inter_module.1.* no longer trained
        m2, v2, s2 = eng.adam_state()
        assert s2 == 0 and m2.numel() < m.numel() and float(m2.abs().max()) == 0.0 and float(v2.abs().max()) == 0.0
    finally:
        eng.close()


def test_text_head_refused_rebind_leaves_nothing_bound_and_the_next_bind_starts_from_zero():
    from text2loc_amd.engine import Engine, T2LError

    eng = Engine(0)
    try:
        tens = _head_tens(1)
        eng.text_train_bind(tens)
        m, v, _ = eng.text_adam_state()
        eng.set_text_adam_state(torch.full_like(m, 0.5), torch.full_like(v, 0.25), 4)
        eng.set_option("train_keep_adam_state", 1)
        broken = dict(tens)
        w = tens[P + "inter_module.0.linear1.weight"][0]
        broken[P + "inter_module.0.linear1.weight"] = (w[:512].contiguous(), torch.zeros_like(w[:512]))
        with pytest.raises(T2LError, match="missing, mis-sized or without a gradient buffer"):
            eng.text_train_bind(broken)
        with pytest.raises(T2LError, match="t2l_text_train_bind first"):
            eng.text_adam_state()
        eng.text_train_bind(tens)
        m1, v1, s1 = eng.text_adam_state()
        assert s1 == 0 and float(m1.abs().max()) == 0.0 and float(v1.abs().max()) == 0.0
    finally:
        eng.close()
