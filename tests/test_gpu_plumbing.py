"""GPU tier: what the shared object_points reader changed in eval mode — ``CrossMatch.encode_cells`` voids the colours of point batches
when "color" is not in use_features (models/object_encoder.py:86-90 does so in both modes) and refuses mixed kinds, as the training arm does."""
import numpy as np
import pytest
import torch

from tests.test_gpu_fine_train_points import scene, weights
from tests.test_oracle_fine_train import fine_args
from text2loc_amd import synth
from text2loc_amd.engine import T2LError

pytestmark = pytest.mark.gpu


def test_fine_eval_voids_the_colours_of_point_batches_like_the_training_arm():
    from text2loc_amd.cross_matcher import CrossMatch

    use, B = ("class", "position", "num"), 2
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, fine_args(False, 2, use), language_encoder=torch.nn.Identity())
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights(5, 2, use).items()}, strict=False)
    model = model.cuda().eval()
    objects, _, batches, _, _ = scene(B, 5)
    rng = np.random.default_rng(6)
    batches = [{"pos": b["pos"], "x": rng.random(b["x"].shape).astype(np.float32)} for b in batches]  # 16 objects of 256 points each
    keep = [b["x"].copy() for b in batches]
    got = model.encode_cells(objects, batches)
    assert tuple(got.shape) == (B, 16, 128) and bool(torch.isfinite(got).all())
    assert all(np.array_equal(b["x"], k) for b, k in zip(batches, keep))  # the caller's colours are untouched
    black = model.encode_cells(objects, [{"pos": b["pos"], "x": np.zeros_like(b["x"])} for b in batches])
    assert torch.equal(got, black)
    # what eval mode computed before: the same weights, the backbone fed the colours as they came
    to_gpu = lambda key: torch.from_numpy(np.concatenate([b[key] for b in batches]).reshape(-1, 256, 3)).cuda()
    f2 = model.engine().pointnet_features(to_gpu("pos"), to_gpu("x"), np.arange(0, 16 * B + 1, 16, dtype=np.int32))
    unvoided = model.encode_cells(objects, list(f2.reshape(B, 16, 256)))
    f2_black = model.engine().pointnet_features(to_gpu("pos"), torch.zeros_like(to_gpu("x")), np.arange(0, 16 * B + 1, 16, dtype=np.int32))
    assert not torch.equal(f2, f2_black) and not torch.equal(unvoided, got)  # (both paths are deterministic: any difference is the colours')
    assert torch.equal(model.encode_cells(objects, list(f2_black.reshape(B, 16, 256))), got)  # features2 tensors pass through as before
    with pytest.raises(T2LError, match="mixes point batches and features2"):
        model.encode_cells(objects, [batches[0], f2[:16]])
    for short in ([f2[:16]], [batches[0]]):  # object_points for one cell, objects for two
        with pytest.raises(T2LError, match="exactly the objects of each cell: 2 cells of 16, got 16"):
            model.encode_cells(objects, short)
