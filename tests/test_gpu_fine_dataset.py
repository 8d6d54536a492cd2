"""GPU tier: ``Kitti360FineDataset(object_points="ids")`` + ``fine_batches`` feeding the engine's fine stage on
tests/golden/k360_fine_tiny (tools/gen_golden_fine_dataset.py): the batch's 16 * B point rows are sampled on the GPU in one launch
(t2l_sample_object_points_indexed) and reach ``CrossMatch`` as the per-pose ``{"pos", "x"}`` views it already accepts."""
import argparse
import os.path as osp

import numpy as np
import pytest
import torch

from oracle import t2l_oracle_pointnet as OP
from tests.test_gpu_fine_train_points import weights
from tests.test_oracle_fine_train import fine_args
from text2loc_amd import kitti360pose as K
from text2loc_amd import synth
from text2loc_amd.fine_training import eval_epoch, train_epoch

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
BASE = osp.join(GOLDEN, "k360_fine_tiny")
B = 4


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "k360_fine_tiny.npz"), allow_pickle=False)


class TextTable(torch.nn.Module):
    """Text-branch stand-in with a trainable table: one row [6,128] of hint encodings per distinct pose text."""

    def __init__(self, texts, seed=0):
        super().__init__()
        self.row = {t: i for i, t in enumerate(sorted(set(texts)))}
        self.table = torch.nn.Parameter(torch.from_numpy(np.random.default_rng(seed).standard_normal((len(self.row), 6, 128)).astype(np.float32)))

    def forward(self, texts):
        return self.table[torch.as_tensor([self.row[t] for t in texts], device=self.table.device)]


def problem(gold, embed, seed=5):
    from text2loc_amd.cross_matcher import CrossMatch

    args = fine_args(embed)
    args.pointnet_freeze = False
    args.regressor_cell, args.regressor_learn = "all", "center"  # the published command
    ds = K.Kitti360FineDataset(BASE, [str(s) for s in gold["scenes"]], args, object_points="ids", transform="fixed", seed=seed)
    model = CrossMatch(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=TextTable([ds[i]["texts"] for i in range(len(ds))]))
    sd = weights(3, 2) if not embed else synth.make_fine_weights(3, num_layers=2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    return ds, model.cuda(), args


def recorded(batches, sink):
    for b in batches:
        sink.append(b)
        yield b


def test_device_sampled_batch_equals_its_host_replay(gold):
    """Published feature mode, B = 4, eval: the offsets from the batch ``fine_batches`` sampled on the GPU equal, bit for bit, the offsets
    from the same batch with every row's points replayed on the host by the numpy restatement over the whole set at seed ^ salt."""
    ds, model, _ = problem(gold, embed=False)
    model.eval()
    batch = next(K.fine_batches(ds, B, "cuda", shuffle=True, seed=1, epoch=2))
    assert len(batch["objects"]) == B and all(tuple(p["pos"].shape) == (16 * 256, 3) and p["pos"].is_cuda for p in batch["object_points"])
    with torch.no_grad():
        model(batch["objects"], batch["texts"], batch["object_points"])  # (first touch of these objects: their reductions get cached)
        got = model(batch["objects"], batch["texts"], batch["object_points"])
    ps = ds.packed()
    xyz = np.concatenate([ps.xyz, ps.pad_points()[0]])
    rgb = np.concatenate([ps.rgb, ps.pad_points()[1]])
    poff = np.append(ps.point_offsets, ps.point_offsets[-1] + 8)
    replay = []
    for rows, salts in zip(batch["object_rows"], batch["draw_salts"]):
        pos, col = np.empty((16, 256, 3), np.float32), np.empty((16, 256, 3), np.float32)
        for s, (row, salt) in enumerate(zip(rows, salts)):
            wpos, wcol = OP.sample_object_points(xyz, rgb, poff, ds.point_seed ^ int(salt), transform="fixed")
            pos[s], col[s] = wpos[row], wcol[row]
        replay.append({"pos": pos.reshape(-1, 3), "x": col.reshape(-1, 3)})
    for p, r in zip(batch["object_points"], replay):
        assert np.array_equal(p["pos"].cpu().numpy(), r["pos"]) and np.array_equal(p["x"].cpu().numpy(), r["x"])
    with torch.no_grad():
        ref = model(batch["objects"], batch["texts"], replay)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # the same (seed, epoch) gives the same batch; another epoch draws anew
    again = next(K.fine_batches(ds, B, "cuda", shuffle=True, seed=1, epoch=2))
    assert again["texts"] == batch["texts"] and all(torch.equal(a["pos"], b["pos"]) for a, b in zip(again["object_points"], batch["object_points"]))


@pytest.mark.parametrize("embed", [False, True], ids=["published", "embedding"])
def test_two_epochs_of_training(gold, embed):
    torch.manual_seed(0)
    ds, model, args = problem(gold, embed)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.MSELoss()
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    seen = [[], []]
    for epoch in range(2):
        stats = train_epoch(model, recorded(K.fine_batches(ds, B, "cuda", epoch=epoch), seen[epoch]), args, opt, crit)
        assert np.isfinite(stats["loss"]) and np.isfinite(stats["pose_offsets"])
    for batches in seen:
        assert [len(b["texts"]) for b in batches] == [4, 4, 3]
        assert np.array_equal(np.concatenate([np.asarray(b["offsets"]) for b in batches]), gold["r4_offsets"])  # targets: regressor "all"
    for b0, b1 in zip(*seen):  # the same items, fresh draws
        assert b0["texts"] == b1["texts"]
        assert not any(torch.equal(p0["pos"], p1["pos"]) for p0, p1 in zip(b0["object_points"], b1["object_points"]))
    after = model.state_dict()
    moved = {k for k, v in before.items() if not torch.equal(v, after[k])}
    prefixes = ["language_encoder.table", "mlp_offsets.", "object_encoder.pos_encoder."] + ([] if embed else ["object_encoder.pointnet.lin2."])
    for p in prefixes:
        assert any(k.startswith(p) and "running_" not in k for k in moved), p
    stats_of = "object_encoder.pos_encoder." if embed else "object_encoder.pointnet."
    assert any(k.startswith(stats_of) and "running_mean" in k for k in moved) and any(k.startswith(stats_of) and "running_var" in k for k in moved)


def test_eval_epoch_over_the_generator(gold):
    ds, model, args = problem(gold, embed=False)
    stats = eval_epoch(model, K.fine_batches(ds, B, "cuda"), args)
    assert np.isfinite(stats["pose_offsets"]) and stats["pose_offsets"] >= 0.0
    assert not model.training
