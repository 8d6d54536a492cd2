"""Drop-in for the reference's fine-stage training loop (training/fine.py:38-121) and its pose error
(training/losses.py:126-170), around the engine's training-mode ``CrossMatch`` (cross_matcher.py).

Batches are in ``Kitti360FineDataset.collate_fn`` format: ``objects`` (per pose, the cell's objects padded / cut to 16),
``texts``, ``offsets`` (target offsets [B,2]), ``poses`` (objects with a ``.pose`` attribute) and ``object_points`` (per pose,
in the published feature mode: the cell's point batch — ``.pos`` / ``.x`` [16*256,3] or a dict with those keys, as the
reference's dataloader builds it — which trains the PointNet++ backbone jointly unless ``--pointnet_freeze``, or precomputed
features2 [16,256] as tensors; ignored when class_embed is on). The reference reads the optimizer and the MSE criterion from
module globals; here they are passed in.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch


class _Stats(dict):
    __getattr__ = dict.__getitem__


def calc_pose_error2(objects, poses, offsets=None, return_samples=False):
    """training/losses.py:126-170: per sample, the x-y distance between the ground-truth pose and the predicted offsets."""
    assert len(objects) == len(poses)
    poses = np.array([pose.pose for pose in poses])[:, 0:2]
    if offsets is None:
        raise TypeError("calc_pose_error2 needs offsets")
    assert len(objects) == len(offsets)
    errors: List[float] = [float(np.linalg.norm(poses[i] - offsets[i])) for i in range(len(poses))]
    return errors if return_samples else float(np.mean(errors))


def train_epoch(model, dataloader, args, optimizer, criterion):
    """training/fine.py:38-91: zero_grad, forward, offset_lambda * MSE, backward, optimizer.step per batch."""
    model.train()
    device = model.device
    stats = _Stats(loss=[], loss_offsets=[], pose_offsets=[])
    for batch in dataloader:
        optimizer.zero_grad()
        output = model(batch["objects"], batch["texts"], batch["object_points"])
        loss_offsets = criterion(output, torch.tensor(np.asarray(batch["offsets"]), dtype=torch.float, device=device))
        loss = args.offset_lambda * loss_offsets
        loss.backward()
        optimizer.step()
        stats["loss"].append(loss.item())
        stats["loss_offsets"].append(loss_offsets.item())
        stats["pose_offsets"].append(calc_pose_error2(batch["objects"], batch["poses"], offsets=output.detach().cpu().numpy()))
    return _Stats({k: float(np.mean(v)) for k, v in stats.items()})


@torch.no_grad()
def eval_epoch(model, dataloader, args):
    """training/fine.py:94-121: mean pose error of the eval-mode offsets."""
    model.eval()
    stats = _Stats(pose_offsets=[])
    for batch in dataloader:
        output = model(batch["objects"], batch["texts"], batch["object_points"])
        stats["pose_offsets"].append(calc_pose_error2(batch["objects"], batch["poses"], offsets=output.detach().cpu().numpy()))
    return _Stats({k: float(np.mean(v)) for k, v in stats.items()})
