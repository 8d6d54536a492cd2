"""Restatements the coarse-batch tests hold the engine against (tests/test_coarse_dataset_cpu.py, tests/test_gpu_coarse_batches*.py).

A mirrored sampler row: oracle/t2l_oracle_pointnet.py: sample_object_points — unchanged — run over a float32 copy of the point set in
which the object's x and / or y were replaced by ``np.float32(1) - x`` (include/t2l.h: t2l_sample_object_points_mirrored), at seed
``seed ^ salt``, row ``g``. Mirroring commutes with the index draw (the key does not contain the code), so mirroring the set first and
sampling it afterwards IS the entry point's definition. A gathered row: the table row, its centre's x / y replaced the same way.
"""
import numpy as np

from oracle import t2l_oracle_pointnet as OP

F32 = np.float32


def mirror_points(xyz, code):
    """float32 copy of ``xyz`` [n,3] with x -> float32(1) - x under bit 0 of ``code`` and y -> float32(1) - y under bit 1."""
    out = np.array(xyz, dtype=F32, copy=True)
    for ax in (0, 1):
        if (int(code) >> ax) & 1:
            out[:, ax] = F32(1) - out[:, ax]
    return out


def sample_rows(xyz, rgb, poff, ids, salts, mirror, seed, transform, cache=None):
    """(pos, rgb) f32[n_rows,256,3]: row r = row ids[r] of the oracle over the set mirrored under mirror[r], at seed ^ salts[r]. The
    oracle samples every object of the arrays it is handed independently, so one run per (salt, code) over the set with EVERY object
    mirrored under that code serves all rows of that (salt, code). An object without points is a row of zeros (include/t2l.h); the
    oracle is handed one spare point behind the last object so that its index 0 of such an object stays inside the arrays."""
    xyz, rgb, poff = np.asarray(xyz, dtype=F32), np.asarray(rgb, dtype=F32), np.asarray(poff, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    salts = np.zeros(len(ids), dtype=np.uint32) if salts is None else np.asarray(salts, dtype=np.uint32)
    mirror = np.zeros(len(ids), dtype=np.uint8) if mirror is None else np.asarray(mirror, dtype=np.uint8)
    cache = {} if cache is None else cache
    empty = (poff[1:] - poff[:-1]) == 0
    pos, col = np.empty((len(ids), 256, 3), F32), np.empty((len(ids), 256, 3), F32)
    for r, (g, salt, code) in enumerate(zip(ids.tolist(), salts.tolist(), mirror.tolist())):
        key = (salt, code, transform)
        if key not in cache:
            spare = np.zeros((1, 3), F32)
            with np.errstate(all="ignore"):  # a one-point object under NormalizeScale is 0 * inf on both sides
                cache[key] = OP.sample_object_points(np.concatenate([mirror_points(xyz, code), spare]), np.concatenate([rgb, spare]), poff,
                                                     int(seed) ^ int(salt), transform=transform)
        pos[r], col[r] = (0, 0) if empty[g] else (cache[key][0][g], cache[key][1][g])
    return pos, col


def gather_rows(table, ids, mirror):
    """The five per-object arrays with one row per id: row ids[r] of ``table`` (numpy arrays), centre mirrored as float32(1) - c."""
    ids = np.asarray(ids, dtype=np.int64)
    out = {k: np.array(np.asarray(table[k])[ids], copy=True) for k in ("class_idx", "color_idx", "rgb", "center", "n_pts")}
    if mirror is not None:
        for ax in (0, 1):
            sel = ((np.asarray(mirror, dtype=np.uint8) >> ax) & 1).astype(bool)
            out["center"][sel, ax] = F32(1) - out["center"][sel, ax]
    return out


class _NoPose:
    """What ``flip_pose_in_cell`` touches of a pose."""

    def __init__(self):
        self.pose, self.descriptions = np.zeros(3), []


def host_flipped_cell(cell, code):
    """The cell as the "sample" dataset hands it on under flip code ``code``: ``kitti360pose.flip_pose_in_cell`` once per set bit
    (horizontal first, as ``Kitti360PoseDataset.__getitem__`` does); code 0 is the record itself."""
    from text2loc_amd import kitti360pose as K

    for bit, direction in ((1, 1), (2, -1)):
        if int(code) & bit:
            _, cell, _ = K.flip_pose_in_cell(_NoPose(), cell, "", direction)
    return cell


def diff_count(a, b):
    """Elements whose BITS differ; two NaNs count as equal whatever their sign (tests/test_gpu_sample_indexed.py: diff_count)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    both_nan = np.isnan(a) & np.isnan(b)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).sum())


__all__ = ["mirror_points", "sample_rows", "gather_rows", "host_flipped_cell", "diff_count"]
