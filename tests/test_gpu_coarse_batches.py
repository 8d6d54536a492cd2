"""GPU tier: coarse training batches from the resident cell set — t2l_sample_object_points_mirrored, t2l_gather_object_rows,
``PackedCellSet.gather_rows`` / ``sample_rows(mirror=...)``, ``coarse_batches`` and ``plumbing.pack_objects`` behind them.

References: oracle/t2l_oracle_pointnet.py: sample_object_points over the mirrored set and the numpy gather (tests/coarse_batch_ref.py),
both bit for bit; ``packing.pack_cells`` of the host-flipped cells (``flip_pose_in_cell``) for what the model reads; the float64
training oracle (oracle/t2l_oracle_train.py) at the bars of tests/test_gpu_train.py for what the model computes from it.
"""
import inspect
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import t2l_oracle_train as OT
from tests import coarse_batch_ref as R
from tests import guards as G
from tests import test_gpu_reduce, test_gpu_train
from tests.test_gpu_memory_safety import dev, engine, same_bits
from tests.test_gpu_train import assert_grads
from text2loc_amd import engine as E
from text2loc_amd import kitti360pose as K
from text2loc_amd import packing, synth

pytestmark = pytest.mark.gpu

TRANSFORMS = ["fixed", "normalize", "rotate_normalize"]
SEED = 0x51F0CA7
SIZES = [37, 0, 1, 2, 300, 37, 0, 300, 1, 2, 0, 300]  # 12 objects; the last one ends the arrays
SALT_POOL = np.array([0, 0xDEADBEEF, 0, 0x9E3779B1], dtype=np.uint32)  # salt 0 = an unsalted row


def _bound(fn, pattern):
    """A tolerance another test file holds, read from that test's source: the number is stated once, there."""
    found = re.findall(pattern, inspect.getsource(fn))
    assert len(found) == 1, (fn.__name__, pattern, found)
    return float(found[0])


# the engine's reduction against the host packer's, rgb / center (tests/test_gpu_reduce.py)
REDUCE_CENTER_BOUND = _bound(test_gpu_reduce.test_gpu_packer_equals_host_packer_and_feeds_the_encoder, r"host\[k\]\)\.max\(\) < ([0-9.e-]+), k")
# the engine's training forward against the float64 oracle (tests/test_gpu_train.py)
TRAIN_OUTPUT_BOUND = _bound(test_gpu_train.forward_backward_case, r"- ref_out\)\.max\(\) < ([0-9.e-]+)")


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def pts():
    rs = np.random.default_rng(12)
    n_pts = np.array(SIZES, dtype=np.int64)
    total = int(n_pts.sum())
    xyz = (rs.uniform(0.2, 0.8, size=(len(SIZES), 3)).repeat(n_pts, axis=0) + rs.standard_normal((total, 3)) * 0.05).astype(np.float32)
    rgb = rs.uniform(0, 1, size=(total, 3)).astype(np.float32)
    poff = np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int64)
    return {"xyz": xyz, "rgb": rgb, "poff": poff, "dev": (dev(xyz), dev(rgb), dev(poff)), "cache": {}}


def row_list():
    """40 rows: every object three times under three different codes (12 divides no run of codes evenly: code = (r + r // 12) % 4),
    then the last object and three more — object 4 twice in a row under two codes; salts cycle through SALT_POOL (half of them 0)."""
    ids = np.array(list(range(12)) * 3 + [11, 4, 4, 7], dtype=np.int32)
    r = np.arange(len(ids))
    return ids, SALT_POOL[r % 4], ((r + r // 12) % 4).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- sampler rows
@pytest.mark.parametrize("transform", TRANSFORMS)
def test_sampler_rows_equal_the_restatement(eng, pts, transform):
    ids, salts, mirror = row_list()
    assert {int(m) for m in mirror} == {0, 1, 2, 3} and len({int(m) for m in mirror[ids == 4]}) >= 2 and 11 in ids
    pos, col = eng.sample_object_points_mirrored(*pts["dev"], ids, salts, mirror, seed=SEED, transform=transform)
    rpos, rcol = R.sample_rows(pts["xyz"], pts["rgb"], pts["poff"], ids, salts, mirror, SEED, transform, pts["cache"])
    p, c = pos.cpu().numpy(), col.cpu().numpy()
    print(f"{transform}: colours differ in {R.diff_count(c, rcol)} elements, positions in {R.diff_count(p, rpos)} of {p.size}")
    assert R.diff_count(c, rcol) == 0
    assert R.diff_count(p, rpos) == 0
    # code 0 = the indexed entry point, same arguments; the colours never depend on the code
    ipos, icol = eng.sample_object_points_indexed(*pts["dev"], ids, salts, seed=SEED, transform=transform)
    plain = torch.from_numpy(np.flatnonzero(mirror == 0)).cuda()
    assert len(plain) >= 9 and same_bits(pos[plain], ipos[plain])
    assert same_bits(col, icol)
    flipped = np.flatnonzero((mirror != 0) & (np.array(SIZES)[ids] > 2))
    assert all(not torch.equal(pos[int(r)], ipos[int(r)]) for r in flipped)  # (the mirror does reach the positions)


def test_null_mirror_and_null_salts_are_zeros(eng, pts):
    ids, salts, mirror = row_list()
    a = eng.sample_object_points_mirrored(*pts["dev"], ids, None, None, seed=SEED, transform="rotate_normalize")
    b = eng.sample_object_points_mirrored(*pts["dev"], ids, np.zeros_like(salts), np.zeros_like(mirror), seed=SEED, transform="rotate_normalize")
    c = eng.sample_object_points_indexed(*pts["dev"], ids, None, seed=SEED, transform="rotate_normalize")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[0], c[0]) and same_bits(a[1], c[1])


def test_packed_cell_set_sample_rows_with_mirror(eng):
    cells, _ = synth.make_k360_records(4, 1, seed=3)
    ps = packing.PackedCellSet(cells)
    rows = np.array([0, ps.n_objects - 1, 5, 5], dtype=np.int32)
    salts, mirror = np.array([3, 0, 9, 9], dtype=np.uint32), np.array([1, 2, 3, 0], dtype=np.uint8)
    pos, col = ps.sample_rows(eng, "cuda", rows, salts, seed=11, transform="normalize", mirror=mirror)
    rpos, rcol = R.sample_rows(ps.xyz, ps.rgb, ps.point_offsets, rows, salts, mirror, 11, "normalize")
    assert R.diff_count(pos.cpu().numpy(), rpos) == 0 and R.diff_count(col.cpu().numpy(), rcol) == 0
    ipos, _ = ps.sample_rows(eng, "cuda", rows, salts, seed=11, transform="normalize")
    assert same_bits(pos[3], ipos[3]) and not torch.equal(pos[2], ipos[2])


# ---------------------------------------------------------------------------------------------------------------- gather rows
def table(n, seed):
    rs = np.random.default_rng(seed)
    return {"class_idx": rs.integers(0, 22, size=n).astype(np.int32), "color_idx": rs.integers(0, 8, size=n).astype(np.int32),
            "rgb": rs.uniform(0, 1, size=(n, 3)).astype(np.float32), "center": rs.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32),
            "n_pts": rs.integers(1, 60000, size=n).astype(np.float32)}


@pytest.mark.parametrize("n_rows", [1, 40, 1000])
def test_gathered_rows_equal_the_table_rows(eng, n_rows):
    t = table(12, 1)
    d = {k: dev(v) for k, v in t.items()}
    rs = np.random.default_rng(n_rows)
    ids = np.concatenate([[11, 0], rs.integers(0, 12, size=n_rows)])[:n_rows].astype(np.int32)
    mirror = (np.arange(n_rows) % 4).astype(np.uint8)
    got = eng.gather_object_rows(d, ids, mirror)
    ref = R.gather_rows(t, ids, mirror)
    for k, v in ref.items():
        g = got[k].cpu().numpy()
        assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g.view(np.uint32), v.view(np.uint32)), k
    none = eng.gather_object_rows(d, ids, None)
    for k, v in R.gather_rows(t, ids, None).items():
        assert np.array_equal(none[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), k


def tiny_set(counts, seed=4):
    """(cells, poses): one cell per entry of ``counts`` with that many objects and one pose in each, cut from synthetic records.
    Every kept object's points are redrawn around its centre and colour with a point count from ``synth.make_cells`` — log-normal
    with KITTI360Pose's mean and spread (1,827 / 2,517), the counts under which tests/test_gpu_train.py holds the bounds the
    model-level test imports: the count feature is standardised by those two constants and batch-normalised, so a narrow range of
    counts (say 24 to 64) leaves that BatchNorm a variance of 2e-5 to divide float32 round-off by, in the parent's path as here."""
    if (tuple(counts), seed) in _TINY:  # built once and shared: no test writes to the records
        return _TINY[(tuple(counts), seed)]
    cells, poses = synth.make_k360_records(60, 600, seed=seed)
    n_pts = synth.make_cells(1, seed=seed, min_obj=sum(counts), max_obj=sum(counts))["n_pts"].astype(np.int64)
    rs = np.random.default_rng([seed, 0x7E57])
    out_c, out_p, used, k = [], [], set(), 0
    for want in counts:
        c = next(c for c in cells if len(c.objects) >= want and c.id not in used and any(p.cell_id == c.id for p in poses))
        used.add(c.id)
        c.objects = c.objects[:want]
        for o in c.objects:
            n, k = int(n_pts[k]), k + 1
            o.xyz = np.mean(o.xyz, axis=0) + 0.02 * rs.standard_normal((n, 3))
            o.rgb = np.clip(np.mean(o.rgb, axis=0) + 0.05 * rs.standard_normal((n, 3)), 0, 1).astype(np.float32)
        out_c.append(c)
        out_p.append(next(p for p in poses if p.cell_id == c.id))
    _TINY[(tuple(counts), seed)] = (out_c, out_p)
    return out_c, out_p


_TINY = {}


COUNTS = [1, 3, 4, 5, 6, 28, 31, 3, 28, 6, 31, 1]  # 12 cells; 31 > object_size = 28: the cut


def test_gathered_cells_against_the_host_packer_of_the_flipped_cells(eng):
    """``gather_rows`` over the set's reductions against ``pack_cells`` of the cells ``flip_pose_in_cell`` mirrored on the host:
    classes, colours and counts equal; rgb within the reduction's bound; center within that bound plus the one float32 step (2^-23)
    the device's ``1 - c`` on the float32 mean may sit from the host's mean of the mirrored float64 points."""
    cells, _ = tiny_set(COUNTS)
    ps = packing.PackedCellSet(cells)
    kc, colors = packing.class_table(synth.KNOWN_CLASS), packing.color_table()
    codes = (np.arange(len(cells)) % 4).astype(np.uint8)
    counts = [len(c.objects) for c in cells]
    got = ps.gather_rows(eng, "cuda", np.arange(ps.n_objects, dtype=np.int32), np.repeat(codes, counts), counts, kc, colors)
    host = packing.pack_cells([R.host_flipped_cell(c, m).objects for c, m in zip(cells, codes)], kc, colors)
    for k in ("offsets", "class_idx", "color_idx", "n_pts"):
        assert np.array_equal(got[k].cpu().numpy(), host[k]), k
    err_rgb = float(np.abs(got["rgb"].cpu().numpy() - host["rgb"]).max())
    err_c = float(np.abs(got["center"].cpu().numpy() - host["center"]).max())
    print(f"rgb {err_rgb:.3e} (bound {REDUCE_CENTER_BOUND}), center {err_c:.3e} (bound {REDUCE_CENTER_BOUND} + 2^-23)")
    assert err_rgb < REDUCE_CENTER_BOUND and err_c < REDUCE_CENTER_BOUND + 2.0 ** -23
    # and bit for bit the set-wide table's rows, centres mirrored
    t = {k: v.cpu().numpy() for k, v in ps.object_table(eng, "cuda", kc, colors).items()}
    assert ps.object_table(eng, "cuda", kc, colors) is ps.object_table(eng, "cuda", kc, colors)
    for k, v in R.gather_rows(t, np.arange(ps.n_objects), np.repeat(codes, counts)).items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------------------- refusals
def _patterned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(G.PATTERN_BYTE)
    return t


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == G.PATTERN_BYTE).all()) for t in tensors)


@pytest.mark.parametrize("what,match", [("id -1", r"object_ids\[2\] = -1"), ("id n", r"object_ids\[2\] = 12"), ("mirror 4", r"mirror\[1\] = 4")])
def test_bad_rows_are_refused_and_nothing_is_written(eng, pts, what, match):
    ids, mirror = np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 3, 1, 2], dtype=np.uint8)
    if what.startswith("id"):
        ids[2] = -1 if what == "id -1" else 12
    else:
        mirror[1] = 4
    d = {k: dev(v) for k, v in table(12, 2).items()}
    for n_out, call in ((2, lambda: eng.sample_object_points_mirrored(*pts["dev"], ids, None, mirror, seed=SEED)),
                        (5, lambda: eng.gather_object_rows(d, ids, mirror))):
        with G.guarded_outputs(E, partly_written=tuple(range(n_out))) as g:
            with pytest.raises(E.T2LError, match=match):
                call()
            torch.cuda.synchronize()
            assert g.count == n_out
            for guard in g.guards:
                assert guard.unwritten_words() == guard.nbytes // 4
    # the engine serves the next call as if nothing had happened
    ok = np.array([0, 4], dtype=np.int32)
    pos, col = eng.sample_object_points_mirrored(*pts["dev"], ok, None, np.array([3, 0], dtype=np.uint8), seed=SEED)
    rpos, rcol = R.sample_rows(pts["xyz"], pts["rgb"], pts["poff"], ok, None, [3, 0], SEED, "fixed")
    assert R.diff_count(pos.cpu().numpy(), rpos) == 0 and R.diff_count(col.cpu().numpy(), rcol) == 0


def test_negative_counts_null_arrays_and_no_rows(eng, pts):
    """Through the C ABI itself (the wrappers derive the counts from the arrays): T2L_EINVAL = -1, patterned outputs untouched."""
    lib, h = eng.lib, eng._h
    xyz, rgb, poff = pts["dev"]
    ids, mirror = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.uint8)
    pos, col = _patterned((2, 256, 3), torch.float32), _patterned((2, 256, 3), torch.float32)
    stream = E._stream_ptr(eng.device)

    def sample(**kw):
        a = dict(xyz=xyz.data_ptr(), rgb=rgb.data_ptr(), poff=poff.data_ptr(), n_objects=12, ids=ids.ctypes.data, salts=None,
                 mirror=mirror.ctypes.data, n_rows=2, pos=pos.data_ptr(), col=col.data_ptr())
        a.update(kw)
        return lib.t2l_sample_object_points_mirrored(h, a["xyz"], a["rgb"], a["poff"], a["n_objects"], a["ids"], a["salts"], a["mirror"],
                                                     a["n_rows"], SEED, 0, 120.0, a["pos"], a["col"], stream)

    for kw, msg in [[dict(n_rows=-1), b"negative count"], [dict(n_objects=-1), b"negative count"]] + \
            [[{k: None}, b"null argument"] for k in ("xyz", "rgb", "poff", "ids", "pos", "col")]:
        assert sample(**kw) == -1 and msg in lib.t2l_last_error(h) and b"t2l_sample_object_points_mirrored" in lib.t2l_last_error(h), kw
    assert sample(n_rows=0) == 0 and sample(n_rows=0, ids=None, pos=None, col=None) == 0
    assert _untouched(pos, col)

    t = {k: dev(v) for k, v in table(12, 2).items()}
    out = {"class_idx": _patterned((2,), torch.int32), "color_idx": _patterned((2,), torch.int32), "rgb": _patterned((2, 3), torch.float32),
           "center": _patterned((2, 3), torch.float32), "n_pts": _patterned((2,), torch.float32)}
    order = ("class_idx", "color_idx", "rgb", "center", "n_pts")

    def gather(**kw):
        a = {k: t[k].data_ptr() for k in order}
        a.update({"out_" + k: out[k].data_ptr() for k in order})
        a.update(n_objects=12, ids=ids.ctypes.data, mirror=mirror.ctypes.data, n_rows=2)
        a.update(kw)
        return lib.t2l_gather_object_rows(h, *[a[k] for k in order], a["n_objects"], a["ids"], a["mirror"], a["n_rows"],
                                          *[a["out_" + k] for k in order], stream)

    for kw, msg in [[dict(n_rows=-1), b"negative count"], [dict(n_objects=-1), b"negative count"]] + \
            [[{k: None}, b"null argument"] for k in order + tuple("out_" + k for k in order) + ("ids",)]:
        assert gather(**kw) == -1 and msg in lib.t2l_last_error(h) and b"t2l_gather_object_rows" in lib.t2l_last_error(h), kw
    assert gather(n_rows=0) == 0 and gather(n_rows=0, ids=None, out_rgb=None) == 0
    assert _untouched(*out.values())
    assert gather() == 0 and sample() == 0  # the same arguments, unbroken, are served
    torch.cuda.synchronize()
    assert not _untouched(pos) and not _untouched(out["center"])
    empty = eng.gather_object_rows(t, np.zeros(0, np.int32), None)
    assert empty["rgb"].shape == (0, 3) and eng.sample_object_points_mirrored(xyz, rgb, poff, np.zeros(0, np.int32))[0].shape == (0, 256, 3)


# ---------------------------------------------------------------------------------------------------------------- model level
class HashText(torch.nn.Module):
    """Text-branch stand-in with a trainable table: the row of a text is its CRC32 modulo the table size."""

    def __init__(self, n=64, seed=1):
        super().__init__()
        self.table = torch.nn.Parameter(torch.randn(n, 256, generator=torch.Generator().manual_seed(seed)))

    def forward(self, texts):
        return self.table[torch.as_tensor([zlib.crc32(t.encode()) % len(self.table) for t in texts], device=self.table.device)]

    @property
    def device(self):
        return self.table.device


def make_model(embed, text=None):
    from tests.test_gpu_train_loop import TableText, _args
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    args = _args(class_embed=embed, color_embed=embed, pointnet_freeze=False, batch_size=4)
    model = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=text or TableText(8, 1))
    sd = dict(synth.make_object_branch_weights(3))  # the weights tests/test_gpu_train.py holds its bounds on (forward_backward_case)
    if not embed:
        sd.update(synth.make_pointnet_weights(2))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    for layer in model.obj_inter_module:  # the oracle below runs without dropout (tests/test_gpu_pointnet_train.py: _model)
        layer.dropout.p = layer.dropout1.p = layer.dropout2.p = 0.0
        layer.self_attn.dropout = 0.0
    return model.to("cuda"), sd, args


def dataset(embed, transform="fixed", aug_seed=3, seed=9):
    cells, poses = tiny_set(COUNTS)
    return K.Kitti360PoseDataset.from_records(cells, poses, object_points="ids", points=not embed, transform=transform, seed=seed,
                                              shuffle_hints=True, flip_poses=True, aug_rng=np.random.RandomState(aug_seed))


@pytest.mark.parametrize("embed", [True, False], ids=["embedding", "pointnet"])
def test_model_encodes_a_coarse_batch_like_the_host_flipped_cells(embed, monkeypatch):
    """``encode_objects`` under ``model.train()`` on ``coarse_batches`` batches (B = 4, 12 cells, every batch) against the float64
    oracle fed ``pack_cells`` of the cells the "sample" dataset would have handed on (mirrored on the host) — in PointNet++ mode with
    the engine's own features2 of the batch's device-sampled points. Bars: tests/test_gpu_train.py's output bound and ``assert_grads``;
    the inputs differ by at most one float32 step of a centre coordinate.
    Those bars are the engine's training step against the oracle, so the test stands on what they were established on: the weights
    ``make_object_branch_weights(3)``, point counts from ``synth.make_cells``, dLoss / d out = 0.05 N(0, 1). Measured on an MI355X:
    1.4e-6 at most from the oracle over the six batches. (On ``make_object_branch_weights(6)`` the same batches sit 1.6e-5 / 2.1e-5
    from the oracle and miss ``assert_grads`` on ``num_encoder.0.0.weight`` — through this path and through the parent's host path
    alike, the two outputs within 1.4e-7 of each other: a property of the training kernels on those weights, not of the batch path.)"""
    model, sd, _ = make_model(embed)
    model.train()
    ds = dataset(embed)
    sd64 = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    oe = model.object_encoder
    seen_codes, seen_counts = set(), set()
    f2 = []
    if not embed:
        eng = model.train_engine()
        real = eng.pointnet_features_train
        monkeypatch.setattr(eng, "pointnet_features_train", lambda *a, **k: f2.append(real(*a, **k)) or f2[-1])
    for batch in K.coarse_batches(ds, 4, "cuda", shuffle=True, seed=2):
        assert isinstance(batch["objects"], K.CoarseBatchObjects) and len(batch["objects"]) == 4
        assert (batch["object_points"][0] is None) == embed
        model.zero_grad(set_to_none=True)
        # dLoss / d out as tests/test_gpu_train.py draws it (0.05 N(0, 1)): assert_grads' absolute terms are sized for that scale
        R_out = (0.05 * torch.randn(4, 256, generator=torch.Generator().manual_seed(len(seen_counts)))).cuda()
        out = model.encode_objects(batch["objects"], batch["object_points"])
        (out * R_out).sum().backward()
        host_cells = [R.host_flipped_cell(c, m).objects for c, m in zip(batch["cells"], batch["mirror"])]
        packed = dict(packing.pack_cells(host_cells, oe.known_classes, oe.known_colors))
        if not embed:
            packed["pn_feat"] = f2[-1].detach().cpu().numpy()
            assert packed["pn_feat"].shape == (int(packed["offsets"][-1]), 256)
        ref_out, info = OT.encode_cells_train(packed, sd64, embed, embed, grad_out=R_out.cpu().numpy().astype(np.float64))
        err = float(np.abs(out.detach().cpu().numpy() - ref_out).max())
        print(f"embed={embed} counts {packed['counts'].tolist()} codes {batch['mirror']}: max |out - oracle| {err:.3e}")
        assert err < TRAIN_OUTPUT_BOUND
        params = dict(model.named_parameters())
        assert all(params[n].grad is not None for n in info["grads"]), [n for n in info["grads"] if params[n].grad is None]
        assert_grads({n: (params[n], params[n].grad) for n in info["grads"]}, info["grads"])
        seen_codes.update(batch["mirror"])
        seen_counts.update(packed["counts"].tolist())
    assert seen_counts == set(COUNTS) and len(seen_codes) >= 3


# ---------------------------------------------------------------------------------------------------------------- epoch loop
def test_two_epochs_through_train_epoch(monkeypatch):
    from text2loc_amd import coarse, plumbing
    from text2loc_amd.losses import ContrastiveLoss
    from text2loc_amd.optim import Adam

    torch.manual_seed(0)
    model, _, args = make_model(False, text=HashText())
    ds = dataset(False, transform="rotate_normalize")
    calls = {"pack_cells_gpu": 0, "gather": 0}
    real_pack, real_gather = packing.pack_cells_gpu, packing.PackedCellSet.gather_rows

    def counting_pack(*a, **k):
        calls["pack_cells_gpu"] += 1
        return real_pack(*a, **k)

    def counting_gather(self, *a, **k):
        calls["gather"] += 1
        return real_gather(self, *a, **k)

    monkeypatch.setattr(packing, "pack_cells_gpu", counting_pack)
    monkeypatch.setattr(packing.PackedCellSet, "gather_rows", counting_gather)
    assert plumbing.packing is packing
    batches = K.coarse_batches(ds, 4, "cuda", shuffle=True, seed=5, engine=model.engine())
    assert len(batches) == 3 and batches.dataset is ds
    opt, crit = Adam(model, lr=1e-3), ContrastiveLoss(temperature=0.1)
    bn = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm1d)}
    branch = next(n for n in bn if n.startswith("object_encoder.pos_encoder"))
    backbone = next(n for n in bn if n.startswith("object_encoder.pointnet.sa1"))
    for epoch in (1, 2):
        before = {n: int(bn[n].num_batches_tracked) for n in (branch, backbone)}
        loss, _ = coarse.train_epoch(model, batches, args, opt, crit)
        assert np.isfinite(loss) and ds._epoch == epoch
        assert int(bn[branch].num_batches_tracked) - before[branch] == 3      # once per batch
        assert int(bn[backbone].num_batches_tracked) - before[backbone] == 12  # once per cell, as the reference's per-cell calls
    assert calls == {"pack_cells_gpu": 0, "gather": 6}

    def point_rows(epoch):
        d = dataset(False, transform="rotate_normalize")
        d.set_epoch(epoch)
        return [(b["texts"], b["mirror"], torch.cat([p["pos"] for p in b["object_points"]]), torch.cat([p["x"] for p in b["object_points"]]))
                for b in K.coarse_batches(d, 4, "cuda", shuffle=True, seed=5)]

    e1, e2, again = point_rows(1), point_rows(2), point_rows(1)
    for a, b in zip(e1, again):  # the same (dataset seed, seed, epoch): the same batches, every bit
        assert a[0] == b[0] and a[1] == b[1] and same_bits(a[2], b[2]) and same_bits(a[3], b[3])
    assert [a[0] for a in e1] != [b[0] for b in e2]  # another epoch: another order ...
    assert not any(a[2].shape == b[2].shape and torch.equal(a[2], b[2]) for a in e1 for b in e2)  # ... and fresh draws
