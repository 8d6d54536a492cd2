"""GPU tier of the PointNet++ block tests: the eval-mode backbone through the product's own launch path
(t2l_pointnet_features of a context made through the dev library libt2l_blocks.so), then every level buffer of that call copied out
through csrc/pointnet_blocks.hip and held against the float64 stage references and derived bounds of tests/pointnet_blocks.py:
bit-equal centres at the three levels, every element of x1, x2, x3, f0, f1 and features2 within its tolerance, each stage fed the
kernel's own output of the stage before.

Outputs are carved from buffers patterned with 0xA5 between halos (tests/guards.py): the halos must keep their pattern and every
payload word must be written. Each test prints its worst err / tol per stage as `PNBLOCK ...` lines (pytest -s); the MI355X figures
are in profiles/pointnet_blocks.md."""
import ctypes

import numpy as np
import pytest

from tests import guards
from tests import pointnet_blocks as PB

pytestmark = pytest.mark.gpu

ARM_OPTIONS = {"split": (0, 0), "f16": (0, 1), "f32": (1, 0)}  # (encoder_f32, encoder_f16)
SHAPES = {"p1": (128, 3), "x1": (128, 64), "p2": (64, 3), "x2": (64, 128), "p3": (32, 3), "x3": (32, 256), "f0": (1024,), "f1": (512,)}


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return PB.load_blocks()


def make_engine(lib, sd):
    from text2loc_amd.engine import Engine

    e = Engine(0, lib=lib)
    e.load_weights(sd, class_embed=False, color_embed=False)
    return e


@pytest.fixture(scope="module")
def sd():
    return PB.weights(0)


@pytest.fixture(scope="module")
def eng(lib, sd):
    e = make_engine(lib, sd)
    yield e
    e.close()


def set_arm(eng, arm, loops):
    f32, f16 = ARM_OPTIONS[arm]
    eng.set_option("encoder_f32", f32)
    eng.set_option("encoder_f16", f16)
    eng.set_option("pointnet_pyg_self_loops", 1 if loops else 0)


def fresh(*shape, dtype=None):
    """an output the door must write whole: payload and halos hold the 0xA5 pattern"""
    import torch

    buf, lo, nbytes, view = guards._carve(shape, dtype or torch.float32, "cuda")
    buf.fill_(guards.PATTERN_BYTE)
    view._guard = guards.Guard(buf, lo, nbytes, view, "empty")
    return view


def ok(lib, rc):
    if rc == -2:  # the HIP runtime reported an error: nothing more is launched on this device by this session
        pytest.exit(f"GPU error in the block tier: {lib.t2l_blk_last_error().decode()}", returncode=3)
    assert rc == 0, f"rc {rc}: {lib.t2l_blk_last_error().decode()}"


def run_levels(eng, lib, pos, rgb, off, first=0, count=None):
    """one t2l_pointnet_features call, then the level buffers of objects [first, first + count) -> ({name: numpy}, flags)"""
    import torch

    n = pos.shape[0]
    count = n - first if count is None else count
    f2 = eng.pointnet_features(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), off)
    torch.cuda.synchronize()
    assert f2.shape == (n, 256)
    outs = {k: fresh(count, *s) for k, s in SHAPES.items()}
    flags = fresh(count, dtype=torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ok(lib, lib.t2l_blk_pointnet_levels(eng._h, n, first, count, *[ptr(outs[k]) for k in SHAPES], ptr(flags)))
    guards.check_halos(*outs.values(), flags)
    for k, t in list(outs.items()) + [("flags", flags)]:
        assert t._guard.unwritten_words() == 0, f"{k}: words of the copy were never written"
    lv = {k: t.cpu().numpy() for k, t in outs.items()}
    lv["f2"] = f2[first:first + count].cpu().numpy()
    return lv, flags.cpu().numpy()


def hold(lv, pos, rgb, off, sd, loops, arm_of, what):
    r, op = PB.hold_all(lv, pos, rgb, off, sd, loops, arm_of)
    arm = arm_of if isinstance(arm_of, str) else "mixed"
    for k, v in r.items():
        print(f"PNBLOCK {k} {arm} loops={int(loops)} {what}: err/tol {v:.4g}")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what} ({arm}, self loops {loops}): err / tol {bad}"
    return op


# ---- every stage of every arm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loops", [True, False], ids=["loops", "noloops"])
@pytest.mark.parametrize("arm", ["split", "f16", "f32"])
def test_every_stage_of_every_arm(eng, lib, sd, arm, loops):
    pos, rgb, off = PB.table_fixture()
    set_arm(eng, arm, loops)
    lv, flags = run_levels(eng, lib, pos, rgb, off)
    op = hold(lv, pos, rgb, off, sd, loops, arm, "table")
    assert not flags.any() and op.max() < PB.WATCH / 2
    assert (lv["f2"] > 0).mean() > 0.2  # not a dead network


# ---- object counts around the launch geometry ---------------------------------------------------------------------------------
COUNT_OFFSETS = {33: [0, 1, 1, 30, 33]}  # a cell of one object, an EMPTY cell in the middle, a cell of 29, a cell of 3


@pytest.mark.parametrize("n_obj", [1, 3, 4, 5, 8, 9, 33])
def test_object_counts_around_the_launch_geometry(eng, lib, sd, n_obj):
    """pn_fps_kernel's four objects per workgroup, pn_self_ws_kernel's eight tiles per round, pn_ga_ws_kernel's four waves, the 32-row
    blocks of lin1 / lin2"""
    pos, rgb, off = PB.count_fixture(n_obj, 100 + n_obj, COUNT_OFFSETS.get(n_obj))
    set_arm(eng, "split", True)
    lv, flags = run_levels(eng, lib, pos, rgb, off)
    hold(lv, pos, rgb, off, sd, True, "split", f"n_obj={n_obj}")
    assert not flags.any()


# ---- geometry fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["split", "f16", "f32"])
def test_geometry_fixtures(eng, lib, sd, arm):
    """radius boundary, saturation counts, chunk placement, ties and the line (their conditions: tests/test_pointnet_blocks_cpu.py)"""
    pos, rgb, off, _ = PB.geometry_fixture()
    set_arm(eng, arm, True)
    lv, flags = run_levels(eng, lib, pos, rgb, off)
    hold(lv, pos, rgb, off, sd, True, arm, "geometry")
    assert not flags.any()


@pytest.mark.parametrize("arm", ["split", "f32"])
def test_raw_cell_frame_coordinates(eng, lib, sd, arm):
    pos, rgb, off = PB.cell_frame_fixture()
    assert PB.in_radius(pos, PB.centres(pos), 0.2).sum(axis=-1).max() > 32  # the saturating regime really occurs
    set_arm(eng, arm, True)
    lv, _ = run_levels(eng, lib, pos, rgb, off)
    hold(lv, pos, rgb, off, sd, True, arm, "cell-frame")


def test_sampling_kernel_alone_on_the_tie_fixtures(lib):
    """pn_fps_kernel<NS> on raw pointers at the three levels' sizes: centres bit-equal, flagged objects left alone"""
    import torch

    pos, _, _, _ = PB.geometry_fixture()
    src = pos
    for ns in (256, 128, 64):
        want = PB.centres(src)
        flags = np.zeros(len(src), np.int32)
        flags[1] = 1
        d_src, d_flags = guards.guarded(torch.from_numpy(src).cuda(), guards.NAN), guards.guarded(torch.from_numpy(flags).cuda(), 0)
        dst = fresh(len(src), ns // 2, 3)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        ok(lib, lib.t2l_blk_pn_fps(ptr(d_src), ptr(dst), ptr(d_flags), len(src), ns))
        guards.check_halos(d_src, d_flags, dst)
        got = dst.cpu().numpy()
        keep = flags == 0
        assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32)), ns
        assert (got[~keep].view(np.int32) == guards.PATTERN_WORD).all()  # the flagged object's centres were not touched
        src = want
    assert lib.t2l_blk_pn_fps(ptr(d_src), ptr(dst), None, 6, 96) == -1 and b"ns must be" in lib.t2l_blk_last_error()


# ---- the magnitude watch --------------------------------------------------------------------------------------------------------
def test_magnitude_watch_flags_and_arms(lib):
    """flags as expected; a flagged object's stages from the flagging level on are the f32 kernels' (held at the f32 arm's bound), the
    rest the split kernels'; centres bit-equal for both; the object flagged at level 2 keeps its split-arm x1"""
    pos, rgb, off, msd, expect, first = PB.magnitude_fixture()
    e = make_engine(lib, msd)
    try:
        set_arm(e, "split", True)
        lv, flags = run_levels(e, lib, pos, rgb, off)
    finally:
        e.close()
    assert flags.tolist() == expect.tolist(), flags
    arm_of = [["f32" if first[o] and s + 1 >= first[o] else "split" for o in range(len(expect))] for s in range(4)]
    assert arm_of[0][3] == "split" and arm_of[1][3] == "f32"
    assert np.isfinite(lv["f2"]).all()
    hold(lv, pos, rgb, off, msd, True, arm_of, "magnitude")


# ---- persistent workgroups wrapping -----------------------------------------------------------------------------------------------
def test_persistent_workgroups_go_round_more_than_once(eng, lib, sd):
    """2,112 objects: pn_self_ws_kernel goes round three times at level 2 and twice at level 3, pn_ga_ws_kernel three times. Cells are
    independent, so the references run on cells from the start, the middle and the end; only those objects' slices are copied out."""
    n = 2112
    pos, rgb, off = PB.count_fixture(n, 77)
    assert n > 8 * 256 and n > 2 * 4 * 256
    set_arm(eng, "split", True)
    for c in (0, len(off) // 2, len(off) - 2):
        lo, hi = int(off[c]), int(off[c + 1])
        lv, flags = run_levels(eng, lib, pos, rgb, off, lo, hi - lo)
        hold(lv, pos[lo:hi], rgb[lo:hi], np.array([0, hi - lo], np.int32), sd, True, "split", f"wrap objects {lo}..{hi}")
        assert not flags.any()


# ---- the door refuses what it cannot serve ----------------------------------------------------------------------------------------
def test_the_door_refuses_instead_of_copying_out_of_bounds(lib, sd):
    import torch

    e = make_engine(lib, sd)
    try:
        buf = fresh(2, 128, 3)
        ptr = ctypes.c_void_p(buf.data_ptr())
        nulls = [None] * 9
        assert lib.t2l_blk_pointnet_levels(e._h, 2, 0, 2, ptr, *nulls[1:]) == -1
        assert b"no t2l_pointnet_features call" in lib.t2l_blk_last_error()
        pos, rgb, off = PB.count_fixture(2, 5)
        e.pointnet_features(torch.from_numpy(pos).cuda(), torch.from_numpy(rgb).cuda(), off)
        for n_obj, lo, cnt, msg in ((3, 0, 2, b"last call served 2"), (2, 1, 2, b"first + count"), (2, -1, 1, b"first + count"),
                                    (2, 0, 0, b"first + count"), (2, 2, 1, b"first + count")):
            assert lib.t2l_blk_pointnet_levels(e._h, n_obj, lo, cnt, ptr, *nulls[1:]) == -1
            assert msg in lib.t2l_blk_last_error(), lib.t2l_blk_last_error()
        assert buf._guard.unwritten_words() == buf.numel()  # nothing was copied by a refused call
        ok(lib, lib.t2l_blk_pointnet_levels(e._h, 2, 1, 1, ptr, *nulls[1:]))
        guards.check_halos(buf)
        assert np.array_equal(buf[0].cpu().numpy(), PB.centres(pos)[1]) and buf._guard.unwritten_words() == buf[1].numel()
    finally:
        e.close()
