"""GPU tier of the PointNet++ training block tests: every kernel of csrc/pointnet_train.h and csrc/gemm_rows2.h as the
step's own launchers launch it, ONE launch at a time through the dev library (csrc/train_blocks.hip: t2l_blk_pn_*), each output held
element by element against the float64 references and derived bounds of tests/pointnet_train_blocks.py — index tables, arg-max rows and
the layout kernels bit for bit.

Conventions of tests/test_gpu_train_blocks.py: inputs sit between NaN halos, outputs are carved from 0xA5-patterned buffers
(tests/guards.py) — halos must stay intact, every payload word of a written output must be written — and outputs the kernels ADD to
(acc, dW, db, dgamma, dbeta, the scattered gradient) start from non-zero contents. rc == -2 ends the session's GPU work. Each test
prints its worst err / tol as a `BLOCK ...` line (pytest -s); the MI355X figures are in profiles/pointnet_train_blocks.md."""
import numpy as np
import pytest

from oracle import arith
from tests import guards
from tests import pointnet_blocks as PB
from tests import pointnet_train_blocks as PT
from tests.test_gpu_train_blocks import Worst, check_buffers, ok, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "the block tier needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    return PT.load_blocks()


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def tdtype(kind):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64, "i32": torch.int32}[kind]


def edge(ar):
    """the storage type of an edge-row tensor"""
    return "bf16" if ar == arith.BF16 else "f32"


def dev(a, kind="f32"):
    """a guarded device copy of an input (NaN halos; zero — an in-range value — around an index table)"""
    import torch

    if kind == "i32":
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()
        return guards.guarded(t, 0)
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(tdtype(kind)).cuda()
    return guards.guarded(t, guards.NAN)


def fresh(*shape, kind="f32"):
    import torch

    buf, lo, nbytes, view = guards._carve(shape, tdtype(kind), "cuda")
    buf.fill_(guards.PATTERN_BYTE)
    view._guard = guards.Guard(buf, lo, nbytes, view, "empty")
    return view


def host(t):
    t = t.detach()
    return (t.double() if t.dtype.is_floating_point else t).cpu().numpy()


def ratio(t, ref, tol):
    """worst err / tol; where the bound is zero the value must be exactly the reference's"""
    got = host(t).astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def same(t, ref):
    return np.array_equal(host(t).reshape(np.asarray(ref).shape), np.asarray(ref, dtype=host(t).dtype))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- rows2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", PT.ARITHS)
def test_rows2(lib, n_cu, ar):
    """every shape, row count and cell layout of PT.rows2_cases: C, the BatchNorm sums, the scattered output"""
    wc, ws, wd = Worst(f"pn_rows2 C arith={ar}"), Worst(f"pn_rows2 sums arith={ar}"), Worst(f"pn_rows2 scatter arith={ar}")
    for kind, K, N, fused, cols, M, lay in PT.rows2_cases(n_cu):
        c = PT.Rows2Case(kind, K, N, fused, cols, M, lay, ar, n_cu)
        want = PT.rows2_reference(c)
        what = f"{kind} K={K} N={N} fused={fused} M={M} cells={lay} tp={c.tp} rpw={c.rpw}"
        A, W = dev(c.A, edge(ar)), dev(c.W)
        bias = None if c.bias is None else dev(c.bias)
        ins, outs = [A, W] + ([bias] if bias is not None else []), []
        f_mean = f_rg = f_beta = rc = acc = src = dst = None
        if fused:
            f_mean, f_rg, f_beta = dev(c.mean), dev(c.rg), dev(c.beta)
            ins += [f_mean, f_rg, f_beta]
        if kind == "stat":
            rc, acc = dev(c.row_cell, "i32"), dev(c.acc0, "f64")
            ins.append(rc)
            outs.append(acc)
        C = None
        if kind == "scat":
            src, dst = dev(c.scat_src, "i32"), dev(c.dst0)
            ins.append(src)
            outs.append(dst)
        else:
            C = fresh(M, N, kind=edge(ar))
            outs.append(C)
        ok(lib, lib.t2l_blk_pn_rows2(ptr(A), ptr(W), ptr(bias), ptr(C), M, N, K, ar, ptr(f_mean), ptr(f_rg), ptr(f_beta), ptr(rc), c.n_cells,
                                     ptr(acc), ptr(src), ptr(dst), cols, getattr(c, "scat_rows", 0)))
        check_buffers(ins, outs, what)
        if kind == "scat":
            wd.hold(ratio(dst, *want["dst"]), what)
            continue
        wc.hold(ratio(C, *want["C"]), what + " C")
        if kind == "stat":
            got = host(acc)
            assert np.array_equal(got[:, :, N:], c.acc0[:, :, N:]), f"{what}: acc changed beyond column N"
            ws.hold(ratio(acc[:, :, :N], *want["acc"]), what + " acc")
    wc.report()
    ws.report()
    wd.report()


# ---- tn2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", PT.ARITHS)
def test_tn2(lib, n_cu, ar):
    """dW [N][k_real] (a write at k >= k_real would land in the next row) and db, both from non-zero contents"""
    w, wb = Worst(f"pn_tn2 dW arith={ar}"), Worst(f"pn_tn2 db arith={ar}")
    for N, K, k_real, fused in PT.TN2_SHAPES:
        for M in PT.tn2_rows(N, K, n_cu):
            c = PT.Tn2Case(N, K, k_real, fused, M, ar)
            want = PT.tn2_reference(c)
            what = f"N={N} K={K} k_real={k_real} fused={fused} M={M}"
            dY, X, dW, db = dev(c.dY, edge(ar)), dev(c.X, edge(ar)), dev(c.dW0), dev(c.db0)
            ins = [dY, X]
            f_mean = f_rg = f_beta = rc = None
            if fused:
                f_mean, f_rg, f_beta, rc = dev(c.mean), dev(c.rg), dev(c.beta), dev(c.row_cell, "i32")
                ins += [f_mean, f_rg, f_beta, rc]
            ok(lib, lib.t2l_blk_pn_tn2(ptr(dY), ptr(X), ptr(dW), ptr(db), M, N, K, k_real, k_real, ptr(f_mean), ptr(f_rg), ptr(f_beta), ptr(rc),
                                       c.n_cells, ar))
            check_buffers(ins, (dW, db), what)
            w.hold(ratio(dW, *want["dW"]), what + " dW")
            wb.hold(ratio(db, *want["db"]), what + " db")
    w.report()
    wb.report()


# ---- one layer forward ----------------------------------------------------------------------------------------------------------
# (K, C, fused, stored a, cell sizes): cells of 2, 31, 32 and 33 rows; 9 cells (more than the finalize kernel's 8 cell lanes); one cell;
# the global level's first layer, which stores a
BLOCK_FWD = ((32, 32, False, False, (2, 31, 32, 33, 502)), (32, 64, True, False, (700, 800)), (96, 128, False, False, (40,) * 9),
             (128, 128, True, False, (1100,)), (288, 512, False, True, (300, 157)), (512, 1024, False, False, (64, 33, 95)))


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_block_fwd(lib, n_cu, ar):
    w, wa = Worst(f"pn_block_fwd arith={ar}"), Worst(f"pn_block_fwd a arith={ar}")
    for K, C, fused, stored_a, sizes in BLOCK_FWD:
        c = PT.BlockFwdCase(K, C, fused, sizes, ar, n_cu)
        p = c.prod
        want = PT.block_fwd_reference(c)
        what = f"K={K} C={C} fused={fused} cells={sizes}"
        X, W, bias, gamma, beta = dev(p.A, edge(ar)), dev(p.W), dev(p.bias), dev(c.gamma), dev(c.beta)
        rm, rv, rc, cnt = dev(c.rm0), dev(c.rv0), dev(p.row_cell, "i32"), dev(c.cnt, "i32")
        ins = [X, W, bias, gamma, beta, rc, cnt]
        f_mean = f_rg = f_beta = None
        if fused:
            f_mean, f_rg, f_beta = dev(p.mean), dev(p.rg), dev(p.beta)
            ins += [f_mean, f_rg, f_beta]
        acc = fresh(c.n_cells, 2, 1024, kind="f64")
        y = fresh(c.E, C, kind=edge(ar))
        a = fresh(c.E, C, kind=edge(ar)) if stored_a else None
        mean, rstd, rg = fresh(c.n_cells, C), fresh(c.n_cells, C), fresh(c.n_cells, C)
        ok(lib, lib.t2l_blk_pn_block_fwd(ptr(X), ptr(W), c.E, K, C, ar, ptr(bias), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(rc), ptr(cnt),
                                         c.n_cells, ptr(acc), ptr(y), ptr(a), ptr(mean), ptr(rstd), ptr(rg), ptr(f_mean), ptr(f_rg), ptr(f_beta)))
        check_buffers(ins, [acc, y, mean, rstd, rg, rm, rv] + ([a] if stored_a else []), what)
        for name, t in (("y", y), ("mean", mean), ("rstd", rstd), ("rg", rg), ("run_mean", rm), ("run_var", rv)):
            w.hold(ratio(t, *want[name]), f"{what} {name}")
        if stored_a:  # the apply kernel against ITS inputs: the y, mean and rstd the launches before it wrote
            wa.hold(ratio(a, *PT.bn_apply_reference(host(y), host(mean), host(rstd), c.gamma, c.beta, p.row_cell, ar)), what + " a")
    w.report()
    wa.report()


# ---- one layer backward, rows form -------------------------------------------------------------------------------------------------
# (C, cell sizes): E on both sides of kStatRows = 1024, a cell boundary inside a 1024-row block and none, 1 / 3 / 9 cells, C = 32 (the
# half-idle grid column)
BWD_ROWS = ((32, (2, 31, 567)), (32, (1024, 1024)), (64, (700, 800)), (128, (100,) * 9), (1024, (1030,)), (128, (1024, 500, 1500)))


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_block_bwd_rows(lib, ar):
    w, wt = Worst(f"pn_block_bwd rows d arith={ar}"), Worst(f"pn_block_bwd rows tables arith={ar}")
    for C, sizes in BWD_ROWS:
        for stored_a in (True, False):
            c = PT.BnRowsCase(C, sizes, stored_a, ar)
            want = PT.bn_rows_reference(c)
            what = f"C={C} cells={sizes} stored_a={stored_a}"
            d, y = dev(c.d, edge(ar)), dev(c.y, edge(ar))
            a = dev(c.a, edge(ar)) if stored_a else None
            mean, rstd, rg, gamma, beta = dev(c.mean), dev(c.rstd), dev(c.rg), dev(c.gamma), dev(c.beta)
            dgamma, dbeta, rc, cnt = dev(c.dgamma0), dev(c.dbeta0), dev(c.row_cell, "i32"), dev(c.cnt, "i32")
            acc, k1, k2 = fresh(c.n_cells, 2, 1024, kind="f64"), fresh(c.n_cells, C), fresh(c.n_cells, C)
            ok(lib, lib.t2l_blk_pn_block_bwd(ptr(d), ptr(y), ptr(a), c.E, C, ar, ptr(mean), ptr(rstd), None if stored_a else ptr(rg), ptr(gamma),
                                             ptr(beta), ptr(dgamma), ptr(dbeta), ptr(rc), ptr(cnt), c.n_cells, ptr(acc), ptr(k1), ptr(k2), None,
                                             None, None, None, None, None, 0, 0))
            check_buffers([y, mean, rstd, rg, gamma, beta, rc, cnt] + ([a] if stored_a else []), [d, dgamma, dbeta, acc, k1, k2], what)
            w.hold(ratio(d, *want["d"]), what + " d")
            for name, t in (("k1", k1), ("k2", k2), ("dgamma", dgamma), ("dbeta", dbeta)):
                wt.hold(ratio(t, *want[name]), f"{what} {name}")
    w.report()
    wt.report()


# ---- segmax and the backward's groups form -----------------------------------------------------------------------------------------
# (C, objects, nd, cells): every nd of the backbone, groups of 1 .. 33 rows, 1 / 3 / 9 cells
GROUPS = ((32, 1, 128, 1), (64, 3, 64, 3), (128, 9, 32, 9), (1024, 9, 1, 3), (64, 6, 1, 3))


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_segmax_and_block_bwd_groups(lib, ar):
    """pt_segmax_kernel: xout within its bound, arg and ysel exact (duplicate rows: the first wins; an all-negative group: xout 0, its
    first row). Then pn_block_bwd's groups form from those exact outputs."""
    ws, w, wt = Worst(f"pn_segmax arith={ar}"), Worst(f"pn_block_bwd groups d arith={ar}"), Worst(f"pn_block_bwd groups tables arith={ar}")
    for C, n_obj, nd, n_cells in GROUPS:
        c = PT.GroupCase(C, n_obj, nd, n_cells, ar)
        seg = PT.segmax_reference(c)
        what = f"C={C} objects={n_obj} nd={nd} cells={n_cells} E={c.E}"
        y, goff, co = dev(c.y, edge(ar)), dev(c.goff, "i32"), dev(c.cell_of_obj, "i32")
        mean, rstd, gamma, beta = dev(c.mean), dev(c.rstd), dev(c.gamma), dev(c.beta)
        xout, arg, ysel = fresh(c.G, C), fresh(c.G, C, kind="i32"), fresh(c.G, C)
        ok(lib, lib.t2l_blk_pn_segmax(ptr(y), ptr(goff), c.G, c.E, C, nd, ptr(co), n_cells, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(xout),
                                      ptr(arg), ptr(ysel), ar))
        check_buffers([y, goff, co, mean, rstd, gamma, beta], [xout, arg, ysel], what)
        assert same(arg, seg["arg"]), f"{what}: arg differs from the first maximum"
        assert np.array_equal(bits(host(ysel)), bits(seg["ysel"])), f"{what}: ysel is not y at arg"
        ws.hold(ratio(xout, *seg["xout"]), what + " xout")
        if c.neg is not None:
            assert (host(xout)[c.neg] == 0).all() and (host(arg)[c.neg] == c.goff[c.neg]).all()
        # backward, groups form, from the reference's forward outputs (xout as the float32 the forward hands on)
        want = PT.bn_groups_reference(c, seg)
        d = fresh(c.E, C, kind=edge(ar))
        b_xout, b_arg, b_ysel, dxout = dev(PT.f32(seg["xout"][0])), dev(seg["arg"], "i32"), dev(seg["ysel"]), dev(c.dxout)
        dgamma, dbeta, cnt = dev(c.dgamma0), dev(c.dbeta0), dev(c.cnt, "i32")
        acc, k1, k2 = fresh(n_cells, 2, 1024, kind="f64"), fresh(n_cells, C), fresh(n_cells, C)
        ok(lib, lib.t2l_blk_pn_block_bwd(ptr(d), ptr(y), None, c.E, C, ar, ptr(mean), ptr(rstd), None, ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta),
                                         None, ptr(cnt), n_cells, ptr(acc), ptr(k1), ptr(k2), ptr(dxout), ptr(b_arg), ptr(b_ysel), ptr(b_xout),
                                         ptr(goff), ptr(co), c.G, nd))
        check_buffers([y, mean, rstd, gamma, beta, cnt, dxout, b_arg, b_ysel, b_xout, goff, co], [d, dgamma, dbeta, acc, k1, k2], what)
        w.hold(ratio(d, *want["d"]), what + " d")
        for name, t in (("k1", k1), ("k2", k2), ("dgamma", dgamma), ("dbeta", dbeta)):
            wt.hold(ratio(t, *want[name]), f"{what} {name}")
    ws.report()
    w.report()
    wt.report()


# ---- row tables + gather -------------------------------------------------------------------------------------------------------------
def _index_fixture(which):
    if which == "geometry":
        pos, rgb, offsets, _ = PB.geometry_fixture()
        offsets = np.array([0, 3, 5, 6], dtype=np.int32)  # (every cell holds an object here: the product refuses an empty one)
    elif which == "cell_frame":
        pos, rgb, offsets = PB.cell_frame_fixture()
    else:
        pos, rgb, offsets = PB.count_fixture(5, 3)
    return pos, rgb, offsets


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_rows(lib, ar):
    """compact (from the reference's own ball-query table) or iota, then gather: tables and X bit for bit; cin 3 is the scalar path,
    64 and 256 the float4 path; with and without centres"""
    for which, self_loops, cin in (("geometry", 1, 3), ("cell_frame", 0, 64), ("count", 1, 64)):
        pos, rgb, offsets = _index_fixture(which)
        n, ns, nd = pos.shape[0], 256, 128
        ctr, nbr33, cnt_g, _ = PT.index_reference(pos, offsets, PB.RADII[0], self_loops)
        goff = np.concatenate([[0], np.cumsum(cnt_g)]).astype(np.int32)
        cell_of_obj = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)
        src, row_group, row_cell = PT.compact_reference(nbr33, goff, nd, cell_of_obj)
        E, G, kp = len(src), n * nd, (cin + 3 + 31) // 32 * 32
        x_src = rgb.reshape(n * ns, 3).astype(np.float64) if cin == 3 else PT.gauss((PT.SEED, 7, cin), n * ns, cin)
        want = PT.gather_reference(x_src, pos.reshape(-1, 3), ctr.reshape(-1, 3), src, row_group, cin, kp, ar)
        d_nbr, d_goff, d_co = dev(nbr33, "i32"), dev(goff, "i32"), dev(cell_of_obj, "i32")
        d_x, d_ps, d_pc = dev(x_src), dev(pos.reshape(-1, 3)), dev(ctr.reshape(-1, 3))
        o_src, o_rg, o_rc, X = fresh(E, kind="i32"), fresh(E, kind="i32"), fresh(E, kind="i32"), fresh(E, kp, kind=edge(ar))
        ok(lib, lib.t2l_blk_pn_rows(1, ptr(d_nbr), ptr(d_goff), G, nd, 0, ptr(d_co), len(offsets) - 1, E, ptr(o_src), ptr(o_rg), ptr(o_rc), ptr(d_x),
                                    ptr(d_ps), ptr(d_pc), n * ns, cin, kp, ptr(X), ar))
        what = f"compact {which} cin={cin} arith={ar}"
        check_buffers([d_nbr, d_goff, d_co, d_x, d_ps, d_pc], [o_src, o_rg, o_rc, X], what)
        assert same(o_src, src) and same(o_rg, row_group) and same(o_rc, row_cell), what + ": row tables"
        assert np.array_equal(bits(host(X)), bits(want)), what + ": X"
    for cin, n_obj, n_cells in ((256, 5, 2), (64, 3, 3)):  # the global level: 32 rows per object, no centres
        per, kp = 32, (cin + 3 + 31) // 32 * 32
        E, G = n_obj * per, n_obj
        cell_of_obj = (np.arange(n_obj) * n_cells // n_obj).astype(np.int32)
        x_src, pos_src = PT.gauss((PT.SEED, 8, cin), E, cin), PT.gauss((PT.SEED, 9, cin), E, 3)
        src = np.arange(E, dtype=np.int32)
        want = PT.gather_reference(x_src, pos_src, None, src, src // per, cin, kp, ar)
        d_co, d_x, d_ps = dev(cell_of_obj, "i32"), dev(x_src), dev(pos_src)
        o_goff, o_src, o_rg, o_rc = fresh(G + 1, kind="i32"), fresh(E, kind="i32"), fresh(E, kind="i32"), fresh(E, kind="i32")
        X = fresh(E, kp, kind=edge(ar))
        ok(lib, lib.t2l_blk_pn_rows(0, None, ptr(o_goff), G, 1, per, ptr(d_co), n_cells, E, ptr(o_src), ptr(o_rg), ptr(o_rc), ptr(d_x), ptr(d_ps), None,
                                    E, cin, kp, ptr(X), ar))
        what = f"iota cin={cin} arith={ar}"
        check_buffers([d_co, d_x, d_ps], [o_goff, o_src, o_rg, o_rc, X], what)
        assert same(o_goff, np.arange(G + 1) * per) and same(o_src, src) and same(o_rg, src // per) and same(o_rc, cell_of_obj[src // per]), what
        assert np.array_equal(bits(host(X)), bits(want)), what + ": X"


# ---- FPS + ball query ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", (1, 0))
def test_index(lib, self_loops):
    """all three levels (ns 256 / 128 / 64) chained on the REFERENCE's centres, on the eval tier's fixtures: 31 / 32 / 33 in-radius
    points, a point on the radius, the self-loop index in a cell's second object. pos_out, nbr33 and cnt_g bit for bit."""
    for which in ("geometry", "cell_frame", "count"):
        pos, _, offsets = _index_fixture(which)
        cur = pos
        for level, radius in enumerate(PB.RADII):
            n, ns, _ = cur.shape
            nd = ns // 2
            ctr, nbr33, cnt_g, base = PT.index_reference(cur, offsets, radius, self_loops)
            d_pos, d_base = dev(cur), dev(base, "i32")
            pos_out, o_nbr, o_cnt = fresh(n, nd, 3), fresh(n * nd, 33, kind="i32"), fresh(n * nd, kind="i32")
            ok(lib, lib.t2l_blk_pn_index(ptr(d_pos), n, ns, nd, float(np.float32(radius)), ptr(d_base), self_loops, ptr(pos_out), ptr(o_nbr),
                                         ptr(o_cnt)))
            what = f"{which} level {level + 1} self_loops={self_loops}"
            check_buffers([d_pos, d_base], [pos_out, o_nbr, o_cnt], what)
            assert np.array_equal(bits(host(pos_out)), bits(ctr)), what + ": centres"
            assert same(o_nbr, nbr33), what + ": nbr33"
            assert same(o_cnt, cnt_g), what + ": cnt_g"
            cur = ctr


# ---- layout kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", PT.ARITHS)
def test_layout(lib, ar):
    """pad, transpose, slice and relu-mask: exact permutations, copies and masks"""
    for rows, kin, kp in ((32, 6, 32), (128, 67, 96), (512, 259, 288)):
        W = PT.gauss((PT.SEED, 10, rows), rows, kin)
        d_W, Wp = dev(W), fresh(rows, kp)
        ok(lib, lib.t2l_blk_pn_layout(0, ptr(d_W), ptr(Wp), rows, kin, kp, ar))
        check_buffers([d_W], [Wp], f"pad {rows} {kin}")
        assert np.array_equal(bits(host(Wp)), bits(np.pad(W, ((0, 0), (0, kp - kin))))), f"pad {rows} x {kin} -> {kp}"
    for N, Kp in ((64, 32), (32, 96), (1024, 512), (33, 7)):
        W = PT.gauss((PT.SEED, 11, N), N, Kp)
        d_W, Wt = dev(W), fresh(Kp, N)
        ok(lib, lib.t2l_blk_pn_layout(1, ptr(d_W), ptr(Wt), N, Kp, 0, ar))
        check_buffers([d_W], [Wt], f"transpose {N} {Kp}")
        assert np.array_equal(bits(host(Wt)), bits(W.T)), f"transpose {N} x {Kp}"
    for rows, cin, kp in ((1, 256, 288), (257, 256, 288), (33, 3, 32)):
        dX = PT.store(PT.gauss((PT.SEED, 12, rows), rows, kp), ar)
        d_dX, out = dev(dX, edge(ar)), fresh(rows, cin)
        ok(lib, lib.t2l_blk_pn_layout(2, ptr(d_dX), ptr(out), rows, cin, kp, ar))
        check_buffers([d_dX], [out], f"slice {rows} {cin}")
        assert np.array_equal(bits(host(out)), bits(dX[:, :cin])), f"slice {rows} x {kp} -> {cin}"
    for n in (1, 255, 256, 257, 5000):
        f, d = PT.gauss((PT.SEED, 13, n), n), PT.gauss((PT.SEED, 14, n), n)
        f[::7] = 0.0
        f[3::11] = -0.0
        d_f, d_d = dev(f), dev(d)
        ok(lib, lib.t2l_blk_pn_layout(3, ptr(d_f), ptr(d_d), n, 0, 0, ar))
        check_buffers([d_f], [d_d], f"relu-mask {n}")
        assert np.array_equal(bits(host(d_d)), bits(np.where(f > 0, d, 0.0))), f"relu-mask n={n}"


# ---- table-content refusals ----------------------------------------------------------------------------------------------------------
def test_tables_outside_the_contract_are_refused(lib):
    """unsorted row_cell, a cnt mismatch, a one-row cell, goff with an empty group, arg / scat_src out of range: -1 with the reason,
    and nothing is launched (the outputs keep their pattern)"""
    C, sizes = 32, (5, 7)
    c = PT.BnRowsCase(C, sizes, True, 0)
    mean, rstd, gamma, beta = dev(c.mean), dev(c.rstd), dev(c.gamma), dev(c.beta)
    y, a = dev(c.y), dev(c.a)
    keep = []  # (every table handed over by pointer stays alive until the test ends)

    def tab(x, kind="f32"):
        keep.append(dev(x, kind))
        return ptr(keep[-1])

    def bwd_rows(row_cell, cnt, reason):
        d, dgamma, dbeta = fresh(c.E, C), fresh(C), fresh(C)
        acc, k1, k2 = fresh(2, 2, 1024, kind="f64"), fresh(2, C), fresh(2, C)
        rc = lib.t2l_blk_pn_block_bwd(ptr(d), ptr(y), ptr(a), c.E, C, 0, ptr(mean), ptr(rstd), None, ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta),
                                      tab(row_cell, "i32"), tab(cnt, "i32"), 2, ptr(acc), ptr(k1), ptr(k2), None, None, None, None, None,
                                      None, 0, 0)
        assert rc == -1 and reason in lib.t2l_blk_last_error(), (rc, reason, lib.t2l_blk_last_error())
        for t in (d, dgamma, dbeta, acc, k1, k2):
            assert t._guard.unwritten_words() == t._guard.nbytes // 4, f"{reason}: something was launched"

    unsorted = c.row_cell.copy()
    unsorted[[2, 8]] = unsorted[[8, 2]]
    bwd_rows(unsorted, c.cnt, b"not sorted")
    bwd_rows(np.where(np.arange(c.E) == c.E - 1, 2, c.row_cell), c.cnt, b"leaves [0, n_cells)")
    bwd_rows(c.row_cell, np.array([6, 6]), b"but the cell has")
    bwd_rows(PT.sizes_to_row_cell((11, 1)), np.array([11, 1]), b"fewer than 2 rows")

    g = PT.GroupCase(32, 2, 2, 2, 0, planted=False)
    seg = PT.segmax_reference(g)
    gy, gm, gr = dev(g.y), dev(g.mean), dev(g.rstd)

    def bwd_groups(goff, arg, reason):
        d, dgamma, dbeta = fresh(g.E, 32), fresh(32), fresh(32)
        acc, k1, k2 = fresh(2, 2, 1024, kind="f64"), fresh(2, 32), fresh(2, 32)
        rc = lib.t2l_blk_pn_block_bwd(ptr(d), ptr(gy), None, g.E, 32, 0, ptr(gm), ptr(gr), None, ptr(gamma), ptr(beta), ptr(dgamma), ptr(dbeta), None,
                                      tab(g.cnt, "i32"), 2, ptr(acc), ptr(k1), ptr(k2), tab(g.dxout), tab(arg, "i32"),
                                      tab(seg["ysel"]), tab(PT.f32(seg["xout"][0])), tab(goff, "i32"), tab(g.cell_of_obj, "i32"),
                                      g.G, g.nd)
        assert rc == -1 and reason in lib.t2l_blk_last_error(), (rc, reason, lib.t2l_blk_last_error())
        for t in (d, dgamma, dbeta, acc, k1, k2):
            assert t._guard.unwritten_words() == t._guard.nbytes // 4, f"{reason}: something was launched"

    bad_arg = seg["arg"].copy()
    bad_arg[1, 5] = g.E
    bwd_groups(g.goff, bad_arg, b"leaves the rows of its group")
    empty = g.goff.copy()
    empty[2] = empty[1]
    bwd_groups(empty, seg["arg"], b"a group with no row")
    short = g.goff.copy()
    short[-1] -= 1
    bwd_groups(short, seg["arg"], b"not at E")

    s = PT.Rows2Case("scat", 128, 64, False, 64, 33, "one", 0, 256)
    dst = fresh(s.scat_rows, 64)
    bad_src = s.scat_src.copy()
    bad_src[7] = s.scat_rows
    rc = lib.t2l_blk_pn_rows2(tab(s.A), tab(s.W), None, None, 33, 64, 128, 0, None, None, None, None, 0, None, tab(bad_src, "i32"),
                              ptr(dst), 64, s.scat_rows)
    assert rc == -1 and b"scat_src[7]" in lib.t2l_blk_last_error()
    assert dst._guard.unwritten_words() == dst._guard.nbytes // 4
