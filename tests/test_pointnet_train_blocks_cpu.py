"""CPU tier of the PointNet++ training block tests: the references and bounds of tests/pointnet_train_blocks.py tell right
from wrong before a GPU is involved. A float32 numpy restatement of every block — with the kernels' wave, tile and workgroup structure
where the bound depends on it — stays inside its bound; the inputs are conditioned as the module promises; every mutant (the ways these
kernels go subtly wrong) leaves the bound or the exact check at the case that targets it; the case lists reach every launcher path at
256 CUs; the wrappers refuse shapes and null pointers outside their contract (that needs the dev library, not a device)."""
import ctypes

import numpy as np
import pytest

from oracle import arith
from tests import pointnet_blocks as PB
from tests import pointnet_train_blocks as PT

F32 = np.float32
CUS = 8  # a small machine for the restatements: the same paths (one, two, three tiles per wave) at a sixteenth of the rows


def worst(got, ref, tol):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def rejected(got, want, names):
    """the mutant leaves the bound of at least one of the named outputs"""
    return any(worst(got[k], *want[k]) > 1.0 for k in names)


# ---- case lists -------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_launcher_path_at_256_cus():
    got = PT.paths_reached(256)
    assert not PT.PATHS_AT_256 - got, sorted(PT.PATHS_AT_256 - got)
    M2, M3 = PT.rows2_big_rows(256)
    assert PT.rows2_plan(M2 - 77, 32, 32, 0, False, 256)[2] == 32  # below it every wave has one tile
    assert PT.rows2_plan(M2, 32, 32, 0, False, 256)[2] == 64 and PT.rows2_plan(M3, 128, 128, 2, True, 256)[2] >= 96
    big = [c for c in PT.rows2_cases(256) if c[5] > 8 * 32 * 256]
    assert {(K, N, f) for _, K, N, f, _, _, _ in big} == set(PT.ROWS2_NARROW)  # the wide shapes stay small
    assert len(PT.tn2_plan(8229, 256, 160, 256)) == 2  # K = 160: a block of 3 k tiles and a narrower one of 2, each its own launch


# ---- acceptance: float32 restatements inside the bounds; conditioning holds -------------------------------------------------------------
@pytest.mark.parametrize("ar", PT.ARITHS)
def test_rows2_restatement_is_accepted(ar):
    top = 0.0
    for kind, K, N, fused, cols, M, lay in PT.rows2_cases(CUS):
        if K * N > 256 * 256 and M not in (33, 600):
            continue  # (the widest shapes at two row counts: the bound's form does not depend on M)
        c = PT.Rows2Case(kind, K, N, fused, cols, M, lay, ar, CUS)
        if fused:
            assert not PT.fused_ambiguous(c.A, c.mean, c.rg, c.beta, c.row_cell, ar).any()
            assert np.array_equal(c.A, PT.store(c.A, ar))
        want, got = PT.rows2_reference(c), PT.rows2_restatement(c)
        for k in want:
            r = worst(got[k], *want[k])
            top = max(top, r)
            assert r <= 1.0, f"{kind} K={K} N={N} M={M} cells={lay} arith={ar} {k}: {r:.3f}"
    print(f"rows2 arith {ar}: float32 restatement worst err / tol {top:.4f}")


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_tn2_restatement_is_accepted(ar):
    for N, K, k_real, fused in PT.TN2_SHAPES:
        for M in PT.tn2_rows(N, K, CUS):
            c = PT.Tn2Case(N, K, k_real, fused, M, ar)
            if fused:
                assert not PT.fused_ambiguous(c.X, c.mean, c.rg, c.beta, c.row_cell, ar).any()
            want, got = PT.tn2_reference(c), PT.tn2_restatement(c, CUS)
            for k in want:
                assert worst(got[k], *want[k]) <= 1.0, f"N={N} K={K} M={M} arith={ar} {k}"


def finalize32(acc, cnt, gamma, rm0, rv0):
    """pt_bn_finalize_kernel in its own arithmetic: float64 statistics from the sums, float32 from the casts on"""
    n = cnt.astype(np.float64)[:, None]
    m = acc[:, 0] / n
    var = np.maximum(acc[:, 1] / n - m * m, 0.0)
    mf = m.astype(F32)
    vu = (var * (n / np.maximum(n - 1.0, 1.0))).astype(F32)
    rs = (F32(1.0) / np.sqrt((var.astype(F32) + F32(1e-5)).astype(F32))).astype(F32)
    rg = (rs * gamma.astype(F32)).astype(F32)
    rm, rv, mom = rm0.astype(F32), rv0.astype(F32), F32(0.1)
    for cell in range(len(cnt)):
        rm = ((F32(1) - mom) * rm + mom * mf[cell]).astype(F32)
        rv = ((F32(1) - mom) * rv + mom * vu[cell]).astype(F32)
    return {"mean": mf, "rstd": rs, "rg": rg, "run_mean": rm, "run_var": rv}


FWD = ((32, 32, False, (2, 31, 32, 33, 502)), (32, 64, True, (700, 800)), (96, 128, False, (40,) * 9), (128, 128, True, (1100,)))


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_block_fwd_restatement_is_accepted(ar):
    for K, C, fused, sizes in FWD:
        c = PT.BlockFwdCase(K, C, fused, sizes, ar, CUS)
        want = PT.block_fwd_reference(c)
        r = PT.rows2_restatement(c.prod)
        got = finalize32(r["acc"], c.cnt, c.gamma, c.rm0, c.rv0)
        got["y"] = r["C"]
        for k in want:
            assert worst(got[k], *want[k]) <= 1.0, f"K={K} C={C} cells={sizes} arith={ar} {k}: {worst(got[k], *want[k]):.3f}"
        # the apply kernel from the tensors it reads
        a_ref, a_tol = PT.bn_apply_reference(got["y"], got["mean"].astype(np.float64), got["rstd"].astype(np.float64), c.gamma, c.beta,
                                             c.prod.row_cell, ar)
        rc = c.prod.row_cell
        a32 = np.maximum(((got["y"].astype(F32) - got["mean"][rc]) * got["rstd"][rc] * c.gamma.astype(F32) + c.beta.astype(F32)), F32(0))
        assert worst(PT.store(a32.astype(np.float64), ar), a_ref, a_tol) <= 1.0


def bwd32(dv, y, mean, rstd, gamma, cnt, term_cell, dgamma0, dbeta0):
    """the backward's three launches in float32: sums per cell (float32 partials), the coefficient tables, the element-wise form"""
    n_cells, C = len(cnt), dv.shape[1]
    f = lambda x: np.asarray(x, dtype=np.float64).astype(F32)
    t2 = (f(dv) * (f(y) - f(mean)[term_cell]) * f(rstd)[term_cell]).astype(F32)
    S = np.zeros((n_cells, 2, C))
    for cell in range(n_cells):
        sel = term_cell == cell
        S[cell, 0], S[cell, 1] = f(dv)[sel].sum(axis=0, dtype=F32), t2[sel].sum(axis=0, dtype=F32)
    nn = cnt.astype(F32)[:, None]
    k1 = (f(gamma) * f(rstd) / nn * S[:, 0].astype(F32)).astype(F32)
    k2 = (f(gamma) * f(rstd) / nn * f(rstd) * S[:, 1].astype(F32)).astype(F32)
    return {"k1": k1, "k2": k2, "dbeta": f(dbeta0) + S[:, 0].sum(axis=0).astype(F32), "dgamma": f(dgamma0) + S[:, 1].sum(axis=0).astype(F32)}


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_block_bwd_restatements_are_accepted(ar):
    f = lambda x: np.asarray(x, dtype=np.float64).astype(F32)
    for C, sizes, stored_a in ((32, (2, 31, 567), True), (64, (700, 800), False), (128, (100,) * 9, False), (32, (1024, 1024), True)):
        c = PT.BnRowsCase(C, sizes, stored_a, ar)
        if not stored_a:  # the recomputed sign is unambiguous, and the float32 expression agrees
            pre, mag = PT.fused_pre(c.y, c.mean, c.rg, c.beta, c.row_cell)
            assert (np.abs(pre) > PT.fused_band(mag)).all()
            pre32 = ((f(c.y) - f(c.mean)[c.row_cell]).astype(np.float64) * c.rg[c.row_cell] + c.beta).astype(F32)
            assert np.array_equal(pre32 > 0, c.mask)
        else:
            assert ((c.a == 0) & (c.d != 0)).any()  # planted zeros under a live gradient
        want = PT.bn_rows_reference(c)
        dv = np.where(c.mask, c.d, 0.0)
        got = bwd32(dv, c.y, c.mean, c.rstd, c.gamma, c.cnt, c.row_cell, c.dgamma0, c.dbeta0)
        rc = c.row_cell
        d32 = (f(c.gamma) * f(c.rstd)[rc] * f(dv) - got["k1"][rc] - (f(c.y) - f(c.mean)[rc]) * got["k2"][rc]).astype(F32)
        got["d"] = PT.store(d32.astype(np.float64), ar)
        for k in want:
            assert worst(got[k], *want[k]) <= 1.0, f"rows C={C} cells={sizes} arith={ar} {k}: {worst(got[k], *want[k]):.3f}"
    for C, n_obj, nd, n_cells in ((32, 1, 128, 1), (64, 3, 64, 3), (128, 9, 32, 9), (64, 6, 1, 3)):
        c = PT.GroupCase(C, n_obj, nd, n_cells, ar)
        assert not PT.group_decisions(c).any()
        seg = PT.segmax_reference(c)
        # the float32 forward makes the reference's decisions
        rc = c.row_cell
        v32 = np.maximum(((f(c.y) - f(c.mean)[rc]) * f(c.rstd)[rc] * f(c.gamma) + f(c.beta)).astype(F32), F32(0))
        arg32 = np.stack([c.goff[g] + v32[c.goff[g]:c.goff[g + 1]].argmax(axis=0) for g in range(c.G)])
        assert np.array_equal(arg32, seg["arg"])
        x32 = v32[arg32, np.arange(C)[None, :]]
        assert worst(x32, *seg["xout"]) <= 1.0
        if c.dup is not None:
            assert (seg["arg"][c.dup] == c.goff[c.dup]).all()  # duplicate rows: the first wins
            assert (seg["xout"][0][c.neg] == 0).all() and (seg["arg"][c.neg] == c.goff[c.neg]).all()  # all negative: xout 0, first row
        assert (np.diff(c.goff) == 1).any() or c.G < 33
        want = PT.bn_groups_reference(c, seg)
        cell_of_group = c.cell_of_obj[np.arange(c.G) // nd]
        dvg = np.where(x32 > 0, c.dxout, 0.0)
        got = bwd32(dvg, seg["ysel"], c.mean, c.rstd, c.gamma, c.cnt, cell_of_group, c.dgamma0, c.dbeta0)
        hit = (seg["arg"][c.row_group] == np.arange(c.E)[:, None]) & (v32 > 0)
        dv = np.where(hit, c.dxout[c.row_group], 0.0)
        d32 = (f(c.gamma) * f(c.rstd)[rc] * f(dv) - got["k1"][rc] - (f(c.y) - f(c.mean)[rc]) * got["k2"][rc]).astype(F32)
        got["d"] = PT.store(d32.astype(np.float64), ar)
        for k in want:
            assert worst(got[k], *want[k]) <= 1.0, f"groups C={C} nd={nd} arith={ar} {k}: {worst(got[k], *want[k]):.3f}"


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
def test_mutant_n_minus_1_in_k1_k2():
    c = PT.BnRowsCase(32, (2, 31, 567), True, 0)
    want, bad = PT.bn_rows_reference(c), PT.bn_rows_reference(c, "n_minus_1")
    assert rejected({k: v[0] for k, v in bad.items()}, want, ("k1",)) and rejected({k: v[0] for k, v in bad.items()}, want, ("k2",))
    assert rejected({k: v[0] for k, v in bad.items()}, want, ("d",))


def test_mutant_running_statistics():
    c = PT.BlockFwdCase(32, 32, False, (2, 31, 32, 33, 502), 0, CUS)
    want = PT.block_fwd_reference(c)
    biased = PT.block_fwd_reference(c, "biased_running_var")
    assert worst(biased["run_var"][0], *want["run_var"]) > 1.0
    once = PT.block_fwd_reference(c, "one_update_per_batch")
    assert worst(once["run_mean"][0], *want["run_mean"]) > 1.0 and worst(once["run_var"][0], *want["run_var"]) > 1.0


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_mutants_of_the_sums_in_the_product_epilogue(ar):
    M2, M3 = PT.rows2_big_rows(CUS)
    inside = PT.Rows2Case("stat", 32, 32, False, 0, 33, "inside", ar, CUS)  # a cell boundary inside a tile
    assert worst(PT.rows2_restatement(inside, mutant="straddle_first")["acc"], *PT.rows2_reference(inside)["acc"]) > 1.0
    for M in (M2, M3):  # a boundary between two tiles of one wave
        wave = PT.Rows2Case("stat", 32, 64, True, 0, M, "wave", ar, CUS)
        assert wave.rpw >= 64
        want = PT.rows2_reference(wave)
        assert worst(PT.rows2_restatement(wave, mutant="no_flush")["acc"], *want["acc"]) > 1.0
        assert worst(PT.rows2_restatement(wave, mutant="straddle_first")["acc"], *want["acc"]) > 1.0


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_mutant_scatter_keeps_one_row_per_source(ar):
    for K, N, cols in PT.ROWS2_SCAT:
        c = PT.Rows2Case("scat", K, N, False, cols, 600, "one", ar, CUS)
        assert np.bincount(c.scat_src).max() == 33 and (np.bincount(c.scat_src, minlength=c.scat_rows) == 0).any()
        assert worst(PT.rows2_restatement(c, mutant="scat_keep_one")["dst"], *PT.rows2_reference(c)["dst"]) > 1.0


def test_mutants_of_the_arg_max_and_the_mask():
    c = PT.GroupCase(64, 3, 64, 3, 0)
    first, last = PT.segmax_reference(c), PT.segmax_reference(c, last_wins=True)
    assert (first["arg"][c.dup] != last["arg"][c.dup]).all() and (first["arg"][c.neg] != last["arg"][c.neg]).all()
    r = PT.BnRowsCase(32, (2, 31, 567), True, 0)
    want, bad = PT.bn_rows_reference(r), PT.bn_rows_reference(r, "ge_mask")
    assert rejected({k: v[0] for k, v in bad.items()}, want, ("d",)) and rejected({k: v[0] for k, v in bad.items()}, want, ("dbeta",))


@pytest.mark.parametrize("ar", PT.ARITHS)
def test_mutants_of_tn2(ar):
    for N, K, k_real, fused in PT.TN2_SHAPES:
        rows = PT.tn2_rows(N, K, CUS)
        c = PT.Tn2Case(N, K, k_real, fused, rows[-1], ar)  # two steps per workgroup, the last one partial
        want = PT.tn2_reference(c)
        assert rejected(PT.tn2_restatement(c, CUS, "drop_partial"), want, ("dW",)), f"N={N} K={K}"
        assert rejected(PT.tn2_restatement(PT.Tn2Case(N, K, k_real, fused, rows[1], ar), CUS, "drop_partial"),
                        PT.tn2_reference(PT.Tn2Case(N, K, k_real, fused, rows[1], ar)), ("dW",))
        if any(p[2] > 1 for p in PT.tn2_plan(c.M, N, K, CUS)):
            assert rejected(PT.tn2_restatement(c, CUS, "db_every_block"), want, ("db",)), f"N={N} K={K}"
        if k_real < K:
            assert rejected(PT.tn2_restatement(c, CUS, "write_pad"), want, ("dW",)), f"N={N} K={K}"
    assert any(p[2] > 1 for N, K, _, _ in PT.TN2_SHAPES for p in PT.tn2_plan(1000, N, K, 256))
    if ar == arith.EXACT:
        # at 256 CUs the two narrow shapes sum over 65,531 and 131,067 rows: the trailing partial step is still seen (Tn2Case weighs it)
        for N, K, k_real, fused in ((64, 32, 32, True), (32, 32, 6, False)):
            c = PT.Tn2Case(N, K, k_real, fused, PT.tn2_rows(N, K, 256)[-1], ar)
            assert worst(PT.tn2_restatement(c, 256, "drop_partial")["dW"], *PT.tn2_reference(c)["dW"]) > 4.0


def test_mutant_relative_position_against_the_previous_centre():
    pos, rgb, offsets = PB.count_fixture(3, 3)
    ctr, nbr33, cnt_g, _ = PT.index_reference(pos, offsets, PB.RADII[0], 1)
    goff = np.concatenate([[0], np.cumsum(cnt_g)]).astype(np.int32)
    co = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)
    src, row_group, row_cell = PT.compact_reference(nbr33, goff, 128, co)
    args = (rgb.reshape(-1, 3).astype(np.float64), pos.reshape(-1, 3), ctr.reshape(-1, 3), src, row_group, 3, 32, 0)
    good, bad = PT.gather_reference(*args), PT.gather_reference(*args, prev_centre=True)
    assert not np.array_equal(good, bad) and np.array_equal(good[:, 6:], np.zeros_like(good[:, 6:]))
    # the compacted tables are the oracle's edges: per cell, source rows relative to the cell's first object
    from oracle import t2l_oracle_pointnet_train as OPT

    sel, edges, _, new_pos = OPT.build_edges(pos, offsets, True)[0]
    assert np.array_equal(new_pos.view(np.uint32), ctr.view(np.uint32))
    base = np.repeat(offsets[:-1], np.diff(offsets))
    for o in range(pos.shape[0]):
        for t in (0, 1, 127):
            g = o * 128 + t
            assert np.array_equal(src[goff[g]:goff[g + 1]] - base[o] * 256, edges[o][t])


@pytest.mark.parametrize("wrong,ar", [(arith.SPLIT_NO_LOHI, arith.SPLIT), (arith.BF16_TRUNC, arith.BF16)])
def test_mutant_operand_arithmetic(wrong, ar):
    for K, N, fused in PT.ROWS2_STAT[:4]:
        c = PT.Rows2Case("stat", K, N, fused, 0, 257, "tile", ar, CUS)
        want = PT.rows2_reference(c)
        assert worst(PT.rows2_reference(c, product=wrong)["C"][0], *want["C"]) > 1.0 or ar == arith.BF16
        assert worst(PT.rows2_reference(c, product=wrong)["acc"][0], *want["acc"]) > 1.0, f"K={K} N={N}"
    for N, K, k_real, fused in PT.TN2_SHAPES[:3]:
        t = PT.Tn2Case(N, K, k_real, fused, 257, ar)
        assert worst(PT.tn2_reference(t, product=wrong)["dW"][0], *PT.tn2_reference(t)["dW"]) > 1.0, f"N={N} K={K}"


# ---- refusals: shapes and null pointers, before anything is launched (no device is needed) ----------------------------------------------
@pytest.fixture(scope="module")
def blocks():
    return PT.load_blocks()


def test_wrappers_refuse_what_is_outside_their_contract(blocks):
    L = blocks
    n = None
    x = ctypes.c_void_p(256)  # a non-null pointer that is never followed: every check below comes before the first access

    def refused(rc, reason):
        assert rc == -1 and reason in L.t2l_blk_last_error(), (rc, reason, L.t2l_blk_last_error())

    def rows2(M=64, N=32, K=64, ar=0, A=x, W=x, bias=x, C=x, fm=n, fr=n, fb=n, rc=n, cells=0, acc=n, ss=n, sd=n, cols=0, srows=0):
        return L.t2l_blk_pn_rows2(A, W, bias, C, M, N, K, ar, fm, fr, fb, rc, cells, acc, ss, sd, cols, srows)

    refused(rows2(ar=3), b"arith must be 0, 1 or 2")
    refused(rows2(ar=-1), b"arith must be 0, 1 or 2")
    refused(rows2(M=0), b"1 <= M")
    refused(rows2(K=40), b"multiple of 16")
    refused(rows2(K=16), b"multiple of 16")
    refused(rows2(N=48), b"multiple of 32")
    refused(rows2(K=512, N=2048, acc=x, rc=x, cells=1), b"C > 1024")
    refused(rows2(K=64, N=64), b"not a layer shape")
    refused(rows2(K=64, N=32, acc=x, rc=x, cells=1), b"not a layer shape")  # (a plain shape with statistics)
    refused(rows2(K=32, N=64, fm=x, fr=x, fb=x, rc=x, cells=1), b"not a layer shape")  # the fused operand without statistics ...
    refused(rows2(K=128, N=128, fm=x, fr=x, fb=x, rc=x, cells=1), b"fused operand without statistics")  # ... at a shape both lists hold
    refused(rows2(A=n), b"null pointer")
    refused(rows2(W=n), b"null pointer")
    refused(rows2(K=64, C=n), b"null pointer")
    refused(rows2(K=32, acc=x, cells=1), b"null pointer (row_cell)")
    refused(rows2(K=32, N=64, acc=x, rc=x, cells=1, fm=x), b"needs a_mean, a_rg and a_beta")
    refused(rows2(K=128, N=64, ss=x), b"come together")
    refused(rows2(K=128, N=64, ss=x, sd=x, cols=65, srows=4), b"scat_cols")
    refused(rows2(K=32, acc=x, rc=x, cells=0), b"n_cells >= 1")

    def tn2(M=64, N=32, K=32, kr=6, ldw=6, ar=0, dY=x, X=x, dW=x, fm=n, fr=n, fb=n, rc=n, cells=0):
        return L.t2l_blk_pn_tn2(dY, X, dW, x, M, N, K, kr, ldw, fm, fr, fb, rc, cells, ar)

    refused(tn2(ar=5), b"arith must be 0, 1 or 2")
    refused(tn2(M=0), b"1 <= M")
    refused(tn2(K=24), b"multiple of 16")
    refused(tn2(N=40), b"multiple of 32")
    refused(tn2(N=64, K=64), b"not a layer shape")
    refused(tn2(N=64, K=32, kr=32, ldw=32), b"not a layer shape")  # (64, 32) exists with the fused operand only
    refused(tn2(kr=0), b"k_real")
    refused(tn2(kr=33, ldw=33), b"k_real")
    refused(tn2(kr=6, ldw=5), b"ldw < k_real")
    refused(tn2(dW=n), b"null pointer")
    refused(tn2(N=64, K=32, kr=32, ldw=32, fm=x, fr=x, fb=x), b"null pointer")

    def fwd(E=64, K=32, C=32, ar=0, X=x, cnt=x, cells=1, fm=n, fr=n, fb=n):
        return L.t2l_blk_pn_block_fwd(X, x, E, K, C, ar, x, x, x, x, x, x, cnt, cells, x, x, n, x, x, x, fm, fr, fb)

    refused(fwd(ar=3), b"arith must be 0, 1 or 2")
    refused(fwd(E=0), b"1 <= E")
    refused(fwd(cells=0), b"n_cells >= 1")
    refused(fwd(K=40), b"multiple of 16")
    refused(fwd(C=16), b"multiple of 32")
    refused(fwd(K=512, C=2048), b"C > 1024")
    refused(fwd(K=64, C=32), b"not a layer shape")
    refused(fwd(X=n), b"null pointer")
    refused(fwd(cnt=n), b"null pointer")
    refused(fwd(K=32, C=64, fm=x), b"needs f_mean, f_rg and f_beta")

    def bwd(E=64, C=32, ar=0, d=x, a=x, rg=n, rc=x, cells=1, dxout=n, arg=n, G=0, nd=0):
        return L.t2l_blk_pn_block_bwd(d, x, a, E, C, ar, x, x, rg, x, x, x, x, rc, x, cells, x, x, x, dxout, arg, x, x, x, x, G, nd)

    refused(bwd(ar=3), b"arith must be 0, 1 or 2")
    refused(bwd(E=0), b"1 <= E")
    refused(bwd(C=48), b"power of two")
    refused(bwd(C=2048), b"power of two")
    refused(bwd(C=16), b"power of two")
    refused(bwd(d=n), b"null pointer")

    def seg(G=4, E=8, C=32, nd=2, ar=0, y=x, cells=1):
        return L.t2l_blk_pn_segmax(y, x, G, E, C, nd, x, cells, x, x, x, x, x, x, x, ar)

    refused(seg(ar=7), b"arith must be 0, 1 or 2")
    refused(seg(C=96), b"power of two")
    refused(seg(G=0), b"1 <= G")
    refused(seg(G=9, E=8), b"1 <= G <= E")
    refused(seg(G=5, nd=2), b"multiple of nd")
    refused(seg(y=n), b"null pointer")

    def rows(sa=1, G=4, nd=2, per=0, cells=1, E=8, n_src=16, cin=3, kp=32, ar=0, X=x, nbr=x):
        return L.t2l_blk_pn_rows(sa, nbr, x, G, nd, per, x, cells, E, x, x, x, x, x, x, n_src, cin, kp, X, ar)

    refused(rows(ar=3), b"arith must be 0, 1 or 2")
    refused(rows(cin=5), b"not a layer shape")
    refused(rows(cin=64, kp=64), b"kp must be")
    refused(rows(E=0), b"1 <= E")
    refused(rows(G=3), b"multiple of nd")
    refused(rows(X=n), b"null pointer")
    refused(rows(nbr=n), b"null pointer")

    def index(n_obj=2, ns=256, nd=128, radius=0.2, pos=x):
        return L.t2l_blk_pn_index(pos, n_obj, ns, nd, radius, x, 1, x, x, x)

    refused(index(ns=100), b"ns must be 256, 128 or 64")
    refused(index(n_obj=0), b"n_obj >= 1")
    refused(index(nd=300), b"nd <= ns")
    refused(index(radius=0.0), b"radius > 0")
    refused(index(radius=float("nan")), b"radius > 0")
    refused(index(pos=n), b"null pointer")

    def layout(op=0, rows_=4, a=6, b=32, ar=0, src=x, dst=x):
        return L.t2l_blk_pn_layout(op, src, dst, rows_, a, b, ar)

    refused(layout(op=4), b"op must be")
    refused(layout(ar=3), b"arith must be 0, 1 or 2")
    refused(layout(rows_=0), b"1 <= rows")
    refused(layout(op=0, a=40, b=32), b"pad needs")
    refused(layout(op=0, a=6, b=40), b"pad needs")
    refused(layout(op=1, a=0), b"transpose needs")
    refused(layout(op=2, a=33, b=32), b"slice needs")
    refused(layout(src=n), b"null pointer")
    refused(layout(op=3, dst=n), b"null pointer")
