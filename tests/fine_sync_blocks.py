"""TEST INFRASTRUCTURE — the phased BatchNorm of the fine step's cross-rank statistics (csrc/fine_train.hip: k_bn_stats_fwd /
k_bn_apply_fwd / k_bn_stats_bwd / k_bn_apply_bwd, run through csrc/fine_train_blocks.hip: t2l_blk_ft_bn_sync_fwd / _bwd with the ranks
emulated as PARTS of the rows) against the float64 reference of the WHOLE row set: tests/test_fine_sync_blocks_cpu.py,
tests/test_gpu_fine_sync_blocks.py; profiles/fine_train_blocks.md. References, cases and the bounds' constants are those of
tests/fine_train_blocks.py (bn_fwd_ref / bn_bwd_ref, C_BN_FWD, C_BN_BWD); two things differ from the one-launch kernels and are derived
here, on top of those bounds, never in their place:

One-pass variance.  The statistics launch cannot centre on a mean it does not know yet, so a slot carries s = Σ y and q = Σ y² in
float64 and the apply launch forms var = q / M - (s / M)². The operands are float32, so every y² is exact in float64; what is left is
the summation (M 2^-53 relative for each of q and s, whatever the order or the split into parts — the parts' sums are added in float64
too), which reaches var through q / M and twice through mean², and three roundings (two divisions, the subtraction), all relative to
s2 = q / M = var + mean²:

    |d var| <= (3 M + 3) 2^-53 s2 =: e_var,        e_rel = e_var / (2 (var + eps))       (rstd = (var + eps)^-1/2)
    |d rstd| += rstd e_rel     |d x̂| += |x̂| e_rel     |d out| += |g| |x̂| e_rel     |d rv| += 0.1 e_var M / (M - 1)

With |mean| = 100 std and M = 128 this is e_rel = 2e-10 — a thousandth of the 3u the bound of rstd already has; an exactly constant
column c (var = 0, s2 = c², eps alone under the root) gets e_rel = 2e-9 c², below u for |c| < 5. ``ONEPASS_SHARE`` holds the terms to a
quarter of the bound they are added to in every case of this tier (the CPU half asserts it).

Parameter gradients from parts.  dg / db receive one float32 addition per part: part p's float64 sum is rounded to float32
(u |part_p|) and added to the running value (u |run_p|):

    |d dg| <= u Σ_p (|part_p| + |run_p|) + M 2^-52 Σ |dz x̂|            (for one part: <= 2u (|dg0| + |Σ|), the one-launch bound)

The tier's factor C = 2 applies to both.
"""
import numpy as np

from tests import fine_train_blocks as B

U, C, F32 = B.U, B.C, B.F32
COLS = (64, 128)
KINDS = ("plain", "offset", "constant")
# rows -> the splits of them into consecutive parts ((M,): the phased form alone)
SPLITS = {128: ((64, 64), (127, 1), (3, 1, 124), (128,)), 2: ((1, 1),)}
ONEPASS_SHARE = 0.25  # the derived one-pass terms stay below this share of the bound they are added to


def onepass_terms(Y, g, rv):
    """the additions to bn_fwd_ref's tolerances: dict xhat, out, rstd, rv"""
    M = Y.shape[0]
    mean = Y.mean(axis=0)
    var = ((Y - mean) ** 2).mean(axis=0)
    e_var = (3 * M + 3) * 2.0 ** -53 * (var + mean ** 2)
    e_rel = e_var / (2 * (var + B.BN_EPS))
    rstd = 1.0 / np.sqrt(var + B.BN_EPS)
    xhat = (Y - mean) * rstd
    out = {"xhat": C * np.abs(xhat) * e_rel, "out": C * np.abs(g) * np.abs(xhat) * e_rel, "rstd": C * rstd * e_rel}
    if rv is not None:
        out["rv"] = C * B.BN_MOM * e_var * M / max(M - 1, 1)
    return out


def sync_fwd_ref(Y, g, b, rm, rv):
    """{name: (ref, tol)} of the phased forward over ALL rows of Y, whatever the split"""
    ref = B.bn_fwd_ref(Y, g, b, rm, rv)
    add = onepass_terms(Y, g, rv)
    return {k: (r, t + add[k] if k in add else t) for k, (r, t) in ref.items()}


def sync_bwd_ref(dout, out, xhat, rstd, g, dg0, db0, rows):
    """{name: (ref, tol)} of the phased backward: dy as bn_bwd_ref over all rows; dg / db with one float32 addition per part"""
    M = dout.shape[0]
    ref = B.bn_bwd_ref(dout, out, xhat, rstd, g, dg0, db0)
    dz = np.where(out > 0, dout, 0.0)
    res = {"dy": ref["dy"]}
    dbl = M * 2.0 ** -52
    for key, v0, terms in (("dg", dg0, dz * xhat), ("db", db0, dz)):
        if v0 is None:
            continue
        run, tol, r0 = v0.astype(np.float64).copy(), np.zeros_like(v0, dtype=np.float64), 0
        for n in rows:
            part = terms[r0:r0 + n].sum(axis=0)
            run = run + part
            tol += C * U * (np.abs(part) + np.abs(run))
            r0 += n
        res[key] = (ref[key][0], tol + dbl * np.abs(terms).sum(axis=0))
    return res


# ---- the kernels' arithmetic in numpy (float32 where they use float32, float64 sums): what a correct device run may return, and
# the mutants a wrong one would
def phased_fwd(Y, rows, g, b, rm, rv, mut=None):
    f = lambda a: np.asarray(a, F32)
    Y32 = f(Y)
    r0 = 0
    stats = []
    for n in rows:  # statistics launch per part: float64 sums of float32 operands
        y = Y32[r0:r0 + n].astype(np.float64)
        stats.append((y.sum(axis=0), (y * y).sum(axis=0), float(n)))
        r0 += n
    s, q, cnt = (sum(x[i] for x in stats) for i in range(3))  # the exchange
    res = {"xhat": np.empty_like(Y32), "out": np.empty_like(Y32)}
    r0 = 0
    for p, n in enumerate(rows):
        sp, qp, cp = stats[p] if mut == "no_exchange" else (s, q, cnt)
        if mut == "local_count":
            cp = float(n)
        mean = sp / cp
        var = np.maximum(qp / cp - mean * mean, 0.0)
        if mut == "f32_sums":
            y = Y32
            m32 = y.mean(axis=0, dtype=F32)
            mean, var = m32.astype(np.float64), np.maximum(((y * y).mean(axis=0, dtype=F32) - m32 * m32).astype(np.float64), 0.0)
        rstd = F32(1.0) / np.sqrt(f(var) + F32(B.BN_EPS), dtype=F32)
        mf = f(mean)
        xh = (Y32[r0:r0 + n] - mf) * rstd
        res["xhat"][r0:r0 + n] = xh
        res["out"][r0:r0 + n] = np.maximum(xh * f(g) + f(b), F32(0))
        if p == 0:
            res["rstd"] = rstd
            if rm is not None:
                res["rm"] = (F32(1) - F32(0.1)) * f(rm) + F32(0.1) * mf
            if rv is not None:
                res["rv"] = (F32(1) - F32(0.1)) * f(rv) + F32(0.1) * f(var * cp / max(cp - 1.0, 1.0))
        r0 += n
    return {k: v.astype(np.float64) for k, v in res.items()}


def phased_bwd(dout, out, xhat, rstd, g, dg0, db0, rows, mut=None):
    f = lambda a: np.asarray(a, F32)
    dz = np.where(out > 0, f(dout), F32(0))
    stats, r0 = [], 0
    dg, db = (None if dg0 is None else f(dg0).copy()), (None if db0 is None else f(db0).copy())
    for n in rows:
        z = dz[r0:r0 + n].astype(np.float64)
        sd, sdx = z.sum(axis=0), (z * f(xhat)[r0:r0 + n].astype(np.float64)).sum(axis=0)
        stats.append((sd, sdx, float(n)))
        if dg is not None and not (mut == "first_part_grads" and r0 > 0):
            dg = dg + f(sdx)
        if db is not None and not (mut == "first_part_grads" and r0 > 0):
            db = db + f(sd)
        r0 += n
    sd, sdx, cnt = (sum(x[i] for x in stats) for i in range(3))
    dy = np.empty_like(dz)
    r0 = 0
    for p, n in enumerate(rows):
        a, bx, c = stats[p] if mut == "no_exchange" else (sd, sdx, cnt)
        Mg = F32(c)
        k = f(g) * f(rstd) / Mg
        dy[r0:r0 + n] = k * (Mg * dz[r0:r0 + n] - f(a) - f(xhat)[r0:r0 + n] * f(bx))
        r0 += n
    res = {"dy": dy.astype(np.float64)}
    if dg is not None:
        res["dg"] = dg.astype(np.float64)
    if db is not None:
        res["db"] = db.astype(np.float64)
    return res


def load_blocks():
    """tests/fine_train_blocks.load_blocks plus this tier's wrapper"""
    import ctypes as Ct

    lib = B.load_blocks()
    p, i = Ct.c_void_p, Ct.c_int
    lib.t2l_blk_ft_bn_sync_fwd.restype, lib.t2l_blk_ft_bn_sync_fwd.argtypes = i, [p, Ct.POINTER(Ct.c_int32), i, i, p, p, p, p, p, p]
    lib.t2l_blk_ft_bn_sync_bwd.restype, lib.t2l_blk_ft_bn_sync_bwd.argtypes = i, [p, p, p, p, p, Ct.POINTER(Ct.c_int32), i, i, p, p, p]
    return lib
