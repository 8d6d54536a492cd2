"""CPU tier: oracle/arith.py — the operand arithmetics the bf16 / split-bf16 training tests hold the kernels to (tests/test_gpu_train_arith.py) —
against torch's own bf16 conversion and the error bounds the kernels declare (gemm_f32.h:30-34), and the ``arith`` argument of the three
training oracles: 0 is the plain product of before, 1 / 2 move the results by what their arithmetic allows and no more."""
import numpy as np
import pytest
import torch

from oracle import arith as A
from oracle import t2l_oracle_pointnet_train as OPT
from oracle import t2l_oracle_text_train as OTT
from oracle import t2l_oracle_train as OT
from text2loc_amd import synth


def _bits(x64):
    return np.asarray(x64).astype(np.float32).view(np.uint32)


def _torch_bf16_bits(x32):
    return torch.from_numpy(x32).to(torch.bfloat16).to(torch.float32).numpy().view(np.uint32)


def _patterns(kind):
    rng = np.random.default_rng([7, len(kind)])
    if kind == "random":      # every finite bit pattern class, both signs
        u = rng.integers(0, 2 ** 32, size=200_000, dtype=np.uint64).astype(np.uint32)
        return u[(u & 0x7F800000) != 0x7F800000]
    if kind == "normal":      # values as they occur, over 60 decades
        return (rng.standard_normal(50_000) * 10.0 ** rng.uniform(-30, 30, 50_000)).astype(np.float32).view(np.uint32)
    if kind == "ties":        # exactly half-way between two bf16 values, kept lsb 0 and 1
        u = (rng.integers(0, 2 ** 16, 20_000).astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000)
        return u[(u & 0x7F800000) != 0x7F800000]
    if kind == "subnormal":
        return rng.integers(1, 0x00800000, 20_000).astype(np.uint32) | (rng.integers(0, 2, 20_000).astype(np.uint32) << np.uint32(31))
    if kind == "large":       # the top binade: some round up to infinity
        return (0x7F7F0000 + rng.integers(0, 0x10000, 20_000)).astype(np.uint32) | (rng.integers(0, 2, 20_000).astype(np.uint32) << np.uint32(31))
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "normal", "ties", "subnormal", "large"])
def test_bf16_rne_is_torch_bf16_bit_for_bit(kind):
    u = _patterns(kind)
    x32 = u.view(np.float32)
    got = _bits(A.bf16_rne(x32))
    assert np.array_equal(got, _torch_bf16_bits(x32))
    assert np.array_equal(got & np.uint32(0xFFFF), np.zeros_like(got))
    if kind == "ties":
        assert ((u >> np.uint32(16)) & np.uint32(1)).min() == 0 and ((u >> np.uint32(16)) & np.uint32(1)).max() == 1
        assert (((got >> np.uint32(16)) & np.uint32(1)) == 0).all()  # to even
    if kind == "large":
        assert np.isinf(A.bf16_rne(x32)).any() and np.isfinite(A.bf16_rne(x32)).any()


def test_bf16_rne_rounds_the_float32_value_and_keeps_specials():
    # float64 -> float32 first: 1 + 2^-8 + 2^-30 is 1 + 2^-8 in float32, a tie that goes to 1.0 (rounding the float64 directly: 1 + 2^-7)
    assert A.bf16_rne(np.array([1.0 + 2.0 ** -8 + 2.0 ** -30]))[0] == 1.0
    sp = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan])
    r = A.bf16_rne(sp)
    assert r[0] == np.inf and r[1] == -np.inf and r[2] == 0 and np.signbit(r[3]) and np.isnan(r[4])


def test_truncating_control_is_another_arithmetic():
    x = np.random.default_rng(1).standard_normal(100_000)
    t, r = A.bf16_trunc(x), A.bf16_rne(x)
    assert (np.abs(t) <= np.abs(x.astype(np.float32))).all()
    assert 0.4 < float((t != r).mean()) < 0.6


def test_split_bf16_reconstructs_to_2_16():
    x = _patterns("normal").view(np.float32).astype(np.float64)
    x = x[np.abs(x) > 1e-30]  # (lo of the smallest normals is subnormal: fewer bits)
    hi, lo = A.split_bf16(x)
    assert np.array_equal(hi, A.bf16_rne(x))
    assert np.array_equal(lo, A.bf16_rne(x.astype(np.float32) - hi.astype(np.float32)))
    assert (np.abs(x - (hi + lo)) <= 2.0 ** -16 * np.abs(x)).all()


def test_product_error_bounds():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((48, 200)) * 10.0 ** rng.uniform(-3, 3, (48, 1))
    b = rng.standard_normal((200, 40)) * 10.0 ** rng.uniform(-3, 3, (1, 40))
    exact, mag = a @ b, np.abs(a) @ np.abs(b)
    e2 = np.abs(A.product(a, b, A.SPLIT) - exact)
    assert (e2 <= (2.0 ** -16 + 2.0 ** -18) * mag).all()
    e1 = np.abs(A.product(a, b, A.BF16) - exact)
    assert (e1 <= (2.0 ** -7 + 2.0 ** -16) * mag).all() and e1.max() > 100 * e2.max()
    # the negative controls are measurably other arithmetics: lo*hi carries ~2^-9 |a||b| per term
    e_nolohi = np.abs(A.product(a, b, A.SPLIT_NO_LOHI) - exact)
    assert np.median(e_nolohi / mag) > 30 * np.median(e2 / mag)
    e_tr = np.abs(A.product(a, b, A.BF16_TRUNC) - exact)
    assert np.median(e_tr / mag) > 2 * np.median(e1 / mag)  # truncation errors all point to zero: they add up
    # 0 is the plain product, bit for bit (views, transposes and batched operands included)
    c = rng.standard_normal((3, 5, 200))
    for x, y in ((a, b), (b.T, a.T), (c, b), (a[:, ::2], b[::2])):
        assert np.array_equal(A.product(x, y, A.EXACT), x @ y)
    assert A.store(a, A.EXACT) is a and A.store(a, A.SPLIT) is a


def _object_case(embed):
    cells = synth.make_cells(4, seed=9, with_pn_feat=True, min_obj=3, max_obj=9)
    sd = synth.make_object_branch_weights(5)
    g = np.random.default_rng(2).standard_normal((4, 256)) * 0.05
    return lambda arith: OT.encode_cells_train(cells, sd, embed, embed, grad_out=g, p_drop=float(np.float32(0.1)), seed=3, arith=arith)


def _text_case():
    sd = synth.make_language_head_weights(2)
    hidden = synth.make_t5_hidden(3 * 4, 5, seed=4)
    g = np.random.default_rng(3).standard_normal((3, 256)).astype(np.float32)
    return lambda arith: OTT.text_head_train(hidden, sd, 3, grad_out=g, p_drop=float(np.float32(0.1)), seed=5, arith=arith)


def _pointnet_case():
    cells = synth.make_cells(2, seed=3, min_obj=2, max_obj=2)
    pos, rgb = synth.make_sampled_points(cells, 3)
    sd = synth.make_pointnet_weights(1)
    R = np.random.default_rng(0).standard_normal((pos.shape[0], 256))
    return lambda arith: OPT.forward_backward(pos, rgb, cells["offsets"], sd, grad_f2=R, arith=arith)


@pytest.mark.parametrize("case", ["object_embed", "object_pn", "text", "pointnet"])
def test_oracle_arithmetics_are_threaded_through(case):
    """split-bf16 stays within float32-class distance of the exact oracle; bf16 moves it by bf16's 2^-9 (and the BatchNorms' amplification
    of it); each negative control lands measurably away from the arithmetic it corrupts — the arithmetic reaches every oracle."""
    run = {"object_embed": lambda: _object_case(True), "object_pn": lambda: _object_case(False), "text": _text_case,
           "pointnet": _pointnet_case}[case]()
    res = {a: run(a) for a in (0, 1, 2, A.BF16_TRUNC, A.SPLIT_NO_LOHI)}
    out0, info0 = res[0]
    names = sorted(info0["grads"])

    def rel(a, b):  # median relative distance over the output and every gradient tensor with a non-trivial norm (a ReLU / arg-max
        d = [float(np.linalg.norm(res[a][0] - res[b][0]) / np.linalg.norm(res[b][0]))]  # flip moves single tensors by percents)
        for n in names:
            x, y = np.asarray(res[a][1]["grads"][n]), np.asarray(res[b][1]["grads"][n])
            ny = np.linalg.norm(y)
            if ny > 1e-6 * max(np.linalg.norm(np.asarray(info0["grads"][m])) for m in names):
                d.append(float(np.linalg.norm(x - y) / ny))
        return float(np.median(d))

    # (measured: split-bf16 5e-6 .. 1e-5 from exact on the object branch and the text head, bf16 1e-2 .. 5e-2, the controls 1e-2 .. 8e-2
    # from what they corrupt. The 4-object PointNet++ case sits on arg-max / ReLU decisions that any change of arithmetic flips: 1.3e-2
    # for split-bf16, 0.4 for bf16 — there only the ordering is asserted)
    if case == "pointnet":
        assert 0 < rel(2, 0) < 0.1 * rel(1, 0) and rel(A.SPLIT_NO_LOHI, 2) > 10 * rel(2, 0) and rel(A.BF16_TRUNC, 1) > 0.1
        return
    assert 0 < rel(2, 0) < 1e-4
    assert rel(1, 0) > 5e-3
    assert rel(A.SPLIT_NO_LOHI, 2) > 1000 * rel(2, 0)
    assert rel(A.BF16_TRUNC, 1) > 5e-3


def test_arith_0_is_the_default_oracle_bit_for_bit():
    for run in (_object_case(False), _text_case(), _pointnet_case()):
        out_a, info_a = run(0)
        out_b, info_b = run(A.EXACT)
        assert np.array_equal(out_a, out_b)
        for n, g in info_a["grads"].items():
            assert np.array_equal(g, info_b["grads"][n]), n
    # and the signature default is 0
    cells = synth.make_cells(2, seed=1, min_obj=3, max_obj=4)
    sd = synth.make_object_branch_weights(1)
    assert np.array_equal(OT.encode_cells_train(cells, sd, True, True)[0], OT.encode_cells_train(cells, sd, True, True, arith=0)[0])


@pytest.mark.parametrize("embed", [True, False], ids=["embed", "pn"])
def test_object_oracle_rounds_exactly_the_gemm_served_forward_products(embed):
    """Product by product, in the forward: under bf16 operands the features and the batch statistics of every BatchNorm behind a
    GEMM-served Linear move, those of the [1|3 -> 64] first layers of the small encoders (float32 FMAs on the device) do not."""
    cells = synth.make_cells(4, seed=9, with_pn_feat=True, min_obj=3, max_obj=9)
    sd = synth.make_object_branch_weights(5)
    _, i0 = OT.encode_cells_train(cells, sd, embed, embed)
    _, i1 = OT.encode_cells_train(cells, sd, embed, embed, arith=A.BF16)
    assert not np.array_equal(i0["features"], i1["features"])
    assert sorted(i0["bn_stats"]) == sorted(i1["bn_stats"])
    smallk = {f"object_encoder.{b}.0.1" for b in ("color_encoder", "pos_encoder", "num_encoder")}
    assert smallk & set(i0["bn_stats"])
    for k in i0["bn_stats"]:
        (m0, v0, _), (m1, v1, _) = i0["bn_stats"][k], i1["bn_stats"][k]
        if k in smallk:
            assert np.array_equal(m0, m1) and np.array_equal(v0, v1), k
        else:
            assert not np.array_equal(m0, m1) and not np.array_equal(v0, v1), k
