"""TEST INFRASTRUCTURE — the reduced-precision operand arithmetic of the training GEMMs, emulated in float64.

What the kernels declare (gemm_f32.h: GemmArgs::bf16, gemm_split_bf16; gemm_rows2.h: pn_store_t; text_head.hip:
th_split_bf16_kernel + th_gemm_kernel<.., BF16>):

* every operand is a float32 value; ``bf16`` rounds it to nearest even (v_cvt_pk_bf16_f32);
* split-bf16: ``hi = bf16(v)``, ``lo = bf16(v - hi)`` (the difference taken in float32) and a product is
  ``hi*hi + hi*lo + lo*hi`` (the ``lo*lo`` term is dropped);
* accumulation is float32 on the device; here it is float64, so what an oracle built on ``product`` leaves between itself and
  a correct kernel is float32 summation order alone.

``product(A, B, arith)``: ``arith`` 0 = exact, 1 = ``bf16(A) @ bf16(B)``, 2 = the three-term split. Two deliberately WRONG
arithmetics exist only as negative controls of the tests (they must fail the bars the kernels meet): ``BF16_TRUNC``
(bf16 by truncation instead of rounding) and ``SPLIT_NO_LOHI`` (split-bf16 without its ``lo*hi`` term).

Only ``tests/`` and the oracles may import this module.
"""
from __future__ import annotations

import numpy as np

EXACT, BF16, SPLIT = 0, 1, 2
BF16_TRUNC = "bf16_trunc"        # negative control: truncating conversion
SPLIT_NO_LOHI = "split_no_lohi"  # negative control: split-bf16 that drops lo(A) * hi(B)


def _f32_bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)).view(np.uint32)


def bf16_rne(x) -> np.ndarray:
    """float64 array of the bf16 values nearest (ties to even) to float32(x): float64 -> float32 -> bf16, bit-exactly (NaN stays NaN)."""
    u = _f32_bits(x)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = np.where(nan, (u | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r)
    return r.view(np.float32).astype(np.float64)


def bf16_trunc(x) -> np.ndarray:
    """NEGATIVE CONTROL: float32(x) truncated to bf16 (round toward zero) — what a kernel that drops the rounding step computes."""
    return (_f32_bits(x) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def split_bf16(x):
    """(hi, lo) as float64 arrays: hi = bf16(float32(x)), lo = bf16(float32(x) - hi) with the difference in float32 (exact: hi holds
    the top 8 significant bits of float32(x), so the difference is representable)."""
    x32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    hi = bf16_rne(x32)
    lo = bf16_rne(x32 - hi.astype(np.float32))
    return hi, lo


def product(A, B, arith=EXACT):
    """A @ B (matmul broadcasting) in float64 under the operand arithmetic ``arith`` (see the module docstring)."""
    if arith == EXACT:
        return A @ B
    if arith == BF16:
        return bf16_rne(A) @ bf16_rne(B)
    if arith == BF16_TRUNC:
        return bf16_trunc(A) @ bf16_trunc(B)
    if arith in (SPLIT, SPLIT_NO_LOHI):
        ah, al = split_bf16(A)
        bh, bl = split_bf16(B)
        out = ah @ bh + ah @ bl
        if arith == SPLIT:
            out = out + al @ bh
        return out
    raise ValueError(f"product: unknown arithmetic {arith!r}")


def store(x, arith):
    """A tensor the PointNet++ training path keeps in memory between two kernels (gemm_rows2.h: pn_store_t): bf16 exactly in the
    single-product arithmetics (1, and its truncating control), float32 otherwise (modelled as exact)."""
    if arith == BF16:
        return bf16_rne(x)
    if arith == BF16_TRUNC:
        return bf16_trunc(x)
    return x
