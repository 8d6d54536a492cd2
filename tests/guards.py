"""Guard bands around the tensors a kernel is handed, and around the ones the ``Engine`` wrappers allocate for it.

``guarded(t, fill)`` copies ``t`` into the middle of a larger buffer whose two halos hold poison; ``guarded_outputs(module)`` makes
every ``torch.empty`` / ``empty_like`` / ``zeros`` of ``module`` (text2loc_amd.engine) come out of such a buffer for the length of a
``with`` block. A kernel that reads past an end picks the poison up (two float fills: a quiet NaN for a stray value that enters
arithmetic, +3e38 for one that enters a comparison, where a NaN would be ignored), one that writes past an end changes a halo, and
one that leaves part of an output unwritten leaves the 0xA5 pattern behind. Works on CPU tensors too (tests/test_guards.py proves
each mechanism with wrong fake kernels); nothing here touches the product.
"""
import contextlib

import torch

MIB = 1 << 20
# the widest tiling in the tree: the text head's 256 rows x 1024 floats (csrc/text_head.hip) = 1 MiB, so max(1 MiB, a tile) = 1 MiB
WIDEST_TILE_BYTES = 256 * 1024 * 4
HALO_BYTES = max(MIB, WIDEST_TILE_BYTES)
assert HALO_BYTES % 256 == 0
PATTERN_BYTE = 0xA5
PATTERN_WORD = int.from_bytes(bytes([PATTERN_BYTE] * 4), "little", signed=True)  # 0xA5A5A5A5 as int32
NAN = float("nan")
BIG = 3.0e38
FLOAT_FILLS = (NAN, BIG)


def fill_id(fill):
    return "nan" if fill != fill else "3e38"


def _round_up(n, m):
    return (n + m - 1) // m * m


class Guard:
    """One guarded buffer: ``buf`` u8[lo + payload + hi], the payload view and a copy of both halos as they were filled."""

    def __init__(self, buf, lo, nbytes, view, kind):
        self.buf, self.lo, self.nbytes, self.view, self.kind = buf, lo, nbytes, view, kind
        self.want_lo = buf[:lo].clone()
        self.want_hi = buf[lo + nbytes:].clone()

    def halo_damage(self):
        """'' if both halos hold what they were filled with, else which one changed and where."""
        out = []
        for name, got, want in (("front", self.buf[:self.lo], self.want_lo), ("back", self.buf[self.lo + self.nbytes:], self.want_hi)):
            if not torch.equal(got, want):
                at = int((got != want).nonzero()[0 if name == "back" else -1])
                dist = at if name == "back" else self.lo - 1 - at
                out.append(f"{name} halo changed {dist} bytes from the payload")
        return "; ".join(out)

    def unwritten_words(self):
        """4-byte words of the payload that still hold the 0xA5 pattern."""
        raw = self.buf[self.lo:self.lo + self.nbytes // 4 * 4].view(torch.int32)
        return int((raw == PATTERN_WORD).sum())


def _carve(shape, dtype, device, skew_bytes=0):
    esize = torch.empty((), dtype=dtype).element_size()
    nbytes = esize
    for s in shape:
        nbytes *= int(s)
    if skew_bytes % esize:
        raise ValueError("the payload must stay aligned to its element size")
    lo = HALO_BYTES + skew_bytes
    hi = _round_up(lo + nbytes, 256) - (lo + nbytes) + HALO_BYTES
    buf = torch.empty((lo + nbytes + hi,), dtype=torch.uint8, device=device)
    view = buf[lo:lo + nbytes].view(dtype).view(tuple(int(s) for s in shape))
    return buf, lo, nbytes, view


def guarded(t, fill, skew_bytes=0):
    """A contiguous copy of ``t`` (same shape, dtype, device) between two halos of at least ``HALO_BYTES`` each filled with ``fill``:
    NaN or 3e38 for a float tensor, for an integer tensor a value that is in range for whatever the kernel indexes with it. ``skew_bytes``
    moves the payload that far off the allocator's 256-byte alignment (a caller's row slice)."""
    if t.dtype.is_floating_point != isinstance(fill, float):
        raise TypeError(f"fill {fill!r} does not suit a {t.dtype} tensor")
    buf, lo, nbytes, view = _carve(t.shape, t.dtype, t.device, skew_bytes)
    buf.view(t.dtype).fill_(fill)  # (the buffer is a multiple of 256 bytes and the payload starts on an element boundary)
    view.copy_(t)
    view._guard = Guard(buf, lo, nbytes, view, "input")
    return view


def check_halos(*tensors):
    """Every halo of these ``guarded`` tensors must hold its fill (synchronises first)."""
    if any(t.is_cuda for t in tensors):
        torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        damage = t._guard.halo_damage()
        assert not damage, f"guarded input {i} {tuple(t.shape)} {t.dtype}: {damage}"


class _TorchProxy:
    """Stands in for the ``torch`` name of a module: forwards everything but the three allocators."""

    def __init__(self, real, sink):
        self.__dict__["_real"], self.__dict__["_sink"] = real, sink

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _alloc(self, shape, dtype, device, kind):
        dtype = dtype or self._real.get_default_dtype()
        buf, lo, nbytes, view = _carve(shape, dtype, device or "cpu")
        buf.fill_(PATTERN_BYTE)
        if kind == "zeros":
            view.zero_()
        self._sink.append(Guard(buf, lo, nbytes, view, kind))
        return view

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)

    def empty(self, *size, dtype=None, device=None):
        return self._alloc(self._shape(size), dtype, device, "empty")

    def zeros(self, *size, dtype=None, device=None):
        return self._alloc(self._shape(size), dtype, device, "zeros")

    def empty_like(self, t, dtype=None, device=None):
        return self._alloc(tuple(t.shape), dtype or t.dtype, device or t.device, "empty")


class OutputGuards:
    """What ``guarded_outputs`` yields: ``count`` allocations guarded so far; ``guards[i]`` in allocation order."""

    def __init__(self):
        self.guards = []

    @property
    def count(self):
        return len(self.guards)

    def check(self, partly_written=()):
        """Halos untouched and no ``empty`` payload word still holding the pattern. ``partly_written``: allocation-order indices of
        outputs the header documents as partly written (halos are still checked)."""
        if any(g.buf.is_cuda for g in self.guards):
            torch.cuda.synchronize()
        for i, g in enumerate(self.guards):
            what = f"output {i} ({g.kind} {tuple(g.view.shape)} {g.view.dtype})"
            damage = g.halo_damage()
            assert not damage, f"{what}: {damage}"
            if g.kind == "empty" and i not in partly_written:
                left = g.unwritten_words()
                assert left == 0, f"{what}: {left} of {g.nbytes // 4} words were never written"


@contextlib.contextmanager
def guarded_outputs(module, partly_written=()):
    """For the block, ``module.torch`` is a proxy whose ``empty`` / ``empty_like`` / ``zeros`` return guarded tensors pre-filled with
    0xA5 (``zeros`` payloads zeroed as the product would). On a clean exit the halos and payloads are checked (``OutputGuards.check``);
    the caller asserts ``.count``, so an output allocated some other way cannot escape unnoticed."""
    real = module.torch
    out = OutputGuards()
    module.torch = _TorchProxy(real, out.guards)
    try:
        yield out
    finally:
        module.torch = real
    out.check(partly_written)
