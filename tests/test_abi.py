"""CPU tier: the C-ABI library loads and exports every symbol include/t2l.h declares (no compute calls)."""
import os.path as osp
import re

import pytest

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _declared():
    src = open(osp.join(REPO, "include", "t2l.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(t2l_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_the_boundary():
    names = _declared()
    for need in ("t2l_create", "t2l_destroy", "t2l_load_weights", "t2l_encode_cells", "t2l_db_set", "t2l_search",
                 "t2l_contrastive_loss", "t2l_last_error"):
        assert need in names


def test_library_exports_every_declared_symbol():
    from text2loc_amd import engine

    lib = engine.load_library()
    for name in _declared():
        assert hasattr(lib, name), f"libt2l.so does not export {name}"
    assert set(engine.EXPORTS) == set(_declared()), "ctypes binding and header disagree"
    assert lib.t2l_abi_version() == 2


def test_null_context_is_rejected_without_a_gpu():
    from text2loc_amd import engine

    lib = engine.load_library()
    assert lib.t2l_search(None, None, 1, 1, None, None, None) == -1  # T2L_EINVAL
    assert lib.t2l_db_rows(None) == -1
    assert lib.t2l_last_error(None) == b"null context"


class _DeviceTensorStub:
    """What _dev_ptr looks at, with an address of the test's choosing (no GPU here to allocate from)."""

    is_cuda = True

    def __init__(self, dtype, ptr, contiguous=True):
        self.dtype, self._ptr, self._contiguous = dtype, ptr, contiguous

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._ptr


def test_alignment_contract_refusals():
    """DESIGN.md, alignment contract: typed arrays need their element's alignment, which every contiguous tensor has; the byte buffer of
    t2l_merge_gathered is read as int32 / float64 and is refused unless it starts on an 8-byte boundary — before any launch."""
    import inspect

    import torch
    from text2loc_amd import engine

    base = 0x7F0000000000
    assert engine._dev_ptr(_DeviceTensorStub(torch.uint8, base + 8), torch.uint8, "blocks", align=8) == base + 8
    for off in (1, 4, 7, 12):
        with pytest.raises(engine.T2LError, match="blocks: must start on a 8-byte boundary"):
            engine._dev_ptr(_DeviceTensorStub(torch.uint8, base + off), torch.uint8, "blocks", align=8)
    # a row slice of a per-point or per-object array (rgb[5:] starts 60 bytes in) is a legal argument: element alignment only
    assert engine._dev_ptr(_DeviceTensorStub(torch.float32, base + 60), torch.float32, "rgb") == base + 60
    with pytest.raises(engine.T2LError, match="contiguous"):
        engine._dev_ptr(_DeviceTensorStub(torch.float32, base, contiguous=False), torch.float32, "rgb")
    # the wrapper asks for it before it touches its outputs or the library
    src = inspect.getsource(engine.Engine.merge_gathered)
    assert src.index('"blocks", align=8') < src.index("torch.empty") < src.index("t2l_merge_gathered(")
    header = open(osp.join(REPO, "include", "t2l.h")).read()
    assert "must start on an 8-byte boundary" in header and "Alignment:" in header


def test_engine_refuses_to_run_without_gpu():
    import torch
    from text2loc_amd import engine

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(engine.T2LError):
        engine.Engine()
