"""What every eval-mode weight loader runs before it touches the device, without a GPU: tests/weight_table_check.cpp includes
text2loc_amd/csrc/weight_table.h alone — the name table of a descriptor list (found tensors, the two error texts, what is refused at
construction, last-wins, the prefix filter, the first error kept) and the host image of a model part's one device blob (offsets at 16
and 256 bytes, contents, pointer fields bound to base + offset) — and asserts them on hand-written lists. This file compiles it with
the host compiler and runs it."""
import os
import subprocess

import pytest

from tests.test_search_plan import CSRC, ROOT, _host_compiler


@pytest.mark.skipif(_host_compiler() is None, reason="needs a C++17 host compiler")
def test_table_errors_and_staging_offsets(tmp_path):
    exe = str(tmp_path / "weight_table_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "weight_table_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "weight_table_check: ok" in run.stdout
