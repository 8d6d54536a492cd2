"""The optimizer-state layout without a GPU: tests/adam_plan_check.cpp includes text2loc_amd/csrc/adam_plan.h alone — each tensor's
offset into the moment buffer, the chunk table of the one-launch Adam step, the backbone's split point, and when a re-bind keeps the
previous moments — and asserts them on hand-written lists. This file compiles it with the host compiler and runs it."""
import os
import subprocess

import pytest

from tests.test_search_plan import CSRC, ROOT, _host_compiler


@pytest.mark.skipif(_host_compiler() is None, reason="needs a C++17 host compiler")
def test_layout_split_point_and_keep_decision(tmp_path):
    exe = str(tmp_path / "adam_plan_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "adam_plan_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adam_plan_check: ok" in run.stdout
