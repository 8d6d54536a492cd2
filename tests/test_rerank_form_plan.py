"""Without a GPU: the shapes of tests/test_gpu_rerank_form.py reach the merged-record re-rank with 16 and 8 records per query, and the
option ``search_rerank_form`` selects the instance there and only there (tests/rerank_form_plan_check.cpp drives plan_segment)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "text2loc_amd", "csrc")


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    return "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None


@pytest.mark.skipif(_host_compiler() is None, reason="needs a C++17 host compiler")
def test_test_shapes_select_the_record_rerank(tmp_path):
    exe = str(tmp_path / "rerank_form_plan_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "rerank_form_plan_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rerank_form_plan_check: ok" in run.stdout
