"""The search host path without a GPU: tests/search_plan_check.cpp includes text2loc_amd/csrc/search_plan.h alone — the launch
planner (which kernels a (Q, k, rows, options) call gets, with what grid, LDS and arguments) and the report-card policy (when the
split-bf16 stand-in, heavy mode, all-exact mode and the merged records switch on and off) — and asserts a table of plans and a set
of policy sequences. This file compiles it with the host compiler and runs it."""
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
def test_planner_and_policy(tmp_path):
    exe = str(tmp_path / "search_plan_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "search_plan_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "search_plan_check: ok" in run.stdout
