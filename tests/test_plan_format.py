"""The tick plan's device format (csrc/plan_format.hpp): item descriptors,
tile-list entries, plan keys, the window padding and the capacity predicate.
A stand-alone program (tests/plan_format_main.cpp) round-trips every field at
its edges, built with g++ alone -- the header includes no HIP header -- once
plainly and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_plan_format_round_trips(tmp_path, flags):
    exe = str(tmp_path / "plan_format")
    src = os.path.join(ROOT, "tests", "plan_format_main.cpp")
    inc = os.path.join(ROOT, "safe_bayesian_optimization_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", exe],
                   check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_format ok" in r.stdout
