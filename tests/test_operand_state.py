"""sbo::OperandState (csrc/operand_state.hpp), the record of how much of a
derived operand is valid: a stand-alone program (tests/operand_state_main.cpp)
walks its operations, built with g++ alone -- the header includes no HIP
header -- once plainly and once under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_operand_state_rules(tmp_path, flags):
    exe = str(tmp_path / "operand_state")
    src = os.path.join(ROOT, "tests", "operand_state_main.cpp")
    inc = os.path.join(ROOT, "safe_bayesian_optimization_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", exe],
                   check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "operand_state ok" in r.stdout
