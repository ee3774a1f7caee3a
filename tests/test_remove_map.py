"""sbo_remove's bookkeeping (csrc/remove_map.hpp): caller indices to stored
positions, and numpy.delete's renumbering of the rows left.  Through
sbo_debug_remove_map (host only, no context, no GPU), and as a stand-alone
program (tests/remove_map_main.cpp) built with g++ alone -- the header
includes no HIP header -- once plainly and once under the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from safe_bayesian_optimization_amd import _native as N
from tests import remove_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBO_OK, SBO_E_INVAL, SBO_E_EMPTY = 0, 1, 5


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def call(order, idx):
    order = np.ascontiguousarray(order, np.int64)
    idx = np.ascontiguousarray(idx, np.int64)
    pos = np.full(max(idx.size, 1), -7, np.int64)
    new_order = np.full(max(order.size - idx.size, 1), -7, np.int64)
    st = N.lib().sbo_debug_remove_map(ptr(order), order.size, ptr(idx) if idx.size else None, idx.size, ptr(pos),
                                      ptr(new_order))
    return st, pos[:idx.size], new_order[:max(order.size - idx.size, 0)]


@pytest.mark.parametrize("n,b", [(1000, 1), (1000, 37), (1000, 999), (7, 3)])
def test_map_is_numpy_delete_on_a_shuffled_order(n, b):
    rng = np.random.default_rng(n + b)
    order = rng.permutation(n)
    idx = rng.choice(n, b, replace=False)
    st, pos, new_order = call(order, idx)
    assert st == SBO_OK
    # the stored positions of the removed caller indices, ascending
    assert np.array_equal(pos, np.sort(np.nonzero(np.isin(order, idx))[0]))
    # numpy.delete semantics: data kept in the caller's numbering is data[new_order] row by row
    data = rng.standard_normal(n)
    stored = data[order]
    assert np.array_equal(np.delete(data, idx)[new_order], np.delete(stored, pos))
    assert np.array_equal(np.sort(new_order), np.arange(n - b))
    mpos, mnew = RM.remove_map(order, idx)
    assert np.array_equal(pos, mpos) and np.array_equal(new_order, mnew)


def test_nothing_removed():
    st, pos, new_order = call([2, 0, 1], [])
    assert st == SBO_OK and pos.size == 0 and np.array_equal(new_order, [2, 0, 1])


@pytest.mark.parametrize("idx,status", [([1, 1], SBO_E_INVAL), ([-1], SBO_E_INVAL), ([5], SBO_E_INVAL),
                                        ([0, 1, 2, 3, 4], SBO_E_EMPTY)],
                         ids=["duplicate", "minus_one", "n", "all"])
def test_rejected_inputs(idx, status):
    st, _, _ = call([4, 2, 0, 3, 1], idx)
    assert st == status


def test_null_and_negative_arguments():
    lib = N.lib()
    order = np.arange(3, dtype=np.int64)
    assert lib.sbo_debug_remove_map(ptr(order), 3, None, 1, None, None) == SBO_E_INVAL
    assert lib.sbo_debug_remove_map(ptr(order), 3, ptr(order), -1, None, None) == SBO_E_INVAL
    assert lib.sbo_debug_remove_map(None, 3, ptr(order), 1, None, None) == SBO_E_INVAL
    assert lib.sbo_remove(None, None, 0, None, 0) == SBO_E_INVAL
    assert lib.sbo_debug_inverse64(None, None, 0) == SBO_E_INVAL


@pytest.mark.parametrize("flags", [[], ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_remove_map_program(tmp_path, flags):
    exe = str(tmp_path / "remove_map")
    src = os.path.join(ROOT, "tests", "remove_map_main.cpp")
    inc = os.path.join(ROOT, "safe_bayesian_optimization_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", exe],
                   check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "remove_map ok" in r.stdout
