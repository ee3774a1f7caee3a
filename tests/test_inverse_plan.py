"""sbo_debug_inverse_plan (the layout of the recursive f64 inverse, csrc/inverse.cpp
plan_inverse) against a plain restatement of its rules:

  split      h = ((ceil(n / b) + 1) // 2) * b for n > b; n <= b is a base case
  slots      slot 0 for single calls; the base case of block k (columns k b ..) in
             slot k + 1; 128-column blocks from max(64, n // 512 + 2); that + n // 128 + 1 in all
  scratch    a node's S (m x h doubles) first, its subtrees' after it: A's and C's in the
             same place -- except under a two-lane top node, where C's follows A's
  slicing    nothing unless two lanes exist, n > b and the top node passes the level test
             (digits != 0, h >= oz_min, h <= 16384, m <= 16384); then every node by that test
  doubling   leaves mode 2, n // b >= 4 and b / 128 a power of two: (n // b) b b / 4 doubles
  workspace  per lane the largest need of its sliced nodes, a node's the larger of its two
             products' (the sliced GEMM's gz_workspace_bytes)

CPU only: the planner is host arithmetic, no device."""
import numpy as np
import pytest

from safe_bayesian_optimization_amd import _native as N

REC = 12
BASES = (1024, 2048, 4096)


def n_values(b):
    return sorted({b, b + 1, 2 * b, 2 * b + 1, 3 * b + 1, 4 * b, 4 * b + 1, 9000, 16384, 40000, 65536})


def library_plan(n, b, leaves, digits, oz_min, lanes, ld=None, panels=16):
    ld = n if ld is None else ld
    cnt = np.zeros(1, np.int64)
    f = N.lib().sbo_debug_inverse_plan
    assert f(n, ld, b, panels, leaves, digits, oz_min, lanes, None, 0, cnt.ctypes.data) == 0
    out = np.full(int(cnt[0]), -7, np.int64)
    assert f(n, ld, b, panels, leaves, digits, oz_min, lanes, out.ctypes.data, out.size, cnt.ctypes.data) == 0
    out = out.reshape(-1, REC)
    head = dict(zip(("nodes", "scratch", "leaf_scratch", "doubling", "leaf128", "info_total", "ws0", "ws1",
                     "half_slots", "two_lane_top"), out[0]))
    keys = ("off", "n", "h", "s_off", "slot", "sliced", "lane", "left", "right", "ws")
    nodes = [dict(zip(keys, (int(v) for v in r))) for r in out[1:]]
    assert head["nodes"] == len(nodes)
    assert not out[:, 10:].any()
    return {k: int(v) for k, v in head.items()}, nodes


def split(n, b):
    return ((n + b - 1) // b + 1) // 2 * b


def level(digits, oz_min, h, m):
    return digits != 0 and h >= oz_min and h <= 16384 and m <= 16384


def gz_workspace_bytes(m, n, k, nd):
    kp, mp, npad = -(-k // 64) * 64, -(-m // 128) * 128, -(-n // 128) * 128
    return (mp + npad) * kp * nd + 12 * (mp + npad) + 256


def seq_scratch(n, b):
    if n <= b:
        return 0
    h = split(n, b)
    return h * (n - h) + max(seq_scratch(h, b), seq_scratch(n - h, b))


def model(n, b, digits, oz_min, lanes):
    """The nodes in the recursion's order, and the scratch total."""
    top_h = split(n, b) if n > b else 0
    slicing = lanes == 2 and n > b and level(digits, oz_min, top_h, n - top_h)
    nodes = []

    def rec(off, n_, s_off, lane, top):
        me = dict(off=off, n=n_, h=0, s_off=-1, slot=off // b + 1, sliced=0, lane=lane, left=-1, right=-1, ws=0)
        nodes.append(me)
        if n_ <= b:
            return
        h = split(n_, b)
        m = n_ - h
        me.update(h=h, s_off=s_off, sliced=int(slicing and level(digits, oz_min, h, m)))
        if me["sliced"]:
            me["ws"] = max(gz_workspace_bytes(m, h, h, digits), gz_workspace_bytes(h, m, m, digits))
        side = top and lanes == 2
        me["left"] = len(nodes)
        rec(off, h, s_off + h * m, lane, False)
        me["right"] = len(nodes)
        rec(off + h, m, s_off + h * m + (seq_scratch(h, b) if side else 0), 1 if side else lane, False)

    rec(0, n, 0, 0, True)
    if n <= b:
        total = 0
    else:
        h, m = top_h, n - top_h
        l, r = seq_scratch(h, b), seq_scratch(m, b)
        total = h * m + (l + r if lanes == 2 else max(l, r))
    return nodes, total


def subtree(nodes, i):
    out, stack = [], [i]
    while stack:
        k = stack.pop()
        out.append(k)
        if nodes[k]["h"]:
            stack += [nodes[k]["left"], nodes[k]["right"]]
    return out


def s_region(nd):
    return (nd["s_off"], nd["s_off"] + nd["h"] * (nd["n"] - nd["h"]))


def disjoint(a, b):
    return a[1] <= b[0] or b[1] <= a[0]


def check_plan(n, b, leaves, digits, oz_min, lanes):
    head, nodes = library_plan(n, b, leaves, digits, oz_min, lanes)
    want_nodes, want_scratch = model(n, b, digits, oz_min, lanes)
    tag = (n, b, leaves, digits, oz_min, lanes)

    # the leaves: the b x b diagonal blocks at multiples of b, the last one partial, block k in slot k + 1
    leaf = [nd for nd in nodes if nd["h"] == 0]
    nblk = -(-n // b)
    assert [(nd["off"], nd["n"]) for nd in leaf] == [(k * b, min(b, n - k * b)) for k in range(nblk)], tag
    assert [nd["slot"] for nd in leaf] == list(range(1, nblk + 1)), tag
    assert 1 + nblk <= head["leaf128"], tag
    assert head["leaf128"] == max(64, n // 512 + 2) and head["info_total"] == head["leaf128"] + n // 128 + 1, tag
    assert head["leaf128"] + (n // b) * b // 128 <= head["info_total"], tag

    # inner nodes: the split rule, children adjacent, slots continuing
    for nd in nodes:
        if nd["h"] == 0:
            assert nd["n"] <= b and nd["s_off"] == -1 and not nd["sliced"], tag
            continue
        assert nd["n"] > b and nd["h"] == split(nd["n"], b) and 0 < nd["h"] < nd["n"] and nd["h"] % b == 0, tag
        le, ri = nodes[nd["left"]], nodes[nd["right"]]
        assert (le["off"], le["n"]) == (nd["off"], nd["h"]), tag
        assert (ri["off"], ri["n"]) == (nd["off"] + nd["h"], nd["n"] - nd["h"]), tag
        assert nd["slot"] == nd["off"] // b + 1, tag
    assert head["half_slots"] == (nodes[0]["h"] // b if nodes[0]["h"] else 0), tag
    assert head["two_lane_top"] == int(lanes == 2 and n > b), tag

    # scratch: every S inside the total, disjoint from its descendants' and from the other lane's subtree
    assert head["scratch"] == want_scratch, tag
    for i, nd in enumerate(nodes):
        if nd["h"] == 0:
            continue
        lo, hi = s_region(nd)
        assert 0 <= lo < hi <= head["scratch"], tag
        for k in subtree(nodes, i)[1:]:
            if nodes[k]["h"]:
                assert disjoint((lo, hi), s_region(nodes[k])), tag
    if head["two_lane_top"]:
        top = nodes[0]
        sides = [[nodes[k] for k in subtree(nodes, top[c]) if nodes[k]["h"]] for c in ("left", "right")]
        assert all(nd["lane"] == 0 for nd in sides[0]) and all(nd["lane"] == 1 for nd in sides[1]), tag
        for x in sides[0]:
            for y in sides[1]:
                assert disjoint(s_region(x), s_region(y)), tag
        assert all(nodes[k]["lane"] == 1 for k in subtree(nodes, top["right"])), tag
    else:
        assert all(nd["lane"] == 0 for nd in nodes), tag

    # the leaves by doubling
    dbl = leaves == 2 and n // b >= 4 and (b // 128) & (b // 128 - 1) == 0
    assert head["doubling"] == int(dbl) and head["leaf_scratch"] == ((n // b) * b * b // 4 if dbl else 0), tag

    # slicing and the lanes' workspaces
    top_h = nodes[0]["h"]
    slicing = lanes == 2 and n > b and level(digits, oz_min, top_h, n - top_h)
    for nd in nodes:
        want = slicing and nd["h"] > 0 and level(digits, oz_min, nd["h"], nd["n"] - nd["h"])
        assert nd["sliced"] == int(want), tag
        if nd["sliced"]:
            h, m = nd["h"], nd["n"] - nd["h"]
            assert nd["ws"] == max(gz_workspace_bytes(m, h, h, digits), gz_workspace_bytes(h, m, m, digits)), tag
        else:
            assert nd["ws"] == 0, tag
    for lane, key in ((0, "ws0"), (1, "ws1")):
        assert head[key] == max([nd["ws"] for nd in nodes if nd["lane"] == lane and nd["sliced"]], default=0), tag

    # and node for node the restatement
    assert nodes == want_nodes, tag
    return head, nodes


@pytest.mark.parametrize("b", BASES)
@pytest.mark.parametrize("lanes", (1, 2))
def test_plan_matches_the_rules(b, lanes):
    for n in n_values(b):
        for leaves in (0, 1, 2):
            for digits, oz_min in ((0, 4096), (6, 4096), (5, 2048), (6, 2048)):
                check_plan(n, b, leaves, digits, oz_min, lanes)


def test_top_over_16384_slices_nothing():
    """n = 40000 at base 2048: the top split is 20480 > 16384, so no level slices although
    the levels below would pass the level test on their own."""
    head, nodes = check_plan(40000, 2048, 2, 6, 2048, 2)
    assert nodes[0]["h"] == 20480 and not any(nd["sliced"] for nd in nodes)
    assert any(level(6, 2048, nd["h"], nd["n"] - nd["h"]) for nd in nodes if nd["h"])
    assert head["ws0"] == 0 and head["ws1"] == 0


def test_sliced_levels_of_the_flagship_shape():
    """n = 16384 at base 2048 with oz_min 2048: the top and both halves' tops slice, the 2048 x
    2048 level too; one lane: nothing."""
    _, nodes = check_plan(16384, 2048, 2, 6, 2048, 2)
    assert sorted({nd["h"] for nd in nodes if nd["sliced"]}) == [2048, 4096, 8192]
    _, nodes = check_plan(16384, 2048, 2, 6, 2048, 1)
    assert not any(nd["sliced"] for nd in nodes)


@pytest.mark.parametrize("b", BASES)
def test_early_half_plan(b):
    """The plan of the half beside the Cholesky: dgemm products, base cases one by one, one lane,
    the sequential layout; its first half's slots are A's base cases."""
    for n in n_values(b):
        if n <= b:
            continue
        head, nodes = check_plan(n, b, 0, 0, 4096, 1)
        assert not any(nd["sliced"] for nd in nodes) and head["scratch"] == seq_scratch(n, b)
        assert head["half_slots"] == nodes[nodes[0]["right"]]["slot"] - 1 == split(n, b) // b
        assert head["doubling"] == 0 and head["leaf_scratch"] == 0


def test_leading_dimension_does_not_move_the_layout():
    a = library_plan(5000, 1024, 2, 6, 2048, 2, ld=5000)
    b = library_plan(5000, 1024, 2, 6, 2048, 2, ld=8192)
    assert a == b


def test_rejects_bad_arguments():
    f = N.lib().sbo_debug_inverse_plan
    cnt = np.zeros(1, np.int64)
    out = np.zeros(REC, np.int64)
    assert f(0, 1, 1024, 16, 0, 0, 4096, 1, None, 0, cnt.ctypes.data) == 1
    assert f(100, 50, 1024, 16, 0, 0, 4096, 1, None, 0, cnt.ctypes.data) == 1          # ld < n
    assert f(100, 100, 1000, 16, 0, 0, 4096, 1, None, 0, cnt.ctypes.data) == 1        # base no multiple of 128
    assert f(100, 100, 1024, 16, 3, 0, 4096, 1, None, 0, cnt.ctypes.data) == 1        # leaves mode
    assert f(100, 100, 1024, 16, 0, 0, 4096, 3, None, 0, cnt.ctypes.data) == 1        # lanes
    assert f(100, 100, 1024, 16, 0, 0, 4096, 1, None, 0, None) == 1
    assert f(5000, 5000, 1024, 16, 0, 0, 4096, 1, out.ctypes.data, out.size, cnt.ctypes.data) == 1   # too small
    assert cnt[0] > REC
