"""tests/plan_model.py against explicit sums: the split, the all-six reference,
a hand-made plan's omitted products, ragged blocks.  No GPU."""
import numpy as np
import pytest

from tests import plan_model as PM


def _state(n, m, seed, spread=1.0):
    """A random lower-triangular f32 operand with tile-dependent magnitudes
    (2^-100 .. 2^3), alpha, coordinates and queries on a few length scales."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    nt = (n + PM.BK - 1) // PM.BK
    for i in range(nt):
        for j in range(nt):
            A[i * 64:(i + 1) * 64, j * 64:(j + 1) * 64] *= 2.0 ** rng.uniform(-100, 3)
    A = np.tril(A).astype(np.float32)
    alpha = rng.standard_normal(n).astype(np.float32)
    x, y = (rng.uniform(0, 3.0 * spread, n).astype(np.float32) for _ in range(2))
    qx, qy = (rng.uniform(0, 3.0 * spread, m).astype(np.float32) for _ in range(2))
    return PM.PlanModel(A, alpha, x, y, 0.4, 2.25, qx, qy)


def test_split_is_exact():
    """a0 + a1 + a2 == A for every f32 entry of |a| >= 2^-110 (n = 200, random
    tiles), each piece a bf16 value, each at most 2^-8 of the one before."""
    md = _state(200, 10, 1)
    a0, a1, a2 = md.a
    nz = md.A != 0
    assert np.abs(md.A[nz]).min() >= 2.0 ** -110 and nz.sum() > 15000
    assert np.array_equal(a0.astype(np.float64) + a1.astype(np.float64) + a2.astype(np.float64), md.A.astype(np.float64))
    assert np.array_equal((a0 + a1) + a2, md.A)
    for p in (a0, a1, a2):
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))
    assert np.all(np.abs(a1) <= 2.0 ** -8 * np.abs(a0)) and np.all(np.abs(a2) <= 2.0 ** -8 * np.abs(a1))
    assert np.any(a2)
    k = md.k
    assert np.array_equal(k[0] + k[1] + k[2], md.k32.astype(np.float64))
    # ties go to even: 1 + 2^-8 is halfway between bf16 1 and 1 + 2^-7
    assert PM.bf16_rne(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]))[0] == 1.0
    assert PM.bf16_rne(np.float32([1 + 3 * 2.0 ** -8]))[0] == np.float32(1 + 2.0 ** -6)


def test_all_six_against_longdouble():
    """The six kept products against A k in longdouble.  RNE to bf16 (8
    significant bits) leaves at most 2^-8 of a value, so |a1| <= 2^-8 |a|,
    |a2| <= 2^-16 |a| and likewise km, kl; the three products the sweep never
    forms are a1 kl, a2 km (each <= 2^-24 |a| |k|) and a2 kl (<= 2^-32), so
    |V6 - A k|_i <= (2^-23 + 2^-32) sum_k |a_ik| |k_k|.  The difference is
    not all rounding: it reaches 2^-30 of that sum somewhere."""
    md = _state(200, 37, 2, spread=0.5)
    AL, KL = md.A.astype(np.longdouble), md.k32.astype(np.longdouble)
    v6 = md.v6()[0]
    exact = AL @ KL
    bound = (2.0 ** -23 + 2.0 ** -32) * (np.abs(AL) @ np.abs(KL))
    err = np.abs(v6.astype(np.longdouble) - exact)
    assert np.all(err <= bound * (1 + 1e-9) + 1e-300)
    assert np.any(err >= 2.0 ** -30 * (np.abs(AL) @ np.abs(KL)))


def _products(md, I, t, q0, q1):
    """The nine piece products of tile (I, t) for queries q0:q1, [3, 3, rows, q] as [a piece][k piece], f64."""
    r0, r1 = md._rows(I)
    c0, c1 = t * 64, min((t + 1) * 64, md.n)
    out = np.zeros((3, 3, r1 - r0, q1 - q0))
    for i in range(3):
        for j in range(3):
            out[i, j] = md.a[i][r0:r1, c0:c1].astype(np.float64) @ md.k[j][c0:c1, q0:q1]
    return out


@pytest.mark.parametrize("n,m", [(300, 200), (520, 128)])
def test_hand_made_plan(n, m):
    """One tile dropped, one at level 1, one at level 2, the rest at level 0:
    the model's deltas are the explicit sums of exactly the omitted products
    (a ragged last row block; at m = 200 a ragged last query block)."""
    md = _state(n, m, 3 + n, spread=0.4)
    nI, nQ = md.nI, md.nQ
    rec = [(I, qb, t, 0) for I in range(nI) for qb in range(nQ) for t in range(4 * (I + 1))]
    last = nI - 1
    tl = (n - 1) // 64                            # the last k-tile that holds points: ragged columns
    special = {(last, 0, tl): None, (last, nQ - 1, 1): 1, (0, nQ - 1, 2): 2, (last, nQ - 1, 0): None}
    rec = [r for r in rec if r[:3] not in special]
    rec += [(I, qb, t, lvl) for (I, qb, t), lvl in special.items() if lvl is not None]
    e = md.effect(np.array(rec, np.int32), nI, nQ)
    dVI2 = np.zeros((nI, m))
    dvar = np.zeros(m)
    dmu = np.zeros(m)
    v6 = md.v6()
    dv_by_item = {}
    for (I, qb, t), lvl in special.items():
        q0, q1 = qb * 128, min((qb + 1) * 128, m)
        p = _products(md, I, t, q0, q1)
        om = p[2, 0] + p[1, 1] + p[0, 2]                         # a2 kh + a1 km + a0 kl
        if lvl is None or lvl == 2:
            om = om + p[1, 0] + p[0, 1]                          # a1 kh + a0 km
        if lvl is None:
            om = om + p[0, 0]                                    # a0 kh
            if I == last:
                c0, c1 = t * 64, min((t + 1) * 64, n)
                dmu[q0:q1] += md.sa[c0:c1] @ md.k32[c0:c1, q0:q1].astype(np.float64)
        dv_by_item[(I, qb)] = dv_by_item.get((I, qb), 0.0) + om
    for (I, qb), dv in dv_by_item.items():
        q0, q1 = qb * 128, min((qb + 1) * 128, m)
        dVI2[I, q0:q1] = (dv * dv).sum(0)
        vp = v6[I][:, q0:q1] - dv
        dvar[q0:q1] += (v6[I][:, q0:q1] ** 2).sum(0) - (vp ** 2).sum(0)
    assert np.any(dVI2 > 0) and np.any(dmu != 0)
    np.testing.assert_allclose(e["dVI2"], dVI2, rtol=1e-12, atol=0)
    np.testing.assert_allclose(e["dV2"], dVI2.sum(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(e["dmu"], dmu, rtol=1e-12, atol=0)
    # the explicit |V6|^2 - |Vp|^2 cancels: compare to its own rounding, 2^-52 |V6|^2 per term
    v2 = sum((v ** 2).sum(0) for v in v6)
    assert np.all(np.abs(e["dvar"] - dvar) <= 1e-12 * np.abs(dvar) + 2.0 ** -48 * v2)
    assert e["mean_lost"].tolist() == ([1] + [0] * (nQ - 2) + [1] if nQ > 1 else [2])
    # the empty plan drops everything: dV is the whole of V6, dmu the whole mean
    e0 = md.effect(np.zeros((0, 4), np.int32), nI, nQ)
    np.testing.assert_allclose(e0["dV2"], v2, rtol=1e-12)
    mu, var = md.dense_posterior(0.25)
    np.testing.assert_allclose(e0["dmu"], mu - 0.25, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(e0["dvar"], md.sf2 - var, rtol=1e-9)
    # and the full plan nothing
    full = np.array([(I, qb, t, 0) for I in range(nI) for qb in range(nQ) for t in range(4 * (I + 1))], np.int32)
    ef = md.effect(full, nI, nQ)
    assert not np.any(ef["dV2"]) and not np.any(ef["dvar"]) and not np.any(ef["dmu"])


def test_check_reports_ratios_and_rejects_bad_records():
    md = _state(300, 130, 9, spread=0.4)
    r = PM.check(md, np.zeros((0, 4), np.int32), md.nI, md.nQ, 20)
    for k in ("V", "var", "mu"):
        assert r[k][0] > 1.0 and 0 <= r[k][1] < 130
    e = r["effect"]
    q = r["V"][1]
    assert r["V"][0] == np.sqrt(e["dV2"][q]) / (2.0 ** -20 * 1.5 / 2 * 0.99)
    with pytest.raises(AssertionError):
        PM.plan_levels(np.array([[0, 0, 4, 0]]), md.nI, md.nQ)      # k-tile 4 is above row block 0's diagonal
    with pytest.raises(AssertionError):
        PM.plan_levels(np.array([[1, 2, 0, 0]]), md.nI, md.nQ)      # query block 2 of 2
    with pytest.raises(AssertionError):
        PM.plan_levels(np.array([[1, 0, 0, 0], [1, 0, 0, 1]]), md.nI, md.nQ)
