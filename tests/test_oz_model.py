"""tests/oz_model.py (the integer model tests/test_gpu_ozgemm.py holds the
int8-sliced GEMM to, bit for bit) against a plain high-precision product, on
the CPU -- so that a mismatch on the GPU can be told apart: a model that meets
this bound is the documented algorithm, and the kernel must equal it.

Reference: the product in np.longdouble (64-bit mantissa), np.sum's pairwise
summation over k.

Bound, elementwise, u_ij = 2^(eA_i + eB_j - 8 ND) (eA, eB the row / column
exponents, 2^e > 1.01 max|.|):

    |model - alpha ref| <= (ND + 2) K |alpha| u_ij + ND 2^-53 |alpha ref|

Derivation.  Write a = (Xa + da) 2^(eA - 8 ND + 1) with |da| <= 1/2 (rint),
|Xa| < 2^(8 ND - 1), and likewise b.  In units of 2^(eA + eB - 16 ND + 2) (one
unit of Xa Xb; u_ij is 2^(8 ND - 2) of them) one term a b - Xa Xb is
da Xb + Xa db + da db, at most 2^(8 ND - 1) + 1/4: over K terms 2 K u_ij (and
K u_ij 2^(-8 ND), nothing).  Xa Xb = sum_L (level L) 256^(2 ND - 2 - L); the
dropped levels L >= ND hold 2 ND - 1 - L digit pairs of at most 2^14 each per
k: level ND gives (ND - 1) K 2^14 256^(ND - 2) units = (ND - 1) K u_ij, the
next ones (ND - 2) / 256 of that and less, all of them together at most
(ND - 1) (256 / 255) K u_ij.  Sum: (ND + 1 + (ND - 1) / 255) K u_ij, which
leaves 0.98 K u_ij of (ND + 2) K u_ij for what follows.  The Horner's lower
steps round partial sums of at most ND K 2^14 256^(ND - 2) (256 / 255) units
of t, that is 2^-53 of it each: below ND 2^(8 ND - 60) K u_ij <= 2e-3 K u_ij at
six digits; its last step, the product with alpha and the reference's own
error (2^-64 per product and per level of the pairwise sum: <= 15 2^(8 ND - 64)
K u_ij <= 3e-4 K u_ij) are covered by that slack and the ND 2^-53 |ref| term.
The constant comes from this derivation, not from a measurement.

Measured here, max over elements of |model - ref| / (K u_ij) -- printed by the
tests (pytest -s): Gaussian and 2^-40-spread rows stay below 0.32 at every ND
and K; the adversarial pair (every lower digit -128 in both operands, so every
dropped product is +2^14; exact integers, no rounding of X) reaches 3.008 /
4.012 / 5.016 at ND = 4 / 5 / 6, and with every X the most negative one and
every entry another 0.49 units past it 4.945 / 5.949 / 6.931 of the bound's
6 / 7 / 8: the bound is not vacuous.
"""
import numpy as np
import pytest

from tests import oz_model as Z

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the reference needs a 64-bit mantissa"

SHAPES = [(16, 16, 64), (33, 17, 200), (16, 16, 4096), (8, 8, 16384)]
KINDS = ["gaussian", "spread40", "adversarial", "adversarial_half"]


def make(kind, m, n, K, nd, seed):
    """op(A) (m x K) and op(B) (K x n), f64."""
    rng = np.random.default_rng(seed)

    def one(rows):
        if kind == "gaussian":
            return rng.standard_normal((rows, K))
        if kind == "spread40":   # 2^-40 .. 2^0 inside every row
            return rng.standard_normal((rows, K)) * np.exp2(-40.0 * rng.random((rows, K)))
        # every lower digit -128, top digits anywhere in [-126, 126], one -126
        # per row: 1.01 max = 0.9985 2^0, just under the power of two
        top = rng.integers(-126, 127, size=(rows, K))
        top[:, rng.integers(0, K)] = -126
        if kind == "adversarial_half":
            # every X the most negative one and every entry 0.49 units below
            # it: rounds to X, and da Xb + Xa db has the dropped levels' sign
            return Z.from_digits(np.full((rows, K), -126), -128, nd) - 0.49 * 2.0 ** -(8 * nd - 1)
        return Z.from_digits(top, -128, nd)

    return one(m), one(n).T


def check(opA, opB, nd, alpha, label):
    m, K = opA.shape
    info = {}
    got = Z.product(opA, opB, nd, alpha, info)
    la, lb = opA.astype(np.longdouble), opB.T.astype(np.longdouble)
    ref = np.longdouble(alpha) * (la[:, None, :] * lb[None, :, :]).sum(axis=-1)
    u = np.ldexp(1.0, (info["eA"][:, None] + info["eB"][None, :] - 8 * nd).astype(np.int32)) * K * abs(alpha)
    err = np.abs(got.astype(np.longdouble) - ref)
    ratio = float((err[u > 0] / u[u > 0]).max())   # (u = 0: an all-zero row or column)
    print(f"{label} nd={nd} K={K}: max |model - ref| / (K |alpha| u) = {ratio:.3f} of {nd + 2}; "
          f"max |l_L| / 2^31 = {info['max_level'] / 2.0 ** 31:.3f}")
    assert np.all(err <= (nd + 2) * u + nd * 2.0 ** -53 * np.abs(ref))
    return ratio, info


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nd", [4, 5, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_model_meets_the_derived_bound(kind, nd, shape):
    m, n, K = shape
    opA, opB = make(kind, m, n, K, nd, seed=1000 * nd + K)
    ratio, info = check(opA, opB, nd, 1.0, kind)
    if kind.startswith("adversarial"):
        assert np.all(info["eA"] == 0) and np.all(info["eB"] == 0)   # 1.01 max stays under 2^0
        # not vacuous: the dropped level ND alone is (ND - 1) K u
        assert ratio > nd - 1


def test_alpha_and_mixed_exponents():
    """alpha neither 1 nor a power of two; rows 2^+-100 apart, a zero row and a zero column."""
    rng = np.random.default_rng(7)
    opA = rng.standard_normal((20, 300)) * np.exp2(rng.integers(-100, 101, size=(20, 1)).astype(np.float64))
    opB = rng.standard_normal((300, 12)) * np.exp2(rng.integers(-100, 101, size=(1, 12)).astype(np.float64))
    opA[3] = 0.0
    opB[:, 5] = 0.0
    for nd in (4, 5, 6):
        _, info = check(opA, opB, nd, -0.75, "mixed")
        assert info["eA"][3] == Z.ZERO_EXP and info["eB"][5] == Z.ZERO_EXP
        got = Z.product(opA, opB, nd, -0.75)
        assert np.all(got[3] == 0.0) and np.all(got[:, 5] == 0.0)


@pytest.mark.parametrize("nd", [4, 5, 6])
def test_int32_overflow_edge(nd):
    """The largest level sum there is: every top digit -126 (the most negative
    one 2^e > 1.01 max|.| admits: -127 would need |X| >= 126.5 256^(ND-1), and
    1.01 times that passes 2^(8 ND - 1)) and every lower digit -128, in both
    operands, at K = 16384: level ND - 1 sums K (2 x 126 x 128 + (ND - 2) x
    128^2), 0.75 2^31 at six digits -- inside int32, and the model's own
    assertion (< 2^31) holds."""
    K = Z.MAX_K
    M = Z.from_digits(np.full((8, K), -126), -128, nd)
    info = {}
    got = Z.product(M, M.T.copy(), nd, 1.0, info)
    expect = K * (2 * 126 * 128 + (nd - 2) * 128 * 128)
    print(f"overflow edge nd={nd}: max |l_L| = {info['max_level']} = {info['max_level'] / 2.0 ** 31:.4f} 2^31")
    assert info["max_level"] == expect < 2 ** 31
    assert np.all(info["eA"] == 0)
    if nd == 6:
        assert expect > 0.74 * 2 ** 31
    check(M, M.T.copy(), nd, 1.0, "overflow edge")
    assert np.all(got > 0.0)


def test_digits_round_ties_to_even_and_recombine():
    """(k + 1/2) units round to the even neighbour; the digit cut is the
    balanced one (top byte signed, the others byte - 128)."""
    nd = 4
    # row maximum 0.75 2^0 -> e = 0, one unit = 2^-31
    row = np.array([[0.75, 0.5 * 2.0 ** -31, 1.5 * 2.0 ** -31, 2.5 * 2.0 ** -31, -0.5 * 2.0 ** -31,
                     -1.5 * 2.0 ** -31, 127.5 * 2.0 ** -31, 128.5 * 2.0 ** -31]])
    e = Z.exponents(row)
    assert e[0] == 0
    X = Z.integers(row, e, nd)
    assert X[0].tolist() == [3 << 29, 0, 2, 2, 0, -2, 128, 128]
    D = Z.digits(X, nd)
    assert D[:, 0, 0].tolist() == [96, 0, 0, 0]
    assert D[:, 0, 2].tolist() == [0, 0, 0, 2]
    assert D[:, 0, 5].tolist() == [0, 0, 0, -2]
    assert D[:, 0, 6].tolist() == [0, 0, 1, -128]      # 128 = 1 * 256 - 128
    # a power-of-two maximum and one just below it share the exponent; 0.99 and
    # 0.9901 of it do not (1.01 x 0.99 < 1 <= 1.01 x 0.9901)
    assert Z.exponents(np.array([[4.0], [np.nextafter(4.0, 0.0)], [3.96], [3.9604]])).tolist() == [3, 3, 2, 3]
    assert Z.exponents(np.zeros((1, 5))).tolist() == [Z.ZERO_EXP]


def test_flags_are_plain_reads_of_the_callers_arrays():
    """Transposes, triangular masks (NaN in the zero part is never looked at),
    BETA1, TRANS_C and LOWER_C restated on dense arrays."""
    rng = np.random.default_rng(3)
    m, n, K, nd = 9, 7, 11, 5
    a, b = rng.standard_normal((m, K)), rng.standard_normal((K, n))
    base = Z.product(a, b, nd, 1.0)
    A = np.full((K + 2, m + 1), np.nan)
    A[:K, :m] = a.T
    B = np.full((n + 3, K), np.nan)
    B[:n, :K] = b.T
    C = np.full((n + 1, m + 2), 7.0)
    out = Z.gemm(A, B, C, m, n, K, nd, 1.0, Z.TRANS_A | Z.TRANS_B | Z.TRANS_C)
    assert np.array_equal(out[:n, :m], base.T) and np.all(out[n:] == 7.0) and np.all(out[:, m:] == 7.0)
    out = Z.gemm(A, B, C, m, n, K, nd, 1.0, Z.TRANS_A | Z.TRANS_B | Z.TRANS_C | Z.BETA1)
    assert np.array_equal(out[:n, :m], 7.0 + base.T)
    # triangular: the masked part NaN in the caller's array, zero in the product
    al = np.where(np.arange(K)[None, :] <= np.arange(m)[:, None], a, np.nan)
    got = Z.gemm(al, b, np.zeros((m, n)), m, n, K, nd, 1.0, Z.TRI_A)
    assert np.array_equal(got, Z.product(np.nan_to_num(al), b, nd, 1.0))
    bl = np.where(np.arange(K)[:, None] >= np.arange(n)[None, :], b, np.nan)
    bu = np.where(np.arange(K)[:, None] <= np.arange(n)[None, :], b, np.nan)
    assert np.array_equal(Z.gemm(a, bl, np.zeros((m, n)), m, n, K, nd, 1.0, Z.TRI_B_LOWER),
                          Z.product(a, np.nan_to_num(bl), nd, 1.0))
    assert np.array_equal(Z.gemm(a, bu, np.zeros((m, n)), m, n, K, nd, 1.0, Z.TRI_B_UPPER),
                          Z.product(a, np.nan_to_num(bu), nd, 1.0))
    # LOWER_C: whole 128 x 128 tiles
    P = rng.standard_normal((300, 16)).astype(np.float32)
    C = np.full((300, 300), 5.0, np.float32)
    out = Z.gemm_packed(P, C, 16, 0, 300, 0, 300, 4, -1.0, Z.BETA1 | Z.LOWER_C)
    assert np.all(out[:128, 128:] == 5.0) and np.all(out[128:256, 256:] == 5.0)
    assert np.all(out[:128, :128] != 5.0) and np.all(out[256:, :] != 5.0)
    assert out.dtype == np.float32
