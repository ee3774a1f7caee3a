"""The int8-sliced GEMM (csrc/ozgemm.hip) alone, through libsbo.so's test
accessors sbo_debug_gz_gemm / sbo_debug_gz_gemm_packed, held BIT FOR BIT to
the integer model tests/oz_model.py (which tests/test_oz_model.py holds to a
long-double product within the algorithm's derived bound).

The fits reach this code only at N >= 4100 and judge it normwise at 1e-6 to
1e-5; a wrong last k-block, a wrong triangular stop, one wrong lower digit or
an exponent off on one row would pass all of them.  Here every case checks
  * the whole C buffer against the model as integers (view(int64 / int32):
    -0.0 and NaN cannot hide) -- which includes every sentinel outside C's
    m x n (ldc > m rows, extra columns) being bitwise untouched;
  * that the result is finite although every padding row and column of A and
    B and the zero part of every triangular operand hold NaN (the header
    promises they are not read).
Shapes are the smallest that cross each boundary of the code: the 128 x 64
(six digits) and 128 x 128 tiles, the 64-k stage, the digit kernel's group of
four k-blocks, the 1024-k and 128-k chunks of the two row-maximum kernels, the
K limit 16384 with the largest level sums there are (0.75 2^31 at six digits).
No inf, NaN or subnormal inside a logical operand: outside the kernel's
contract.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.gp import Context  # noqa: E402
from tests import oz_model as Z  # noqa: E402

OK, INVAL = 0, 1
assert (Z.TRI_A, Z.TRANS_A, Z.TRI_B_LOWER, Z.TRI_B_UPPER, Z.TRANS_B, Z.TRANS_C, Z.BETA1, Z.LOWER_C) == (
    N.SBO_GZ_TRI_A, N.SBO_GZ_TRANS_A, N.SBO_GZ_TRI_B_LOWER, N.SBO_GZ_TRI_B_UPPER, N.SBO_GZ_TRANS_B,
    N.SBO_GZ_TRANS_C, N.SBO_GZ_BETA1, N.SBO_GZ_LOWER_C)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def seeded(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def nasty(rng, rows, K, nd, dtype):
    """rows x K operand rows (f64 values representable in dtype), by row
    index mod 11: Gaussian; all zero; a single nonzero; all negative; maximum
    exactly a power of two; maximum just below one (1.01 max crosses the
    binade); exact ties of rint ((j + 1/2) units: to even); 2^+100 (f32:
    2^+30) with a 2^-40 spread inside the row; 2^-100 (2^-30) with the spread;
    maximum 0.99 / 0.9901 of a power of two (1.01 max on either side of it);
    Gaussian at a random power of two."""
    big = 100 if dtype == np.float64 else 30
    M = rng.standard_normal((rows, K))
    for i in range(rows):
        kind, p = i % 11, int(rng.integers(-8, 9))
        k0 = int(rng.integers(0, K))
        if kind == 1:
            M[i] = 0.0
        elif kind == 2:
            M[i] = 0.0
            M[i, k0] = rng.standard_normal()
        elif kind == 3:
            M[i] = -np.abs(M[i]) - 2.0 ** -20
        elif kind in (4, 5, 9):
            M[i] = np.clip(M[i] * 0.3, -0.9, 0.9) * 2.0 ** p
            top = dtype(2.0 ** p)
            if kind == 5:
                top = np.nextafter(top, dtype(0))
            if kind == 9:
                top = dtype((0.99 if (i // 11) % 2 == 0 else 0.9901) * 2.0 ** p)
            M[i, k0] = -top if i % 2 else top
        elif kind == 6:
            # row maximum 0.75 2^p -> e = p; one unit of X is 2^(p - 8 nd + 1)
            j = rng.integers(-2 ** 20, 2 ** 20, size=K).astype(np.float64)
            M[i] = (j + 0.5) * 2.0 ** (p - 8 * nd + 1)
            M[i, k0] = 0.75 * 2.0 ** p
        elif kind == 7:
            M[i] *= 2.0 ** big * np.exp2(-40.0 * rng.random(K))
        elif kind == 8:
            M[i] *= 2.0 ** -big * np.exp2(-40.0 * rng.random(K))
        elif kind == 10:
            M[i] *= 2.0 ** int(rng.integers(-big, big + 1))
    M = M.astype(dtype).astype(np.float64)
    tiny = float(np.finfo(dtype).tiny)
    assert np.all(np.isfinite(M)) and np.all((M == 0.0) | (np.abs(M) >= tiny))
    return M


def call_gemm(ctx, nd, f32, A, B, C, m, n, K, alpha, flags):
    """sbo_debug_gz_gemm on Fortran-ordered host buffers: (status, C after the call)."""
    A, B, out = np.asfortranarray(A), np.asfortranarray(B), np.array(C, copy=True, order="F")
    st = N.lib().sbo_debug_gz_gemm(ctx.handle, nd, int(f32), A.ctypes.data, A.shape[0], A.shape[1], B.ctypes.data,
                                   B.shape[0], B.shape[1], m, n, K, float(alpha), out.ctypes.data, out.shape[0],
                                   out.shape[1], flags)
    return st, out


def call_packed(ctx, nd, P, C, mpack, K, a0, m, b0, n, alpha, flags):
    P, out = np.asfortranarray(P), np.array(C, copy=True, order="F")
    st = N.lib().sbo_debug_gz_gemm_packed(ctx.handle, nd, P.ctypes.data, P.shape[0], mpack, K, a0, m, b0, n,
                                          float(alpha), out.ctypes.data, out.shape[0], out.shape[1], flags)
    return st, out


def buffers(rng, opA, opB, flags, dtype, pad=(3, 1)):
    """The caller's A, B and C buffers for op(A) (m x K) and op(B) (K x n):
    NaN in every padding row and column and in a triangular operand's zero
    part, random finite sentinels all over C (its m x n part is the preload
    BETA1 adds to)."""
    m, K = opA.shape
    n = opB.shape[1]
    i, k, j = np.arange(m)[:, None], np.arange(K), np.arange(n)[None, :]
    if flags & Z.TRI_A:
        opA = np.where(k[None, :] <= i, opA, np.nan)
    if flags & Z.TRI_B_LOWER:
        opB = np.where(k[:, None] >= j, opB, np.nan)
    if flags & Z.TRI_B_UPPER:
        opB = np.where(k[:, None] <= j, opB, np.nan)

    def place(M):
        buf = np.full((M.shape[0] + pad[0], M.shape[1] + pad[1]), np.nan, dtype, order="F")
        buf[:M.shape[0], :M.shape[1]] = M
        return buf

    A = place(opA.T if flags & Z.TRANS_A else opA)
    B = place(opB.T if flags & Z.TRANS_B else opB)
    cr, cc = (n, m) if flags & Z.TRANS_C else (m, n)
    C = np.asfortranarray(rng.standard_normal((cr + 5, cc + 2)).astype(dtype))
    return A, B, C


def check_gemm(ctx, rng, opA, opB, nd, f32, alpha, flags):
    dtype = np.float32 if f32 else np.float64
    m, K = opA.shape
    n = opB.shape[1]
    A, B, C = buffers(rng, opA, opB, flags, dtype)
    want = Z.gemm(A, B, C, m, n, K, nd, alpha, flags)
    tiny = float(np.finfo(dtype).tiny)
    assert np.all(np.isfinite(want)) and np.all((want == 0.0) | (np.abs(want) >= tiny)), "test input: subnormal result"
    st, got = call_gemm(ctx, nd, f32, A, B, C, m, n, K, alpha, flags)
    assert st == OK, N.lib().sbo_last_error(ctx.handle)
    region = got[:n, :m].T if flags & Z.TRANS_C else got[:m, :n]
    assert np.all(np.isfinite(region)), "NaN read from a padding row or a triangular operand's zero part"
    outside = np.ones(got.shape, bool)
    (outside[:n, :m] if flags & Z.TRANS_C else outside[:m, :n])[...] = False
    assert np.array_equal(bits(got)[outside], bits(C)[outside]), "a sentinel outside C's m x n was written"
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (f"{len(bad)} elements differ from the model, first at {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


ENTRIES = [(False, 4), (False, 5), (False, 6), (True, 4), (True, 5)]
ENTRY_IDS = ["f64-4", "f64-5", "f64-6", "f32-4", "f32-5"]

# tile edges: 128 x 64 tiles at six digits, 128 x 128 at four and five; 257 k
# crosses the digit kernel's group of four k-blocks; 1100 the 1024-k chunk of
# gz_max_kernel and the 128-k chunks of gz_rowmax_kernel
SHAPES = [(1, 1, 1), (16, 16, 64), (129, 65, 65), (130, 129, 257), (200, 150, 1100)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("f32,nd", ENTRIES, ids=ENTRY_IDS)
def test_tile_edges_dense(ctx, f32, nd, shape):
    m, n, K = shape
    rng = seeded(m, n, K, nd, f32)
    dtype = np.float32 if f32 else np.float64
    opA, opB = nasty(rng, m, K, nd, dtype), nasty(rng, n, K, nd, dtype).T
    check_gemm(ctx, rng, opA, opB, nd, f32, 1.0, 0)
    check_gemm(ctx, rng, opA, opB, nd, f32, -0.75, Z.TRANS_A | Z.TRANS_B)   # the other two pack kernels


# (flags, alpha, (m, n, K)): every flag alone, then the product's own
# combinations at triangular sizes with a partial last tile (h = 200, m = 70)
T = Z
FLAG_CASES = [
    ("transA", T.TRANS_A, 1.0, (130, 70, 200)),
    ("transB", T.TRANS_B, 1.0, (130, 70, 200)),
    ("transC", T.TRANS_C, 1.0, (130, 70, 200)),
    ("beta1", T.BETA1, -0.75, (130, 70, 200)),
    ("triA", T.TRI_A, 1.0, (200, 70, 200)),
    ("triA-short-K", T.TRI_A, 1.0, (200, 70, 100)),
    ("triBLower", T.TRI_B_LOWER, 1.0, (70, 200, 200)),        # S = L21 A^-1 (dense A, lower B)
    ("triBUpper", T.TRI_B_UPPER, 1.0, (70, 200, 200)),
    ("triBLower-short-K", T.TRI_B_LOWER, 1.0, (70, 200, 100)),   # columns >= K: nothing left of them
    ("X21", T.TRANS_A | T.TRANS_B | T.TRI_B_UPPER | T.TRANS_C, -1.0, (200, 70, 70)),   # X21 = -(S^T C^T)^T
    ("X21-wide", T.TRANS_A | T.TRANS_B | T.TRI_B_UPPER | T.TRANS_C, -1.0, (70, 200, 200)),
    ("triA-transA-beta1", T.TRI_A | T.TRANS_A | T.BETA1, 1.0, (200, 70, 200)),
    ("triBLower-transB-transC-beta1", T.TRI_B_LOWER | T.TRANS_B | T.TRANS_C | T.BETA1, -1.0, (70, 200, 200)),
]


@pytest.mark.parametrize("case", FLAG_CASES, ids=[c[0] for c in FLAG_CASES])
@pytest.mark.parametrize("f32,nd", ENTRIES, ids=ENTRY_IDS)
def test_flags(ctx, f32, nd, case):
    name, flags, alpha, (m, n, K) = case
    rng = seeded(name, nd, f32)
    dtype = np.float32 if f32 else np.float64
    check_gemm(ctx, rng, nasty(rng, m, K, nd, dtype), nasty(rng, n, K, nd, dtype).T, nd, f32, alpha, flags)


@pytest.mark.parametrize("nd", [4, 5])
def test_lower_c_f32(ctx, nd):
    """kGzLowerC (f32 form): the 128 x 128 tiles wholly above C's diagonal keep
    their sentinels, the tiles that meet it are written whole -- the model
    states that rule; the test also names the two parts."""
    rng = np.random.default_rng(40 + nd)
    m = n = 300
    K = 70
    opA, opB = nasty(rng, m, K, nd, np.float32), nasty(rng, n, K, nd, np.float32).T
    for flags, alpha in ((Z.LOWER_C, 1.0), (Z.LOWER_C | Z.BETA1 | Z.TRANS_B, -1.0)):
        check_gemm(ctx, rng, opA, opB, nd, True, alpha, flags)
    A, B, C = buffers(rng, opA, opB, Z.LOWER_C, np.float32)
    st, got = call_gemm(ctx, nd, True, A, B, C, m, n, K, 1.0, Z.LOWER_C)
    assert st == OK
    for (r0, r1, c0, c1) in ((0, 128, 128, 300), (128, 256, 256, 300)):
        assert np.array_equal(bits(got[r0:r1, c0:c1]), bits(C[r0:r1, c0:c1]))
    full = Z.gemm(A, B, C, m, n, K, nd, 1.0, 0)
    for (r0, r1, c0, c1) in ((0, 128, 0, 128), (128, 256, 0, 256), (256, 300, 0, 300)):
        assert np.array_equal(bits(got[r0:r1, c0:c1]), bits(full[r0:r1, c0:c1]))


@pytest.mark.parametrize("nd", [4, 5, 6])
def test_k_limit_and_largest_level_sums(ctx, nd):
    """K = 16384 with every top digit -126 and every lower digit -128 in both
    operands: the largest int32 level sums the construction admits (0.75 2^31
    at six digits; tests/test_oz_model.py::test_int32_overflow_edge)."""
    rng = np.random.default_rng(nd)
    M = Z.from_digits(np.full((16, Z.MAX_K), -126), -128, nd)
    info = {}
    Z.product(M, M.T, nd, 1.0, info)
    assert info["max_level"] == Z.MAX_K * (2 * 126 * 128 + (nd - 2) * 128 * 128)
    check_gemm(ctx, rng, M, M.T, nd, False, 1.0, 0)
    # and mixed signs at the limit, both layouts
    top = rng.integers(-126, 127, size=(16, Z.MAX_K))
    M2 = Z.from_digits(top, -128, nd)
    check_gemm(ctx, rng, M2, M.T, nd, False, -1.0, Z.TRANS_A | Z.TRANS_B)


@pytest.mark.parametrize("nd", [4, 5])
def test_k_limit_f32(ctx, nd):
    rng = np.random.default_rng(50 + nd)
    check_gemm(ctx, rng, nasty(rng, 16, Z.MAX_K, nd, np.float32), nasty(rng, 16, Z.MAX_K, nd, np.float32).T, nd, True,
               1.0, 0)


def test_rejected_arguments_leave_c_alone(ctx):
    """K = 0 and K = 16385, digits outside each entry's set and the flag
    combinations the code does not implement are SBO_E_INVAL; m = 0 or n = 0
    is SBO_OK; C comes back bitwise as it went in every time."""
    rng = np.random.default_rng(9)
    for f32 in (False, True):
        dtype = np.float32 if f32 else np.float64
        A = rng.standard_normal((20, Z.MAX_K + 1)).astype(dtype)
        B = rng.standard_normal((Z.MAX_K + 1, 20)).astype(dtype)
        C = rng.standard_normal((24, 24)).astype(dtype)

        def run(nd, m, n, K, flags=0, want=INVAL):
            st, got = call_gemm(ctx, nd, f32, A, B, C, m, n, K, 1.0, flags)
            assert st == want, (f32, nd, m, n, K, flags, st)
            assert np.array_equal(bits(got), bits(C))

        run(4, 16, 16, Z.MAX_K + 1)
        run(4, 16, 16, 0)
        run(4, 0, 16, 64, want=OK)
        run(4, 16, 0, 64, want=OK)
        run(4, 0, 0, 64, want=OK)
        for nd in (0, 3, 7) + ((6,) if f32 else ()):
            run(nd, 16, 16, 64)
        run(4, 16, 16, 64, Z.LOWER_C | Z.TRANS_C)
        if not f32:
            run(6, 16, 16, 64, Z.LOWER_C)
        run(4, 16, 16, 64, 256)          # not a flag
        run(4, 25, 16, 16)               # C's 24 rows cannot hold m = 25
        run(4, 21, 16, 16)               # nor A's 20 rows
        st, _ = call_gemm(ctx, 4, f32, A, B, C, 16, 16, 64, 1.0, 0)
        assert st == OK                  # (and the same arguments without the fault pass)
    assert N.lib().sbo_debug_gz_gemm(None, 4, 0, None, 1, 1, None, 1, 1, 1, 1, 1, 1.0, None, 1, 1, 0) == INVAL


# ------------------------------------------------------------- packed entry
MPACK, KPACK = 384, 192
PACKED = [(0, 384, 0, 128, 0, 1.0), (128, 256, 128, 256, Z.BETA1 | Z.LOWER_C, -1.0), (128, 130, 0, 100, Z.BETA1, -1.0)]


@pytest.fixture(scope="module")
def panels():
    """The Cholesky's panel, 384 x 192 f32, one per digit count (the ties rows
    depend on it), in a buffer with NaN padding rows; shared and left unchanged."""
    out = {}
    for nd in (4, 5):
        rng = np.random.default_rng(70 + nd)
        P = np.full((MPACK + 5, KPACK), np.nan, np.float32, order="F")
        P[:MPACK] = nasty(rng, MPACK, KPACK, nd, np.float32)
        P.setflags(write=False)
        out[nd] = P
    return out


@pytest.mark.parametrize("case", PACKED, ids=lambda c: "-".join(map(str, c[:4])))
@pytest.mark.parametrize("nd", [4, 5])
def test_packed_both_epilogues(ctx, panels, nd, case):
    """As the blocked Cholesky calls it (pack once, products of row ranges of
    the pack): a 16-byte-aligned C with ldc % 4 == 0 takes the 16-byte
    epilogue, an odd ldc the scalar one; both equal the model bit for bit, and
    so each other."""
    a0, m, b0, n, flags, alpha = case
    P = panels[nd]
    rng = np.random.default_rng(a0 + m + n + nd)
    results = []
    for ldc in ((m + 3) // 4 * 4 + 4, (m + 3) // 4 * 4 + 5):
        C = np.asfortranarray(rng.standard_normal((ldc, n + 2)).astype(np.float32))
        want = Z.gemm_packed(P, C, KPACK, a0, m, b0, n, nd, alpha, flags)
        assert np.all(np.isfinite(want))
        st, got = call_packed(ctx, nd, P, C, MPACK, KPACK, a0, m, b0, n, alpha, flags)
        assert st == OK, N.lib().sbo_last_error(ctx.handle)
        assert np.all(np.isfinite(got[:m, :n]))
        assert np.array_equal(bits(got[m:]), bits(C[m:])) and np.array_equal(bits(got[:, n:]), bits(C[:, n:]))
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, (ldc, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        if flags & Z.LOWER_C:
            assert np.array_equal(bits(got[:128, 128:n]), bits(C[:128, 128:n]))   # the tile above the diagonal
        results.append(got[:m, :n] - C[:m, :n] if flags & Z.BETA1 else got[:m, :n])
    if not flags & Z.BETA1:
        assert np.array_equal(bits(results[0]), bits(results[1]))


def test_packed_rejects(ctx, panels):
    P = panels[4]
    C = np.asfortranarray(np.random.default_rng(1).standard_normal((400, 400)).astype(np.float32))

    def run(nd, a0, m, b0, n, flags=0, K=KPACK, want=INVAL):
        st, got = call_packed(ctx, nd, P, C, MPACK, K, a0, m, b0, n, 1.0, flags)
        assert st == want, (nd, a0, m, b0, n, flags, K, st)
        assert np.array_equal(bits(got), bits(C))

    run(4, 64, 128, 0, 128)              # a0 not a multiple of 128
    run(4, 0, 128, 64, 128)              # b0
    run(4, 128, 257, 0, 128)             # a0 + m > mpack
    run(4, 0, 128, 256, 129)             # b0 + n > mpack
    for f in (Z.TRANS_C, Z.TRI_A, Z.TRI_B_LOWER, Z.TRI_B_UPPER):
        run(4, 0, 128, 0, 128, f)
    for nd in (3, 6):
        run(nd, 0, 128, 0, 128)
    run(4, 0, 128, 0, 128, K=0)
    run(4, 0, 0, 0, 128, want=OK)
    run(4, 0, 128, 0, 0, want=OK)
