"""A numpy integer restatement of the int8-sliced GEMM (csrc/ozgemm.hip), so
that its results can be predicted bit for bit WITHOUT reading a line of the
kernel: the construction is deterministic (ozgemm.hip's header, include/sbo.h
at sbo_debug_gz_gemm).

C (m x n) = alpha op(A) op(B) (+ C), op(A) m x K, op(B) K x n, ND digits:
  * every row of op(A) and every column of op(B) gets one exponent
    e = frexp(1.01 max|.|)[1] (2^e > 1.01 max; -900 for an all-zero one);
  * every entry one integer X = rint(a 2^(8 ND - 1 - e)) (ties to even),
    |X| < 2^(8 ND - 1) / 1.01;
  * X is cut into ND balanced base-256 digits D_0 (top) .. D_{ND-1}: the bytes
    of X + bias, bias = 0x80 in each of the ND - 1 lower bytes; the top byte is
    read as int8, the others as byte - 128, so every digit lies in [-128, 127]
    and sum_s D_s 256^(ND-1-s) = X;
  * level sums l_L = sum_{s+u=L} D_s(A) D_u(B)^T for L < ND, exact integers
    below 2^31 (the kernel's int32 accumulators); levels L >= ND are dropped;
  * an f64 Horner t = l_{ND-1}; t = l_L 2^(8 (ND-1-L)) + t for L = ND-2 .. 0:
    the product is exact, so each step rounds once, as the kernel's fma does;
  * val = alpha ldexp(t, eA_i + eB_j - 8 ND - 6);
  * f64 output: val, or C + val with BETA1; f32 output: float32(val), or
    float32(float64(C) + val).
Triangular flags zero the masked part of the operand BEFORE the row maxima are
taken (that part of the caller's array is never read: it may hold NaN);
transposes only change how the caller's arrays are read.  LOWER_C (f32 form)
leaves the 128 x 128 tiles wholly above C's diagonal alone and writes the
tiles that meet it whole.

Buffers are 2-D arrays indexed [row, column] of the caller's column-major
storage (shape (ld, cols); Fortran order when they go to the library).
Test helper, not product code."""
import numpy as np

TRI_A, TRANS_A, TRI_B_LOWER, TRI_B_UPPER, TRANS_B, TRANS_C, BETA1, LOWER_C = 1, 2, 4, 8, 16, 32, 64, 128
MAX_K = 16384
ZERO_EXP = -900
TILE = 128   # rows and columns of an f32 tile (LOWER_C's granularity)


def exponents(M):
    """e = frexp(1.01 max|row|)[1] per row of the f64 matrix M (ZERO_EXP for an all-zero row)."""
    amax = np.abs(M).max(axis=1) if M.shape[1] else np.zeros(M.shape[0])
    e = np.frexp(amax * 1.01)[1].astype(np.int64)
    return np.where(amax > 0.0, e, ZERO_EXP)


def integers(M, e, nd):
    """X = rint(a 2^(8 nd - 1 - e)) as int64, row by row (the scaling by a power of two is exact)."""
    scale = np.where(e > ZERO_EXP, np.ldexp(1.0, (8 * nd - 1 - e).astype(np.int32)), 0.0)
    X = np.rint(M * scale[:, None])
    assert np.all(np.isfinite(X)) and np.all(np.abs(X) * 1.01 < 2.0 ** (8 * nd - 1) + 2)
    return X.astype(np.int64)


def digits(X, nd):
    """The nd balanced base-256 digits of X, top first: (nd, rows, K) int64 in [-128, 127]."""
    bias = sum(0x80 << (8 * j) for j in range(nd - 1))
    Y = X + bias
    D = np.empty((nd,) + X.shape, np.int64)
    for s in range(nd):
        b = (Y >> (8 * (nd - 1 - s))) & 0xFF
        D[s] = np.where(b >= 128, b - 256, b) if s == 0 else b - 128
    assert D.min(initial=0) >= -128 and D.max(initial=0) <= 127
    assert np.array_equal(sum(D[s] << (8 * (nd - 1 - s)) for s in range(nd)), X)
    return D


def level_sums(DA, DB):
    """l_L = sum_{s+u=L} D_s(A) D_u(B)^T for L < nd: (nd, m, n) int64, each |l_L| < 2^31.

    The digit matrices are multiplied in float64 (BLAS): every product is an
    integer of at most 2^14 and every partial sum of one level stays below
    nd K 2^14 <= 2^31 < 2^53, so the float sums are exact in any order."""
    nd = DA.shape[0]
    fa, fb = DA.astype(np.float64), DB.astype(np.float64)
    lv = np.zeros((nd, DA.shape[1], DB.shape[1]), np.float64)
    for s in range(nd):
        for u in range(nd - s):
            lv[s + u] += fa[s] @ fb[u].T
    assert np.array_equal(lv, np.rint(lv)) and np.abs(lv).max(initial=0.0) < 2.0 ** 31
    return lv.astype(np.int64)


def product(opA, opB, nd, alpha=1.0, info=None):
    """alpha op(A) op(B) as the sliced GEMM computes it: (m, n) float64.
    opA (m, K) and opB (K, n) are dense f64 (masks already applied).  info (a
    dict) receives eA, eB and the largest |level sum|."""
    opA, opBt = np.asarray(opA, np.float64), np.asarray(opB, np.float64).T
    assert opA.ndim == 2 and opBt.ndim == 2 and opA.shape[1] == opBt.shape[1]
    assert 1 <= opA.shape[1] <= MAX_K and 1 <= nd <= 6
    eA, eB = exponents(opA), exponents(opBt)
    lv = level_sums(digits(integers(opA, eA, nd), nd), digits(integers(opBt, eB, nd), nd))
    t = lv[nd - 1].astype(np.float64)
    for L in range(nd - 2, -1, -1):
        t = lv[L].astype(np.float64) * 2.0 ** (8 * (nd - 1 - L)) + t   # (the product is exact: one rounding)
    ex = (eA[:, None] + eB[None, :] - 8 * nd - 6).astype(np.int32)
    if info is not None:
        info.update(eA=eA, eB=eB, max_level=int(np.abs(lv).max(initial=0)))
    return np.float64(alpha) * np.ldexp(t, ex)


def operands(A, B, m, n, K, flags):
    """op(A) (m x K) and op(B) (K x n) in f64 read from the caller's buffers,
    the triangular operands' zero part set to zero without looking at it."""
    opA = np.asarray(A)[:K, :m].T if flags & TRANS_A else np.asarray(A)[:m, :K]
    opB = np.asarray(B)[:n, :K].T if flags & TRANS_B else np.asarray(B)[:K, :n]
    opA, opB = opA.astype(np.float64), opB.astype(np.float64)
    i, k = np.arange(m)[:, None], np.arange(K)[None, :]
    if flags & TRI_A:
        opA = np.where(k <= i, opA, 0.0)
    k, j = np.arange(K)[:, None], np.arange(n)[None, :]
    if flags & TRI_B_LOWER:
        opB = np.where(k >= j, opB, 0.0)
    if flags & TRI_B_UPPER:
        opB = np.where(k <= j, opB, 0.0)
    return opA, opB


def store(C, val, flags):
    """The caller's whole C buffer after the call: the m x n result (n x m
    storage with TRANS_C) written or added in C's own type, everything else
    left as it was."""
    out = np.array(C, copy=True, order="F")
    m, n = val.shape
    dst = out[:n, :m].T if flags & TRANS_C else out[:m, :n]
    new = (dst.astype(np.float64) + val if flags & BETA1 else val).astype(out.dtype)
    if flags & LOWER_C:
        i, j = np.arange(m)[:, None], np.arange(n)[None, :]
        new = np.where(i // TILE >= j // TILE, new, dst)
    dst[...] = new
    return out


def gemm(A, B, C, m, n, K, nd, alpha=1.0, flags=0, info=None):
    """What sbo_debug_gz_gemm leaves in the caller's C buffer."""
    opA, opB = operands(A, B, m, n, K, flags)
    return store(C, product(opA, opB, nd, alpha, info), flags)


def gemm_packed(P, C, K, a0, m, b0, n, nd, alpha=1.0, flags=0, info=None):
    """What sbo_debug_gz_gemm_packed leaves in C: alpha P[a0:a0+m] P[b0:b0+n]^T (+ C)."""
    P = np.asarray(P)
    return store(C, product(P[a0:a0 + m, :K], P[b0:b0 + n, :K].T, nd, alpha, info), flags)


def from_digits(top, lower, nd, e=0):
    """The f64 entries whose integer has top digit `top` (array) and every
    lower digit `lower`, at row exponent e: exactly representable."""
    X = np.asarray(top, np.int64) << (8 * (nd - 1))
    for j in range(nd - 1):
        X = X + (np.int64(lower) << (8 * j))
    return np.ldexp(X.astype(np.float64), e - (8 * nd - 1))
