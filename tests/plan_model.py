"""The tick plan's effect on the split sweep, tile by tile, in plain numpy f64.

The split sweep (csrc/predict_x3_rowhalf.hpp) multiplies A = sf2 L^-1 by K*
with both operands cut into three bf16 pieces, a = a0 + a1 + a2 and
k = kh + km + kl, and keeps six of the nine piece products.  The tick plan
(csrc/kernels.hip: plan_count_kernel) runs each (row block I of 256 rows,
k-tile t of 64 columns) pair of a 128-query block at one of three levels or
not at all (x3_step, predict_x3_rowhalf.hpp:117-138 and the MFMA chain at
:210-221):

    level 0                   a2 kh + a1 km + a0 kl + a1 kh + a0 km + a0 kh
    level 1                                           a1 kh + a0 km + a0 kh
    level 2                                                           a0 kh
    absent from the records   nothing

The reference is every tile of every row block at level 0.  This module forms
what a plan leaves out directly from the omitted products (no difference of
two nearly equal sums), in f64:

    dV_I(q)      the omitted part of row block I's rows of V
    |dV(q)|_2^2  = sum_I |dV_I(q)|_2^2
    dvar(q)      = |V6|^2 - |V_plan|^2 = sum_rows dV (2 V6 - dV)
    dmu(q)       the k-tiles of the last row block absent from the records,
                 sum_k (sf2 alpha_k) K*(k, q): the mean reads the f32 product
                 (float)sf2 * alpha[k] (pack_kcoord_kernel, operand.hip:72)
                 against the f32 K* of the tile (x3_step :201-207, x3_kstar
                 :263), whatever the tile's level.

The pieces.  A's are the round-to-nearest-even split of the f32 operand
(split3, bf16_split.hpp:36-41, applied by pack_x3_kernel,
predict_x3_rowhalf.hpp:571), the split the tile norms take their bounds of
(operand.hip) and test_tile_gain_bounds_are_bounds uses.  K*'s are the same
split3 of the f32 value the sweep forms in registers (kstar1, :107-110):
dx = xk - xq, dy = yk - yq in f32, s = fmaf(dy, dy, dx * dx), e = exp2(s * cexp) with
cexp = (float)(-1 / (2 (float)l^2 ln 2)) (exp2_coef, kernels.hip:1763); then
split3(e) (:189-190, :259).  The device evaluates exp2 with v_exp_f32 (one ulp,
results below 2^-126 flushed to zero); here it is the correctly rounded f32 of
the f64 exp2, flushed the same way.  That difference enters reference and plan
alike and moves an omitted product by 2^-23 of itself.

f64 rounding of the model itself: every sum is a BLAS dot product of at most
n <= 4352 f64 terms, each an exact product of two bf16 values (16 bits), so a
computed entry is within n 2^-53 sum |terms| = 5e-13 of the exact sum,
relative to the sum of magnitudes; the tests allow a relative 1e-12.
"""
import numpy as np

BM, BK, BN = 256, 64, 128      # rows of a row block, columns of a k-tile, queries of a block
DROPPED = 3                    # the level code of a (row block, k-tile) pair absent from the records


def bf16_rne(a):
    """f32 -> the nearest bf16 (ties to even), as f32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def split3(a):
    """a = p0 + p1 + p2: each piece the bf16 rounding of what the ones before
    left, the subtractions in f32 (exact: a - bf16(a) has at most 16 bits).
    Exact for every f32 whose lowest bit is at least 2^-133, the bf16
    subnormal step: |a| >= 2^-110."""
    a = np.ascontiguousarray(a, np.float32)
    p0 = bf16_rne(a)
    r1 = a - p0
    p1 = bf16_rne(r1)
    p2 = bf16_rne(r1 - p1)
    return p0, p1, p2


def bf16_bits(p):
    """The 16 bits of a bf16 value held as f32."""
    return (np.ascontiguousarray(p, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def cexp_f32(ell):
    """The sweep's exp2 coefficient: (float)(-1 / (2 (float)l^2 ln 2))."""
    e = float(np.float32(ell))
    return np.float32(-1.0 / (2.0 * e * e * 0.69314718055994530942))


def kstar_f32(xk, yk, xq, yq, cexp):
    """K*[k, q] as the sweep's registers hold it (f32, without sf2: A carries it)."""
    xk, yk, xq, yq = (np.ascontiguousarray(v, np.float32) for v in (xk, yk, xq, yq))
    dx = xk[:, None] - xq[None, :]
    dy = yk[:, None] - yq[None, :]
    dx2 = (dx * dx).astype(np.float64)                       # the f32 product, rounded
    s = (dy.astype(np.float64) * dy.astype(np.float64) + dx2).astype(np.float32)    # fmaf: one rounding
    arg = s * np.float32(cexp)
    e = np.exp2(arg.astype(np.float64)).astype(np.float32)
    e[arg < np.float32(-126.0)] = np.float32(0.0)
    return e


def plan_levels(rec, nI, nQ):
    """[nI, nQ, 4 nI] level codes from the (I, qb, t, level) records: 0, 1, 2,
    DROPPED for a pair absent from them, -1 for t beyond the row block's
    4 (I + 1) k-tiles."""
    rec = np.asarray(rec, np.int64).reshape(-1, 4)
    lv = np.full((nI, nQ, 4 * nI), DROPPED, np.int8)
    for I in range(nI):
        lv[I, :, 4 * (I + 1):] = -1
    if rec.size:
        assert rec[:, 0].min() >= 0 and rec[:, 0].max() < nI and rec[:, 1].min() >= 0 and rec[:, 1].max() < nQ
        assert np.all(rec[:, 2] >= 0) and np.all(rec[:, 2] < 4 * (rec[:, 0] + 1)) and np.all((rec[:, 3] >= 0) & (rec[:, 3] <= 2))
        assert np.unique(rec[:, :3], axis=0).shape[0] == rec.shape[0], "a pair is in the records twice"
        lv[rec[:, 0], rec[:, 1], rec[:, 2]] = rec[:, 3]
    return lv


class PlanModel:
    """One fitted state and one query set in sweep order.

    A: the f32 operand sf2 L^-1 (n x n; only its lower triangle is read),
    alpha in internal order, x / y the training coordinates in internal
    order, qx / qy the queries in sweep order (position p belongs to query
    block p // 128)."""

    def __init__(self, A, alpha, x, y, length_scale, sf2, qx, qy):
        A = np.tril(np.ascontiguousarray(A, np.float32))
        self.n = n = A.shape[0]
        self.m = m = int(np.size(qx))
        self.nI = (n + BM - 1) // BM
        self.nQ = (m + BN - 1) // BN
        self.sf2 = float(sf2)
        self.A = A
        self.a = split3(A)                                   # three n x n f32 arrays of bf16 values
        self.k32 = kstar_f32(x, y, qx, qy, cexp_f32(length_scale))     # [n, m]
        self.k = tuple(p.astype(np.float64) for p in split3(self.k32))
        # the mean's operand: (float)sf2 * alpha[k] in f32
        self.sa = (np.float32(sf2) * np.ascontiguousarray(alpha, np.float32)).astype(np.float64)
        self._v6 = None

    def _cols(self, I):
        return min(4 * (I + 1) * BK, self.n)

    def _rows(self, I):
        return I * BM, min((I + 1) * BM, self.n)

    def v6(self):
        """The reference: every tile at six products, per row block [rows, m]."""
        if self._v6 is None:
            kh, km, kl = self.k
            out = []
            for I in range(self.nI):
                r0, r1 = self._rows(I)
                c = self._cols(I)
                a0, a1, a2 = (p[r0:r1, :c].astype(np.float64) for p in self.a)
                # (a0 + a1 + a2) kh + (a0 + a1) km + a0 kl: the six products (the piece sums are exact in f64)
                out.append((a0 + a1 + a2) @ kh[:c] + (a0 + a1) @ km[:c] + a0 @ kl[:c])
            self._v6 = out
        return self._v6

    def dense_posterior(self, prior_mean):
        """(mu, var) of the reference, f64: m0 + sum_k (sf2 alpha_k) K*, sf2 - |V6|^2."""
        v2 = sum((v * v).sum(0) for v in self.v6())
        return prior_mean + self.sa @ self.k32.astype(np.float64), self.sf2 - v2

    def effect(self, rec, nI, nQ):
        """What the plan leaves out, per query: dict of dV2 [m], dVI2 [nI, m],
        dvar [m], dmu [m] and mean_lost [nQ] (k-tiles of the last row block
        absent from the records)."""
        assert nI == self.nI and nQ == self.nQ, (nI, nQ, self.nI, self.nQ)
        lv = plan_levels(rec, nI, nQ)
        kh, km, kl = self.k
        m = self.m
        dVI2 = np.zeros((nI, m))
        dvar = np.zeros(m)
        dmu = np.zeros(m)
        mean_lost = np.zeros(nQ, np.int64)
        v6 = self.v6()
        for I in range(nI):
            r0, r1 = self._rows(I)
            c = self._cols(I)
            a0, a1, a2 = (p[r0:r1, :c].astype(np.float64) for p in self.a)
            for qb in range(nQ):
                q0, q1 = qb * BN, min((qb + 1) * BN, m)
                l = np.repeat(lv[I, qb, :4 * (I + 1)], BK)[:c, None]
                m1, m2, m3 = (l >= 1), (l >= 2), (l >= DROPPED)
                if I == nI - 1:   # (k-tiles of padding columns alone hold nothing to lose)
                    mean_lost[qb] = int((lv[I, qb, :(c + BK - 1) // BK] == DROPPED).sum())
                if not m1.any():
                    continue
                # omitted from level 1 up: a2 kh + a1 km + a0 kl; from level 2 up
                # also a1 kh + a0 km; dropped: also a0 kh.  Grouped by A piece (the
                # K* piece sums are exact in f64: the pieces' bits do not overlap).
                dv = a2 @ (kh[:c, q0:q1] * m1)
                dv += a1 @ (km[:c, q0:q1] * m1 + kh[:c, q0:q1] * m2)
                dv += a0 @ (kl[:c, q0:q1] * m1 + km[:c, q0:q1] * m2 + kh[:c, q0:q1] * m3)
                dVI2[I, q0:q1] = (dv * dv).sum(0)
                dvar[q0:q1] += (dv * (2.0 * v6[I][:, q0:q1] - dv)).sum(0)
                if I == nI - 1:
                    dmu[q0:q1] = (self.sa[:c, None] * (self.k32[:c, q0:q1].astype(np.float64) * m3)).sum(0)
        return dict(dV2=dVI2.sum(0), dVI2=dVI2, dvar=dvar, dmu=dmu, mean_lost=mean_lost)


def tau2(B, sf2):
    """The |dV(q)|_2 budget the builder shares over a query block's row blocks:
    refresh_skip_budget (sbo_api.cpp) hands skip_cutoffs tau2 = 2^-B sqrt(sf2)
    / 2 * 0.99 (the 1 % pays for the |dV|^2 term of the variance); skip_cutoffs
    stores lg_tau = log2(tau2 / sqrt(nI)) and plan_ref (kernels.hip) turns it
    back into the block's reference budget lg_tau + log2(nI) / 2 - 1e-4, i.e.
    tau2 less a rounding guard.  The guard sits below tau2, so tau2 is the
    inequality the plan has to meet."""
    return 2.0 ** -B * np.sqrt(sf2) / 2.0 * 0.99


def check(model, rec, nI, nQ, B, var_budget=None):
    """The three worst-case ratios of a plan against budget B and the query
    attaining each: 'V' |dV(q)|_2 / tau2, 'var' |dvar(q)| / (2^-B sf2) (or
    var_budget), 'mu' |dmu(q)| / (2^-B sqrt(sf2)); plus the effect itself."""
    e = model.effect(rec, nI, nQ)
    sf2 = model.sf2
    rV = np.sqrt(e["dV2"]) / tau2(B, sf2)
    rvar = np.abs(e["dvar"]) / (2.0 ** -B * sf2 if var_budget is None else var_budget)
    rmu = np.abs(e["dmu"]) / (2.0 ** -B * np.sqrt(sf2))
    out = {}
    for name, r in (("V", rV), ("var", rvar), ("mu", rmu)):
        q = int(np.argmax(r))
        out[name] = (float(r[q]), q)
    out["effect"] = e
    return out
