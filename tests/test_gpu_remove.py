"""sbo_remove (include/sbo.h, csrc/remove.hip) through the C ABI on cuda:0:
training points leave the f32 factor L and the f64 inverse X = L^-1 by Givens
rotations, against the f64 model of tests/remove_model.py and the oracle
fitted on the points that remain.

Unless a test says otherwise: default hyper-parameters, training points
uniform over a square of about 8 points per l^2, the 37 x 29 raster grid of
tests/test_gpu_stream_tick.py reaching 0.3 beyond the data box, oracle.fit /
oracle.predict in f64 on the remaining points compared over every grid point
(the 1e-5 normwise contract, max |d| / max |ref|, on mu and sigma^2),
SBO_OPT_RESORT 0 and SBO_OPT_REMOVE_MAX 64.  The sizes are the smallest that
cross every boundary the kernels have: 128-column chain steps, 256-row row
blocks, 64-point k-tiles and 64-column strips of X, a partial last block, and
ld != n.

Factor and inverse against the model, normwise max |d| / max |model|:
  L' within 2^-22: one f32 rounding of an f64 result (2^-24 relative to the
     largest entry or below), with a factor 4 for the last f64 bits moving it;
  X' within 1e-9: about 8 x the first-order worst case n^2 2^-53 / sqrt(noise)
     ~ 1.3e-10, and 60 x below what one f32 intermediate would leave (6e-8).
Measured on an MI355X: L' 4.0e-8 at worst (one point at position 0; the
batch of 17: 3.5e-8), X' 7.3e-16 (the batch); the posterior after a removal
within 2.7e-6 (mu) and 1.3e-6 (variance) of the oracle.
The evidence after a removal is held to the model from scratch on the
remaining points within tests/test_gpu_evidence.py's end-to-end tolerance (the
rotated inverse is the inverse of the f64 rotated factor, which the stored
f32 factor rounds: the "given the device factor" reference of that file does
not apply).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from safe_bayesian_optimization_amd import TerrainMapper  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.terrain import Hyper, normal, smooth_field, uniform  # noqa: E402
from tests import evidence_model as EM  # noqa: E402
from tests import remove_model as RM  # noqa: E402
from tests.test_gpu_evidence import E2E_TOL  # noqa: E402

REL_TOL = 1e-5
BETA = 2.0
L_TOL = 2.0 ** -22
X_TOL = 1e-9
ALPHA_TOL = 1e-3
HYPER = Hyper()
DEFAULT_OPTIONS = ((N.SBO_OPT_RESORT, 0), (N.SBO_OPT_REMOVE_MAX, 64))
SBO_E_INVAL, SBO_E_EMPTY, SBO_E_STATE = 1, 5, 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def nrel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


class Rig:
    """A pool of n_total points, the raster grid over their box, one mapper,
    and the caller's view of what the mapper holds (cx, cy, cobs in the
    caller's numbering: fitted, appended, numpy.delete'd)."""

    def __init__(self, n_total, seed=1, options=DEFAULT_OPTIONS, grid=(37, 29)):
        h = HYPER
        side = h.length_scale * np.sqrt(n_total / 8.0)
        u = uniform(seed, 2 * n_total)
        self.x, self.y = f32(u[0::2] * side), f32(u[1::2] * side)
        field = smooth_field(self.x, self.y, side, h.length_scale, seed)
        self.obs = f32(field + np.sqrt(h.sn2) * normal(seed + 1, n_total))
        self.f_min = float(np.percentile(self.obs, 40.0))
        gx = np.linspace(-0.3, side + 0.3, grid[0])
        gy = np.linspace(-0.3, side + 0.3, grid[1])
        QY, QX = np.meshgrid(gy, gx, indexing="ij")
        self.qx, self.qy = f32(QX.reshape(-1)), f32(QY.reshape(-1))
        self.m = self.qx.size
        self.gm = TerrainMapper(0, h)
        for opt, val in options:
            self.gm.set_option(opt, val)
        self.used = 0
        self.cx = self.cy = self.cobs = np.empty(0, np.float32)

    def fit(self, n0):
        self.used = n0
        self.cx, self.cy, self.cobs = self.x[:n0].copy(), self.y[:n0].copy(), self.obs[:n0].copy()
        self.gm.fit(self.cx, self.cy, self.cobs)

    def append(self, b):
        a, self.used = self.used, self.used + b
        nx, ny, no = self.x[a:self.used], self.y[a:self.used], self.obs[a:self.used]
        self.gm.append(nx, ny, no)
        self.cx, self.cy, self.cobs = (np.concatenate(p) for p in ((self.cx, nx), (self.cy, ny), (self.cobs, no)))

    def remove(self, idx):
        info = self.gm.remove(idx)
        idx = np.asarray(list(idx), np.int64)
        self.cx, self.cy, self.cobs = (np.delete(a, idx) for a in (self.cx, self.cy, self.cobs))
        return info

    def tick(self, stream=False):
        outs = dict(mu=np.empty(self.m, np.float32), sd=np.empty(self.m, np.float32),
                    lo=np.empty(self.m, np.float64), hi=np.empty(self.m, np.float64),
                    safe=np.empty(self.m, np.uint8))
        fn = self.gm.tick_stream if stream else self.gm.tick
        key = fn(self.qx, self.qy, BETA, self.f_min, outputs=outs)
        return outs, (key.score, int(key.idx))

    def oracle(self):
        h = HYPER
        Lcm, alpha = O.fit(self.cx, self.cy, self.cobs, h.length_scale, h.sf2, h.sn2, h.prior_mean)
        return O.predict(Lcm, alpha, self.cx, self.cy, self.qx, self.qy, h.length_scale, h.sf2, h.prior_mean)

    def posterior_errors(self, outs=None):
        """(mu error, variance error) of a tick against the oracle, and the oracle's (mu, var)."""
        outs = outs or self.tick()[0]
        omu, ovar = self.oracle()
        e = nrel(outs["mu"], omu), nrel(outs["sd"].astype(np.float64) ** 2, ovar)
        print(f"n {self.gm.n}: mu {e[0]:.2e} var {e[1]:.2e}")
        return e, (omu, ovar)

    def check_posterior(self, outs=None):
        (emu, evar), o = self.posterior_errors(outs)
        assert emu <= REL_TOL and evar <= REL_TOL, (emu, evar)
        return o

    def check_order(self):
        """The stored points are the caller's, in sbo_get_order's numbering:
        order is a permutation, and the device's alpha of stored row i is the
        oracle's alpha of caller index order[i].  ALPHA_TOL: the f32 factor's
        error, eps_f32 cond(K) with cond(K) <= (n sf2 + sn2) / sn2 ~ 6e3 at
        n = 600, is 4e-4; a point behind the wrong index moves alpha by O(1)."""
        h = HYPER
        o = self.gm.order()
        assert np.array_equal(np.sort(o), np.arange(self.cx.size))
        _, alpha = O.fit(self.cx, self.cy, self.cobs, h.length_scale, h.sf2, h.sn2, h.prior_mean)
        e = nrel(self.gm.factor()[1], alpha[o])
        print(f"alpha in the caller's numbering: {e:.2e}")
        assert e <= ALPHA_TOL
        return o

    def state(self):
        s = (ctypes.c_int64 * 13)()
        assert N.lib().sbo_debug_state(self.gm.ctx.handle, s, 13) == 0
        return list(s)


def same(a, b):
    (ha, ka), (hb, kb) = a, b
    return ka == kb and all(np.array_equal(ha[k], hb[k]) for k in ("mu", "sd", "lo", "hi", "safe"))


def remove_and_compare(rig, positions):
    """Remove the points stored at `positions`; the device's L' and X' against
    the model applied to the values read before.  Returns (info, dL, dX)."""
    gm = rig.gm
    n = gm.n
    L0 = gm.factor()[0].astype(np.float64)
    X0 = gm.inverse64()
    order0 = gm.order()
    state0 = rig.state()
    idx = order0[np.asarray(positions)]
    info = rig.remove(idx)
    pos, new_order = RM.remove_map(order0, idx)
    assert np.array_equal(pos, np.sort(positions))
    assert gm.n == n - len(positions) == info["n"]
    assert np.array_equal(gm.order(), new_order)
    assert info["path"] == 1 and info["reason"] == "DOWNDATED" and info["removed"] == len(positions)
    assert info["first_row"] == min(positions)
    assert info["rotations"] == sum(n - 1 - p for p in positions)
    state1 = rig.state()
    assert state1[0] == state1[4] == state1[5] == gm.n and state1[12] > state0[12]
    Lm, Xm = RM.remove(L0, X0, positions)
    L1 = gm.factor()[0].astype(np.float64)
    X1 = gm.inverse64()
    dL, dX = nrel(L1, Lm), nrel(X1, Xm)
    print(f"positions {list(positions)[:6]}{'...' if len(positions) > 6 else ''}: L' {dL:.3e} (2^-22 = {L_TOL:.3e}) "
          f"X' {dX:.3e}")
    return info, dL, dX


# ------------------------------------------------- 1. factor and inverse
@pytest.fixture(scope="module")
def rig600(dev):
    return Rig(600)


@pytest.mark.parametrize("position", [0, 127, 128, 255, 256, 599])
def test_one_point_matches_model(rig600, position):
    rig600.fit(600)
    _, dL, dX = remove_and_compare(rig600, [position])
    assert dL <= L_TOL and dX <= X_TOL


@pytest.fixture(scope="module")
def batch(rig600):
    """Fit 600 and remove 17 random stored positions in one call; kept for the tests below."""
    rig600.fit(600)
    positions = sorted(int(p) for p in np.random.default_rng(3).choice(600, 17, replace=False))
    info, dL, dX = remove_and_compare(rig600, positions)
    outs, key = rig600.tick()
    return dict(rig=rig600, info=info, dL=dL, dX=dX, outs=outs, key=key)


def test_batch_matches_model(batch):
    assert batch["dL"] <= L_TOL and batch["dX"] <= X_TOL


# ------------------------------------------------ 2. posterior against the oracle
def test_batch_posterior_and_sets(batch):
    rig = batch["rig"]
    omu, ovar = rig.check_posterior(batch["outs"])
    # a second mapper fitted on the remaining points: the same safe set
    # wherever the oracle's lower bound is further from f_min than the
    # contract lets either mapper move it (|d mu| <= tol max |mu|, |d sd| <=
    # sqrt(|d var|) <= sqrt(tol max var)), and the same key up to that margin
    other = TerrainMapper(0, HYPER)
    other.fit(rig.cx, rig.cy, rig.cobs)
    o2 = dict(mu=np.empty(rig.m, np.float32), sd=np.empty(rig.m, np.float32), lo=np.empty(rig.m, np.float64),
              hi=np.empty(rig.m, np.float64), safe=np.empty(rig.m, np.uint8))
    k2 = other.tick(rig.qx, rig.qy, BETA, rig.f_min, outputs=o2)
    margin = REL_TOL * np.abs(omu).max() + BETA * np.sqrt(REL_TOL * ovar.max())
    olo = omu - BETA * np.sqrt(np.maximum(ovar, 0.0))
    clear = np.abs(olo - rig.f_min) > margin
    assert clear.sum() > rig.m // 2
    assert np.array_equal(batch["outs"]["safe"][clear], o2["safe"][clear])
    assert np.array_equal(batch["outs"]["safe"][clear], (olo > rig.f_min)[clear].astype(np.uint8))
    (s1, i1), (s2, i2) = batch["key"], (k2.score, int(k2.idx))
    assert abs(s1 - s2) <= 2.0 * margin
    if i1 != i2:   # two widths within the margin of each other
        w2 = o2["hi"] - o2["lo"]
        assert abs(w2[i1] - w2[i2]) <= 2.0 * margin


# ------------------------------------------------ 3. row block lost, ld != n
def test_row_block_lost_with_grown_capacity(dev):
    rig = Rig(530, seed=2)
    rig.fit(500)
    rig.append(30)                       # the capacity grows past n: ld != n
    assert rig.state()[1] == 768
    idx = np.random.default_rng(5).choice(530, 19, replace=False)
    info = rig.remove(idx)
    assert info["path"] == 1 and rig.gm.n == 511 and rig.state()[1] == 512
    rig.check_order()
    rig.check_posterior()


def test_row_block_lost_by_one_point(dev):
    rig = Rig(513, seed=3)
    rig.fit(513)
    assert rig.state()[1] == 768
    info = rig.remove([int(rig.gm.order()[300])])
    assert info["path"] == 1 and info["first_row"] == 300 and rig.gm.n == 512 and rig.state()[1] == 512
    rig.check_posterior()


def test_last_stored_point_on_a_row_block_edge(dev):
    """first_row == the new n == a multiple of 256: nothing left to rotate or move."""
    rig = Rig(513, seed=4)
    rig.fit(513)
    info = rig.remove([int(rig.gm.order()[512])])
    assert info["path"] == 1 and info["first_row"] == 512 and info["rotations"] == 0 and rig.state()[1] == 512
    rig.check_posterior()


# ------------------------------------------------ 4. append after remove
def test_append_after_remove(dev):
    rig = Rig(610, seed=6)
    rig.fit(600)
    rig.remove(np.random.default_rng(7).choice(600, 10, replace=False))
    rig.append(10)
    assert rig.gm.n == 600
    o = rig.check_order()
    assert np.array_equal(np.sort(o[-10:]), np.arange(590, 600))
    rig.check_posterior()


# ------------------------------------------------ 5. sliding window
def test_sliding_window(dev):
    rig = Rig(440, seed=8)
    rig.fit(400)
    for rnd in range(1, 41):
        info = rig.gm.forget_oldest(1)
        rig.cx, rig.cy, rig.cobs = rig.cx[1:], rig.cy[1:], rig.cobs[1:]
        assert info["path"] == 1
        rig.append(1)
        if rnd % 10 == 0:
            assert rig.gm.n == 400
            rig.check_posterior()
    rig.check_order()


# ------------------------------------------------ 6. readers after a removal
def test_evidence_after_removal(batch):
    rig = batch["rig"]
    h = HYPER
    info = N.sbo_evidence_info()
    info.struct_size = ctypes.sizeof(info)
    n = rig.gm.n
    mean, var = np.full(n, np.nan), np.full(n, np.nan)
    st = N.lib().sbo_evidence(rig.gm.ctx.handle, ctypes.byref(info), ctypes.c_void_p(mean.ctypes.data),
                              ctypes.c_void_p(var.ctypes.data), 0)
    assert st == 0, N.lib().sbo_last_error(rig.gm.ctx.handle)
    ref = EM.evidence(rig.cx, rig.cy, rig.cobs, h.length_scale, h.sigma_f, h.noise_level, h.prior_mean)
    got = dict(lml=info.lml, data_fit=info.data_fit, log_det=info.log_det, loo_log_pred=info.loo_log_pred,
               grad=np.array(info.grad[:]), loo_mean=mean, loo_var=var)
    for k, v in got.items():
        d = nrel(np.atleast_1d(v), np.atleast_1d(np.asarray(ref[k], np.float64)))
        print(f"{k}: {d:.2e}")
        assert d <= E2E_TOL, (k, d)


def test_kept_posterior_readers_wait_for_a_tick(dev):
    rig = Rig(600, seed=9)
    rig.fit(600)
    rig.tick(stream=True)
    cx, cy = rig.qx[:4].copy(), rig.qy[:4].copy()
    rig.gm.whatif(cx, cy, BETA, rig.f_min)
    rig.gm.sample(2, 1, BETA, rig.f_min, features=64)
    rig.remove([5, 17, 300])
    for call in (lambda: rig.gm.whatif(cx, cy, BETA, rig.f_min), lambda: rig.gm.sample(2, 1, BETA, rig.f_min, features=64)):
        with pytest.raises(N.SboError) as e:
            call()
        assert e.value.status == SBO_E_STATE
    streamed = rig.tick(stream=True)
    si = rig.gm.stream_info()
    assert si["path"] == 0 and si["reason"] == "REFIT"
    assert same(streamed, rig.tick(stream=False))
    rig.gm.whatif(cx, cy, BETA, rig.f_min)
    assert rig.gm.sample(2, 1, BETA, rig.f_min, features=64)["n"] == 597


# ------------------------------------------------ 7. refit paths
REFIT_CASES = {
    "NO_INVERSE": (((N.SBO_OPT_INVERSE_BITS, 32),), 5),
    "OVER_CAP": (((N.SBO_OPT_REMOVE_MAX, 4),), 5),
    "RESORT": (((N.SBO_OPT_RESORT, 25), (N.SBO_OPT_REMOVE_MAX, 256)), 156),       # 26 % of 600
}


@pytest.mark.parametrize("reason", list(REFIT_CASES))
def test_refit_paths(dev, reason):
    extra, b = REFIT_CASES[reason]
    idx = np.random.default_rng(13).choice(600, b, replace=False)
    rot = Rig(600, seed=10, options=DEFAULT_OPTIONS + ((N.SBO_OPT_REMOVE_MAX, 256),))
    rot.fit(600)
    order0 = rot.gm.order()
    assert rot.remove(idx)["path"] == 1
    rig = Rig(600, seed=10, options=DEFAULT_OPTIONS + extra)
    rig.fit(600)
    bounds = rig.gm.bounds()
    info = rig.remove(idx)
    assert info["path"] == 0 and info["reason"] == reason and info["n"] == 600 - b == rig.gm.n
    assert rig.gm.bounds() == bounds
    # the same caller numbering as the rotation path gives: the same point
    # behind every index (the stored order differs: the refit sorts again)
    assert np.array_equal(rot.gm.order(), RM.remove_map(order0, idx)[1])
    rot.check_order()
    rig.check_order()
    rig.check_posterior()


# ------------------------------------------------ 8. arguments and state
def test_rejected_calls_change_nothing(dev):
    rig = Rig(300, seed=11)
    rig.fit(300)
    lib, hnd = N.lib(), rig.gm.ctx.handle
    order0, tick0 = rig.gm.order(), rig.tick()

    def call(idx, b=None):
        a = np.ascontiguousarray(idx, np.int64)
        return lib.sbo_remove(hnd, ctypes.c_void_p(a.ctypes.data) if a.size else None, a.size if b is None else b,
                              None, 0)

    assert call([], 1) == SBO_E_INVAL                      # NULL idx with b > 0
    assert call([1], -1) == SBO_E_INVAL
    assert call([-1]) == SBO_E_INVAL
    assert call([300]) == SBO_E_INVAL
    assert call([7, 7]) == SBO_E_INVAL
    assert call(np.arange(300)) == SBO_E_EMPTY
    assert call([], 0) == 0                                # nothing happens
    assert rig.gm.n == 300 and np.array_equal(rig.gm.order(), order0)
    assert same(rig.tick(), tick0)


def test_unfitted_and_imported_states(dev):
    rig = Rig(300, seed=12)
    lib = N.lib()
    one = np.zeros(1, np.int64)
    assert lib.sbo_remove(rig.gm.ctx.handle, ctypes.c_void_p(one.ctypes.data), 1, None, 0) == SBO_E_STATE
    rig.fit(300)
    other = TerrainMapper(0, HYPER)
    other.import_state(rig.gm.export_state())
    assert lib.sbo_remove(other.ctx.handle, ctypes.c_void_p(one.ctypes.data), 1, None, 0) == SBO_E_STATE
    assert other.n == 300


# ------------------------------------------------ 9. repeatable and exportable
def test_repeatable_and_exportable(dev):
    idx = np.random.default_rng(17).choice(600, 9, replace=False)
    rigs = [Rig(600, seed=14), Rig(600, seed=14)]
    for r in rigs:
        r.fit(600)
        r.remove(idx)
    a, b = rigs
    assert np.array_equal(a.gm.factor()[0], b.gm.factor()[0])
    assert np.array_equal(a.gm.inverse64(), b.gm.inverse64())
    ta = a.tick()
    assert same(ta, b.tick())
    other = TerrainMapper(0, HYPER)
    other.import_state(a.gm.export_state())
    outs = dict(mu=np.empty(a.m, np.float32), sd=np.empty(a.m, np.float32), lo=np.empty(a.m, np.float64),
                hi=np.empty(a.m, np.float64), safe=np.empty(a.m, np.uint8))
    k = other.tick(a.qx, a.qy, BETA, a.f_min, outputs=outs)
    assert same(ta, (outs, (k.score, int(k.idx))))
