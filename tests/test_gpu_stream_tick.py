"""sbo_tick_stream: the planning tick with a kept posterior (include/sbo.h,
csrc/predict_update.hip) through the C ABI on cuda:0.

Unless a test says otherwise: default hyper-parameters, training points
uniform over a square of about 8 points per l^2, a 37 x 29 raster grid
(m = 1073, no multiple of 128) reaching 0.3 beyond the data box, the oracle is
oracle.predict given the device factor, and every comparison runs over all m
points.  The contract is 1e-5 normwise (max |d| / max |ref|) on mu and sigma^2.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from safe_bayesian_optimization_amd import TerrainMapper  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.dist import key_tensor_to_pairs  # noqa: E402
from safe_bayesian_optimization_amd.terrain import Hyper, normal, smooth_field, uniform  # noqa: E402
from tests import stream_model as SM  # noqa: E402

REL_TOL = 1e-5
BETA = 2.0


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
    """n_total training points (fitted and appended in the caller's order), a
    raster grid over their box and one mapper."""

    def __init__(self, dev, n_total, seed=1, x_range=None, y_range=None, grid=(37, 29), hyper=None, options=()):
        self.dev = dev
        self.hyper = hyper or Hyper()
        side = self.hyper.length_scale * np.sqrt(n_total / 8.0)
        (x0, x1), (y0, y1) = x_range or (0.0, side), y_range or (0.0, side)
        u = uniform(seed, 2 * n_total)
        self.x = f32(x0 + u[0::2] * (x1 - x0))
        self.y = f32(y0 + u[1::2] * (y1 - y0))
        field = smooth_field(self.x - x0, self.y - y0, max(x1 - x0, y1 - y0), self.hyper.length_scale, seed)
        self.obs = f32(field + np.sqrt(self.hyper.sn2) * normal(seed + 1, n_total))
        self.f_min = float(np.percentile(self.obs, 40.0))
        gx = np.linspace(x0 - 0.3, x1 + 0.3, grid[0])
        gy = np.linspace(y0 - 0.3, y1 + 0.3, grid[1])
        QY, QX = np.meshgrid(gy, gx, indexing="ij")
        self.set_queries(QX.reshape(-1), QY.reshape(-1))
        self.gm = TerrainMapper(0, self.hyper)
        for opt, val in options:
            self.gm.set_option(opt, val)
        self.n = 0

    def set_queries(self, qx, qy):
        self.qx, self.qy = f32(qx), f32(qy)
        self.m = self.qx.size
        self.dqx, self.dqy = self.t(self.qx), self.t(self.qy)

    def t(self, a):
        return torch.tensor(f32(a), device=self.dev)

    def fit(self, n0):
        self.gm.fit(self.t(self.x[:n0]), self.t(self.y[:n0]), self.t(self.obs[:n0]))
        self.n = n0

    def append(self, b):
        a, self.n = self.n, self.n + b
        self.gm.append(self.t(self.x[a:self.n]), self.t(self.y[a:self.n]), self.t(self.obs[a:self.n]))

    def outputs(self):
        m, dev = self.m, self.dev
        return dict(mu=torch.empty(m, dtype=torch.float32, device=dev),
                    sd=torch.empty(m, dtype=torch.float32, device=dev),
                    lo=torch.empty(m, dtype=torch.float64, device=dev),
                    hi=torch.empty(m, dtype=torch.float64, device=dev),
                    safe=torch.empty(m, dtype=torch.uint8, device=dev))

    def tick(self, stream=True, **kw):
        """(host outputs, (score, index)) of one device-pointer tick."""
        outs = self.outputs()
        fn = self.gm.tick_stream if stream else self.gm.tick
        key = fn(self.dqx, self.dqy, BETA, self.f_min, outputs=outs, **kw)
        torch.cuda.synchronize()
        (pair,) = key_tensor_to_pairs(key)
        return {k: v.cpu().numpy() for k, v in outs.items()}, pair

    def tick_host(self, stream=True, **kw):
        outs = dict(mu=np.empty(self.m, np.float32), sd=np.empty(self.m, np.float32),
                    lo=np.empty(self.m, np.float64), hi=np.empty(self.m, np.float64),
                    safe=np.empty(self.m, np.uint8))
        fn = self.gm.tick_stream if stream else self.gm.tick
        key = fn(self.qx, self.qy, BETA, self.f_min, outputs=outs, **kw)
        return outs, (key.score, int(key.idx))

    def factor64(self):
        """(L f64 dense lower, x, y, obs in the factor's order)."""
        L, _ = self.gm.factor()
        o = self.gm.order()
        return L.astype(np.float64), self.x[:self.n][o], self.y[:self.n][o], self.obs[:self.n][o]

    def oracle(self):
        L, alpha = self.gm.factor()
        o = self.gm.order()
        h = self.hyper
        return O.predict(O.colmajor_from_lower(L.astype(np.float64)), alpha.astype(np.float64), self.x[:self.n][o],
                         self.y[:self.n][o], self.qx, self.qy, h.length_scale, h.sf2, h.prior_mean)

    def posterior_errors(self, h):
        omu, ovar = self.oracle()
        return nrel(h["mu"], omu), nrel(h["sd"].astype(np.float64) ** 2, ovar)


def same(a, b):
    """Two ticks' outputs and keys, bit for bit."""
    (ha, ka), (hb, kb) = a, b
    return ka == kb and all(np.array_equal(ha[k], hb[k]) for k in ("mu", "sd", "lo", "hi", "safe"))


def check_sets_and_key(h, key, f_min, index_offset=0, ucb=False):
    """lo/hi/S and the key are the oracle's ComputeSets and masked argmax of
    the tick's own mu/sigma, bit for bit."""
    olo, ohi, osafe = O.compute_sets(h["mu"], h["sd"], BETA, f_min)
    assert np.array_equal(h["lo"], olo) and np.array_equal(h["hi"], ohi) and np.array_equal(h["safe"], osafe)
    oidx, oval = O.argmax(ohi if ucb else ohi - olo, osafe)
    assert key[1] == (oidx + index_offset if oidx >= 0 else -1), (key, oidx)
    if oidx >= 0:
        assert key[0] == oval


def test_first_call_is_the_tick(dev):
    r = Rig(dev, 200)
    r.fit(200)
    ref = r.tick(stream=False)
    got = r.tick()
    info = r.gm.stream_info()
    assert same(ref, got)
    assert (info["path"], info["reason"], info["m"]) == (0, "FIRST", r.m)
    assert same(ref, r.tick(stream=False))   # sbo_tick itself is untouched by the kept posterior


# More than 64 appended rows: the update kernel's eight-block instantiation
# (65 .. 128 rows) and its second pass over the tiles (more than 128), under
# SBO_OPT_STREAM_MAX_ROWS 256.  (300, 65): a fifth row block of one row, n = 365
# ends in a 45-column k-tile; (650, 150): the second pass's last block holds six
# rows, n = 800 ends in a 32-column tile.  Neither append re-sorts
# (SBO_OPT_RESORT 25: 100 b <= 25 n0) or refits (b <= 256, so z stays current).
WIDE_SHAPES = [(300, 65), (650, 150)]


def wide_options(b):
    return [(N.SBO_OPT_STREAM_MAX_ROWS, 256)] if b > 64 else []


@pytest.mark.parametrize("b,n0", [(b, n0) for n0 in [200, 250] for b in [1, 16, 17, 33]]
                         + [(b, n0) for n0, b in WIDE_SHAPES])
def test_update_against_the_oracle(dev, n0, b):
    """n crosses a 64-column k-tile (250 -> 256+) and the 256-row block; b on
    both sides of the 16-row MFMA block and of one and two blocks a pass, and
    WIDE_SHAPES."""
    r = Rig(dev, n0 + b, seed=n0 + b, options=wide_options(b))
    r.fit(n0)
    r.tick()
    r.append(b)
    h, key = r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["reason"], info["rows"], info["n_map"]) == (1, "UPDATED", b, n0)
    emu, evar = r.posterior_errors(h)
    print(f"n0 {n0} b {b}: mu {emu:.2e} var {evar:.2e} L {info['cutoff_log2']} "
          f"tiles {info['tiles_kept']}/{info['tiles_total']}")
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    check_sets_and_key(h, key, r.f_min)


def test_two_appends_before_one_tick(dev):
    r = Rig(dev, 208, seed=5)
    r.fit(200)
    r.tick()
    r.append(3)
    r.append(5)
    h, key = r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["rows"], info["n_map"]) == (1, 8, 200)
    emu, evar = r.posterior_errors(h)
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    check_sets_and_key(h, key, r.f_min)
    # nothing appended: acquisition only, the same outputs
    again = r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["reason"], info["rows"], info["updates_since_full"]) == (1, "UPDATED", 0, 2)
    assert same((h, key), again)


# Largest normwise deviation of the kernel's own delta from the numpy model
# measured on the MI355X over the shapes below: d mu at n0 = 250, b = 17
# (d sigma^2 at most 8.9e-16, n0 = 250, b = 33).
DELTA_MEASURED = 2.047e-15
# The same over WIDE_SHAPES, measured on the build before the two sweeps shared
# their k-tile walk (and the same figures, digit for digit, on this one): d mu
# at n0 = 650, b = 150 (more rows per sum; d sigma^2 at most 1.22e-15).
DELTA_MEASURED_WIDE = 7.717e-15


@pytest.mark.parametrize("skip", [0, 200])
@pytest.mark.parametrize("n0,b", [(200, 1), (250, 17), (250, 33)] + WIDE_SHAPES)
def test_kernel_delta_against_the_model(dev, skip, n0, b):
    """The kept f64 state before and after one update, dense
    (SBO_OPT_TILE_SKIP 0: the caller's order; 200: the same arithmetic under the
    sweep's query order), against the model's d sigma^2 and d mu from the
    device's own factor: max |d_dev - d_model| / max sigma^2 (resp. max |mu|).
    Tolerance: 16 x the largest deviation measured over these shapes on the
    MI355X, DELTA_MEASURED = 2.047e-15 (measured: d sigma^2 4.5e-16 / 8.4e-16 /
    8.9e-16 and d mu 9.0e-16 / 2.0e-15 / 1.9e-15 for the three shapes, the same
    under both orders), so 3.3e-14; for WIDE_SHAPES 16 x DELTA_MEASURED_WIDE =
    7.717e-15 (measured: d sigma^2 1.02e-15 / 1.22e-15 and d mu 5.32e-15 /
    7.72e-15 for (300, 65) / (650, 150), the same under both orders), so 1.2e-13;
    whatever is measured must stay below 1e-9 -- an f32 slip anywhere in the path
    would show near 6e-8 |L^-1_r|_1, about 7e-7.  Every tile is multiplied
    (tiles_kept == tiles_total), counted on the first pass only."""
    r = Rig(dev, n0 + b, seed=3 * n0 + b, options=[(N.SBO_OPT_TILE_SKIP, skip)] + wide_options(b))
    r.fit(n0)
    r.tick()
    mu0, var0 = r.gm.stream_state(r.m)
    r.append(b)
    r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["reason"], info["rows"]) == (1, "UPDATED", b)
    assert info["tiles_kept"] == info["tiles_total"] > 0
    mu1, var1 = r.gm.stream_state(r.m)
    L, x, y, obs = r.factor64()
    dvar, dmu, _, _ = SM.update(L, x, y, obs, r.hyper.prior_mean, n0, r.qx, r.qy, r.hyper.length_scale, r.hyper.sf2)
    evar = np.abs((var1 - var0) - dvar).max() / var1.max()
    emu = np.abs((mu1 - mu0) - dmu).max() / np.abs(mu1).max()
    print(f"skip {skip} n0 {n0} b {b}: d var {evar:.3e} d mu {emu:.3e} (|d var| {np.abs(dvar).max():.2e})")
    assert np.abs(dvar).max() > 1e-3   # the update is not a no-op
    assert max(evar, emu) < 1e-9
    assert max(evar, emu) <= 16 * (DELTA_MEASURED_WIDE if (n0, b) in WIDE_SHAPES else DELTA_MEASURED), (evar, emu)


@pytest.mark.parametrize("query_order", [0, 1])
def test_scattered_queries_host_pointers_offset_and_ucb(dev, query_order):
    r = Rig(dev, 208, seed=9, options=[(N.SBO_OPT_QUERY_ORDER, query_order)])
    u = uniform(77, 260)
    r.set_queries(-0.3 + u[0::2] * (r.x.max() + 0.6), -0.3 + u[1::2] * (r.y.max() + 0.6))
    assert r.m == 130
    kw = dict(score=N.SCORE_UCB, index_offset=1000)
    r.fit(200)
    r.tick(**kw)
    r.append(5)
    d = r.tick(**kw)                     # device pointers run the update ...
    assert r.gm.stream_info()["rows"] == 5
    hst = r.tick_host(**kw)              # ... host pointers the acquisition from the same state
    info = r.gm.stream_info()
    assert (info["path"], info["reason"], info["rows"]) == (1, "UPDATED", 0)
    assert same(d, hst)
    emu, evar = r.posterior_errors(d[0])
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    check_sets_and_key(d[0], d[1], r.f_min, index_offset=1000, ucb=True)
    r.append(3)
    hst = r.tick_host(**kw)              # and the other way round
    assert (r.gm.stream_info()["path"], r.gm.stream_info()["rows"]) == (1, 3)
    d = r.tick(**kw)
    assert same(d, hst)
    emu, evar = r.posterior_errors(d[0])
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    check_sets_and_key(d[0], d[1], r.f_min, index_offset=1000, ucb=True)


def ev_resort(r):
    r.append(60)        # 30 % of the sorted points: SBO_OPT_RESORT re-sorts and refactors


def ev_refit(r):
    r.fit(200)


def ev_ulp(r):
    qx = r.qx.copy()
    qx[517] = np.nextafter(qx[517], np.float32(np.inf))
    r.set_queries(qx, r.qy)


def ev_other_m(r):
    r.set_queries(r.qx[:-1], r.qy[:-1])


def ev_hyper(r):
    r.gm.hyper = Hyper(length_scale=0.5)
    r.hyper = r.gm.hyper
    r.fit(200)


def ev_import(r):
    src = Rig(r.dev, 230, seed=21)
    src.fit(230)
    r.gm.import_state(src.gm.export_state())
    src.gm.close()


def ev_inverse32(r):
    r.gm.set_option(N.SBO_OPT_INVERSE_BITS, 32)
    r.append(5)


def ev_reset(r):
    r.gm.stream_reset()


def ev_rows_over_cap(r):
    r.gm.set_option(N.SBO_OPT_STREAM_MAX_ROWS, 8)
    r.append(9)


@pytest.mark.parametrize("event,reason", [
    (ev_resort, "REFIT"), (ev_refit, "REFIT"), (ev_ulp, "QUERIES_CHANGED"), (ev_other_m, "QUERIES_CHANGED"),
    (ev_hyper, "REFIT"), (ev_import, "REFIT"), (ev_inverse32, "NO_INVERSE"), (ev_reset, "RESET"),
    (ev_rows_over_cap, "ROWS_OVER_CAP")], ids=lambda v: getattr(v, "__name__", v))
def test_every_fallback_is_the_full_tick(dev, event, reason):
    r = Rig(dev, 260, seed=13)
    r.fit(200)
    r.tick()
    event(r)
    got = r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["reason"]) == (0, reason), info
    assert same(got, r.tick(stream=False))
    # the full path kept its posterior: the next call is an (empty) update of
    # it, unless the context has no f64 inverse to update from at all
    assert same(got, r.tick())
    info = r.gm.stream_info()
    if event in (ev_import, ev_inverse32):
        assert (info["path"], info["reason"]) == (0, "NO_INVERSE"), info
    else:
        assert (info["path"], info["reason"], info["rows"]) == (1, "UPDATED", 0), info


def test_rows_at_the_cap_still_update(dev):
    r = Rig(dev, 208, seed=13, options=[(N.SBO_OPT_STREAM_MAX_ROWS, 8)])
    r.fit(200)
    r.tick()
    r.append(8)
    r.tick()
    assert r.gm.stream_info()["reason"] == "UPDATED"


@pytest.mark.parametrize("b", [1, 16])
def test_precise_regime(dev, b):
    """SBO_OPT_PRECISION 1 on the mapping node's own box: the update of the
    precise sweep's posterior stays inside the contract."""
    r = Rig(dev, 500 + b, seed=17, x_range=(0.0, 1.0), y_range=(0.0, 2.5), options=[(N.SBO_OPT_PRECISION, 1)])
    r.fit(500)
    assert r.gm.precision()[0]
    r.tick()
    r.append(b)
    h, key = r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["rows"]) == (1, b)
    emu, evar = r.posterior_errors(h)
    print(f"precise b {b}: mu {emu:.2e} var {evar:.2e} L {info['cutoff_log2']}")
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    check_sets_and_key(h, key, r.f_min)


def test_cutoff_spends_no_more_than_its_bound(dev):
    """n0 = 2048 on a box of side 16 l, a 48 x 48 grid, b = 4: three contexts
    capture the same posterior under the automatic cutoff, then update it
    under the automatic cutoff, dense (0) and with L = 150."""
    ell = Hyper().length_scale
    box = (0.0, 16 * ell)
    rigs = {s: Rig(dev, 2052, seed=31, x_range=box, y_range=box, grid=(48, 48)) for s in (-1, 0, 150)}
    state = {}
    for s, r in rigs.items():
        r.fit(2048)
        r.tick()
        before = r.gm.stream_state(r.m)
        r.gm.set_option(N.SBO_OPT_TILE_SKIP, s)
        r.append(4)
        r.tick()
        state[s] = (before, r.gm.stream_state(r.m), r.gm.stream_info())
    for s in (0, 150):   # the same starting point in all three
        assert np.array_equal(state[s][0][0], state[-1][0][0]) and np.array_equal(state[s][0][1], state[-1][0][1])
    info = state[-1][2]
    assert info["path"] == 1 and 16 <= info["cutoff_log2"] < 150
    # on the CPU: (8 x 16 grid patch, k-tile) pairs beyond the cutoff radius exist
    r = rigs[-1]
    o = r.gm.order()
    tiles = SM.tile_boxes(r.x[o], r.y[o])
    QX, QY = r.qx.reshape(48, 48), r.qy.reshape(48, 48)
    patches = [(QX[i:i + 16, j:j + 8].min(), QX[i:i + 16, j:j + 8].max(), QY[i:i + 16, j:j + 8].min(),
                QY[i:i + 16, j:j + 8].max()) for i in range(0, 48, 16) for j in range(0, 48, 8)]
    r2 = 2.0 * ell * ell * np.log(2.0) * info["cutoff_log2"] / 0.999
    far = sum(SM.box_distance2(t, p) > r2 * 1.001 for t in tiles for p in patches)
    print(f"cutoff L {info['cutoff_log2']}: tiles {info['tiles_kept']}/{info['tiles_total']}, "
          f"{far} pairs beyond the radius on the CPU; err_var {info['err_var']:.2e} err_mean {info['err_mean']:.2e}")
    assert far > 0
    assert info["tiles_total"] == len(tiles) * len(patches)
    assert info["tiles_kept"] < info["tiles_total"]
    assert 0 < info["err_var"] <= info["budget_var"] and 0 < info["err_mean"] <= info["budget_mean"]
    (mu_a, var_a), (mu_d, var_d) = state[-1][1], state[0][1]
    dvar, dmu = np.abs(var_a - var_d).max(), np.abs(mu_a - mu_d).max()
    print(f"cutoff against dense: d var {dvar:.2e} d mu {dmu:.2e}")
    assert dvar <= info["err_var"] and dmu <= info["err_mean"]
    assert state[0][2]["tiles_kept"] == state[0][2]["tiles_total"] and state[0][2]["err_var"] == 0.0
    # L >= 150 drops exact zeros only (its radius, 14.4 l, leaves few or no pairs to drop on this box)
    print(f"L 150: tiles {state[150][2]['tiles_kept']}/{state[150][2]['tiles_total']}")
    assert state[150][2]["cutoff_log2"] == 150 and state[150][2]["err_var"] == 0.0
    assert np.array_equal(state[150][1][0], mu_d) and np.array_equal(state[150][1][1], var_d)


@pytest.mark.parametrize("share,second", [(0, "BUDGET"), (10, "UPDATED")])
def test_budget(dev, share, second):
    r = Rig(dev, 202, seed=41, options=[(N.SBO_OPT_STREAM_SHARE, share)])
    r.fit(200)
    r.tick()
    r.append(1)
    r.tick()
    info = r.gm.stream_info()
    assert (info["path"], info["reason"]) == (1, "UPDATED")
    assert 0 < info["err_var"] <= info["budget_var"] * 2.0 ** -share
    assert info["err_mean"] <= info["budget_mean"] * 2.0 ** -share
    r.append(1)
    got = r.tick()
    info = r.gm.stream_info()
    print(f"share {share}: second call {info['reason']} err_var {info['err_var']:.2e} of {info['budget_var']:.2e}")
    assert info["reason"] == second and info["path"] == (1 if second == "UPDATED" else 0)
    if second == "BUDGET":
        assert same(got, r.tick(stream=False))
        assert info["err_var"] == 0.0 and info["updates_since_full"] == 0


def run_loop(dev):
    r = Rig(dev, 600, seed=51)
    r.fit(300)
    steps = [r.tick()]
    reasons = []
    for _ in range(10):
        r.append(30)
        steps.append(r.tick())
        reasons.append(r.gm.stream_info()["reason"])
    return r, steps, reasons


def test_loop_is_deterministic_and_stays_in_the_contract(dev):
    """n 300 -> 600 in ten appends of 30 with a tick each (SBO_OPT_RESORT
    re-sorts on the way: those ticks are full sweeps), twice."""
    r, steps, reasons = run_loop(dev)
    r2, steps2, reasons2 = run_loop(dev)
    assert reasons == reasons2 and "REFIT" in reasons and reasons.count("UPDATED") >= 6, reasons
    assert all(same(a, b) for a, b in zip(steps, steps2))
    h, key = steps[-1]
    emu, evar = r.posterior_errors(h)
    ht, _ = r.tick(stream=False)
    dmu = nrel(h["mu"], ht["mu"].astype(np.float64))
    dvar = nrel(h["sd"].astype(np.float64) ** 2, ht["sd"].astype(np.float64) ** 2)
    print(f"loop: {reasons}; oracle mu {emu:.2e} var {evar:.2e}; against sbo_tick mu {dmu:.2e} var {dvar:.2e}")
    assert emu < REL_TOL and evar < REL_TOL, (emu, evar)
    assert dmu <= 2e-5 and dvar <= 2e-5, (dmu, dvar)
    check_sets_and_key(h, key, r.f_min)
