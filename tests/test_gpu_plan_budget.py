"""The tick plan's error budget, held to the exact f64 model of its tiles
(tests/plan_model.py).

The plan may drop a (row block, k-tile) pair of a 128-query block or run it at
three or one bf16 product(s) instead of six; in exchange every query's sigma^2
moves by at most 2^-B sf2 and its mu by at most 2^-B sqrt(sf2), B =
SBO_OPT_SKIP_BUDGET, and the builder meets that through |dV(q)|_2 <= tau2 =
0.99 2^-B sqrt(sf2) / 2.  The device's own plan (sbo_debug_plan)
goes through the model, which sums exactly the omitted products of the staged
bf16 pieces in f64: no f32 output noise enters, so the budget is asserted as
stated, with a relative 1e-12 for the model's own f64 sums (dot products of at
most 4352 terms, each an exact product of two bf16 values: n 2^-53 = 5e-13).

SBO_OPT_PRECISION 0 (the probe cannot change the sweep), SBO_OPT_QUERY_ORDER 0
(sweep position = caller index, so query block qb is queries 128 qb ..
128 qb + 127), sigma_f = 1.5 (sf2 = 2.25: the budgets' scaling by sf2 counts),
prior mean 0.25.

Queries: compact 128-query blocks built here.  8 x 16 patches at l / 4 spacing
along the line y = side / 2, their left edges from 4 l inside the data's right
edge to 12 l beyond it every 2 l -- K* falls from 1 to 2^-150, exactly zero in
f32, within 14.4 l, so every transition six -> three -> one -> dropped lies in
that stretch -- and one at 40 l; one degenerate block of 128 copies of a point
3 l out (its box has no extent: the box bound K*max is attained); a partial
last block of 50 queries 5 l out.  m = 1458 (434 at n = 4100: patches at -2 l
and 5 l, the degenerate block, 50 queries 7 l out).

Training sets: (a) `synthetic`; (b) its points with observations = prior mean
+ 1 (alpha of one sign where the data is dense: the mean's lost share adds
coherently); (c) half the points in a disc of radius 2 l at the right edge, on
the patches' line, the rest spread out, noise 0.01 (large, very unequal tile
norms; cheap and expensive row blocks in one plan); (d) (a) at 250 points plus
a block append of 70 without re-sort (across a k-tile and the row block
boundary at 256); (e) the same with a re-sorting append; (f) (a) exported and
imported into a fresh context; one n = 4100 (17 row blocks, A2 pieces down to
2^-80); (a) at n = 1100 also under variant 22 (drops only); and (g) 300 points
on a jittered lattice 3 l apart.  On (a) - (f) the bounds keep a factor 3 to 10
of room (|dV| / tau2 <= 0.30): the data is dense, L^-1 damps the smooth K*
columns, and no query aligns K* with a tile's leading singular vector.  On the
lattice the points hardly couple, A is close to a multiple of the identity,
every singular value of a tile is its norm and K* of a degenerate block is
nearly one entry: |dV| / tau2 reaches 0.91, and a builder budget one bit too
large (lg_tau + 1 where PlanRule is built) gives 1.04 to 1.87 at every B --
(g) is the case that fails under that mutation; (a) - (f) do not (0.88 at most).

Measured ratios and noise: the tests' docstrings; every case is in
profiles/plan_budget.log.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import TerrainMapper, synthetic  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.gp import Context  # noqa: E402
from safe_bayesian_optimization_amd.terrain import Hyper, synthetic_box, uniform  # noqa: E402
from tests import plan_model as PM  # noqa: E402

ELL, SIGMA_F, M0 = 0.4, 1.5, 0.25
SF2 = SIGMA_F * SIGMA_F
BUDGETS = (10, 13, 20, 27)
RTOL = 1e-12          # the model's own f64 rounding (module docstring)

# name: (n fitted, training set, appended, SBO_OPT_RESORT, kernel variant)
CASES = {
    "a300": (300, "a", 0, 25, 3),
    "b300": (300, "b", 0, 25, 3),
    "c300": (300, "c", 0, 25, 3),
    "a1100": (1100, "a", 0, 25, 3),
    "b1100": (1100, "b", 0, 25, 3),
    "c1100": (1100, "c", 0, 25, 3),
    "a1100_v22": (1100, "a", 0, 25, 22),
    "d320": (250, "a", 70, 0, 3),
    "e320": (250, "a", 70, 25, 3),
    "f300": (300, "f", 0, 25, 3),
    "a4100": (4100, "a", 0, 25, 3),
    "g300": (300, "g", 0, 25, 3),
}
# What a case's records can hold: variant 22 keeps every tile at six products (drops only); on the lattice all
# blocks but one lie beyond the data, where a kept tile runs at one product
LEVELS = {c: "six" if CASES[c][4] == 22 else ("far" if CASES[c][1] == "g" else "all") for c in CASES}


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def training(case):
    """(x, y, obs, hyper, side) of a case, all n + appended points."""
    n0, kind, add, _, _ = CASES[case]
    n = n0 + add
    noise = 0.01 if kind == "c" else 0.1
    hyper = Hyper(ELL, SIGMA_F, noise, M0)
    wl = synthetic(n, 8, 8, seed=41 + n, hyper=hyper)
    x, y, obs = wl.x.copy(), wl.y.copy(), wl.obs.copy()
    if kind == "b":
        obs = np.full(n, M0 + 1.0)
    if kind == "c":
        u = uniform(977, 2 * (n // 2))
        r, a = 2.0 * ELL * np.sqrt(u[0::2]), 2.0 * np.pi * u[1::2]
        x[:n // 2] = wl.side - 2.0 * ELL + r * np.cos(a)
        y[:n // 2] = wl.side / 2.0 + r * np.sin(a)
    side = float(wl.side)
    if kind == "g":
        u = uniform(311, 2 * n)
        i = np.arange(n)
        x = (i % 18 + 0.5 + 0.2 * (u[0::2] - 0.5)) * 3.0 * ELL
        y = (i // 18 + 0.5 + 0.2 * (u[1::2] - 0.5)) * 3.0 * ELL
        side = 18 * 3.0 * ELL
    return f32(x), f32(y), f32(obs), hyper, side


def queries(case, side, B):
    small = CASES[case][0] < 4000
    offs = (-4, -2, 0, 2, 4, 6, 8, 10, 12, 40) if small else (-2, 5)
    py = side / 2.0 + 0.25 * ELL * (np.arange(16) - 7.5)
    bx, by = [], []
    if CASES[case][1] == "g":
        # Degenerate blocks alone, every l / 10 across the distance at which the
        # nearest lattice column (1.5 l inside the edge) leaves the plan: a lone
        # point's gain is c = sf2 / sqrt(sf2 + noise), and c exp(-r^2 / 2 l^2) =
        # tau2 at r = l sqrt(2 ln(c / tau2)); the increments before the drop and
        # the other columns move that by a few tenths of l.
        r = np.sqrt(2.0 * np.log(SF2 / np.sqrt(SF2 + 0.1) / PM.tau2(B, SF2)))
        offs = ()
        for d in r - 1.5 + 0.1 * np.arange(-8, 3):
            bx.append(np.full(128, side + d * ELL))
            by.append(np.full(128, side / 2.0 + 0.3 * ELL))
    for off in offs:
        px = side + off * ELL + 0.25 * ELL * np.arange(8)
        X, Y = np.meshgrid(px, py, indexing="ij")
        bx.append(X.reshape(-1))
        by.append(Y.reshape(-1))
    if offs:
        bx.append(np.full(128, side + 3.0 * ELL))      # the degenerate block
        by.append(np.full(128, side / 2.0 + 0.3 * ELL))
    far = (5.0 if small else 7.0) * ELL                 # the partial last block: 5 x 10
    if not offs:
        far = -6.0 * ELL                                # (g: inside the lattice, the only block with near tiles)
    X, Y = np.meshgrid(side + far + 0.25 * ELL * np.arange(5), side / 2.0 + 0.25 * ELL * np.arange(10), indexing="ij")
    bx.append(X.reshape(-1))
    by.append(Y.reshape(-1))
    qx, qy = f32(np.concatenate(bx)), f32(np.concatenate(by))
    assert qx.size % 128 == 50 and qx.size <= (1536 if small else 512)
    return qx, qy


def debug_plan(gm, qx, qy):
    """sbo_debug_plan as (nI, nQ, items [nI, nQ, 2] = (thr, count), records [kept, 4] = (I, qb, t, level))."""
    lib = N.lib()
    n = ctypes.c_int64(0)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, None, 0, ctypes.byref(n)))
    buf = np.empty(n.value, np.int32)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, buf.ctypes.data, buf.size,
                                    ctypes.byref(n)))
    nI, nQ, kept = int(buf[0]), int(buf[1]), int(buf[2])
    items = buf[4:4 + 2 * nI * nQ].reshape(nI, nQ, 2).copy()
    rec = buf[4 + 2 * nI * nQ:].reshape(kept, 4).copy()
    assert int(items[:, :, 1].sum()) == kept
    return nI, nQ, items, rec


def operand(gm):
    n = gm.n
    A = np.zeros((n, n), np.float32)
    gm.ctx.check(N.lib().sbo_get_inverse(gm.ctx.handle, A.ctypes.data))
    return np.tril(A)


def stream_state(gm, qx, qy, profile=False):
    """The kept f64 (mu, var) of a first sbo_tick_stream, and with `profile` its tiles_by_level."""
    lib = N.lib()
    gm.stream_reset()
    if profile:
        lib.sbo_profile(gm.ctx.handle, 1)
    gm.tick_stream(qx, qy, 2.0, 0.0)
    lv = (ctypes.c_int64 * 3)()
    if profile:
        mf = ctypes.c_double()
        gm.ctx.check(lib.sbo_profile_mfma(gm.ctx.handle, ctypes.byref(mf), lv))
        lib.sbo_profile(gm.ctx.handle, 0)
    assert gm.stream_info()["path"] == 0
    mu, var = gm.stream_state(qx.size)
    gm.stream_reset()
    return mu, var, list(lv)


OPTIONS = {N.SBO_OPT_PRECISION: (0, -1), N.SBO_OPT_QUERY_ORDER: (0, 1), N.SBO_OPT_KERNEL_VARIANT: (3, 3),
           N.SBO_OPT_TILE_SKIP: (-1, -1), N.SBO_OPT_SKIP_BUDGET: (20, 20), N.SBO_OPT_RESORT: (25, 25)}


class Lab:
    """One context for every case; each (case, B) is fitted, planned and put
    through the model once, and the tests share the result."""

    def __init__(self):
        self.ctx = Context(0)
        self.models = {}
        self.results = {}

    def configure(self, gm, B, resort, variant):
        for o, (v, _) in OPTIONS.items():
            gm.set_option(o, v)
        gm.set_option(N.SBO_OPT_SKIP_BUDGET, B)      # takes effect at the next fit / append
        gm.set_option(N.SBO_OPT_RESORT, resort)
        gm.set_option(N.SBO_OPT_KERNEL_VARIANT, variant)

    def restore(self, gm):
        for o, (_, d) in OPTIONS.items():
            gm.set_option(o, d)

    def run(self, case, B):
        if (case, B) in self.results:
            return self.results[(case, B)]
        n0, kind, add, resort, variant = CASES[case]
        x, y, obs, hyper, side = training(case)
        qx, qy = queries(case, side, B)
        gm = TerrainMapper(0, hyper, ctx=self.ctx)
        tgt = None
        try:
            self.configure(gm, B, resort, variant)
            gm.fit(x[:n0], y[:n0], obs[:n0])
            if add:
                gm.append(x[n0:], y[n0:], obs[n0:])
            assert gm.n == n0 + add
            _, alpha = gm.factor()
            order = gm.order()
            if add:   # the batch stays behind the fitted points unless the append re-sorted
                assert (sorted(order[n0:]) == list(range(n0, n0 + add))) == (resort == 0)
            tgt = gm
            if kind == "f":
                tgt = TerrainMapper(0, hyper)
                self.configure(tgt, B, resort, variant)
                tgt.import_state(gm.export_state())
            A = operand(tgt)
            key = case
            md = self.models.get(key)
            if md is None or not (np.array_equal(md[0], A) and np.array_equal(md[1], alpha) and np.array_equal(md[3], qx)):
                md = (A, alpha, PM.PlanModel(A, alpha, x[order], y[order], ELL, SF2, qx, qy), qx)
                self.models[key] = md
            model = md[2]
            nI, nQ, items, rec = debug_plan(tgt, qx, qy)
            res = PM.check(model, rec, nI, nQ, B)
            res.update(model=model, rec=rec, items=items, nI=nI, nQ=nQ, qx=qx, qy=qy,
                       levels=[int((rec[:, 3] == l).sum()) for l in range(3)],
                       dropped=int((PM.plan_levels(rec, nI, nQ)[:, :, :(model.n + 63) // 64] == PM.DROPPED).sum()))
            if B == 10:
                mu_p, var_p, lv = stream_state(tgt, qx, qy, profile=True)
                tgt.set_option(N.SBO_OPT_TILE_SKIP, 0)
                mu_d, var_d, _ = stream_state(tgt, qx, qy)
                tgt.set_option(N.SBO_OPT_TILE_SKIP, -1)
                res.update(mu_p=mu_p, var_p=var_p, mu_d=mu_d, var_d=var_d, swept=lv)
            if case == "a300" and B == 20:
                lib, nb = N.lib(), ctypes.c_int64(0)
                gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, None, 0, ctypes.byref(nb)))
                x3 = np.empty(nb.value, np.uint8)
                gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, x3.ctypes.data, x3.size, ctypes.byref(nb)))
                res["x3"] = x3
        except RuntimeError as ex:
            # a device error leaves the context unusable: end the module, run nothing more on it
            if "hip" in str(ex).lower() or "illegal" in str(ex).lower():
                pytest.exit(f"device error in {case} B={B}: {ex}", returncode=3)
            raise
        finally:
            self.restore(gm)
            if tgt is not None and tgt is not gm:
                tgt.close()
        print(f"plan_budget: {case} B={B} n={model.n} m={model.m} nI={nI} nQ={nQ} "
              f"ratio |dV|/tau2 {res['V'][0]:.4f} (q {res['V'][1]}) dvar/budget {res['var'][0]:.4f} (q {res['var'][1]}) "
              f"dmu/budget {res['mu'][0]:.4f} (q {res['mu'][1]}) tiles six/three/one {res['levels']} "
              f"dropped {res['dropped']} mean lost {int(res['effect']['mean_lost'].sum())}")
        self.results[(case, B)] = res
        return res

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def lab():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lb = Lab()
    yield lb
    lb.close()


def test_model_planes_are_the_staged_operand(lab):
    """The model's three bf16 planes of A against sbo_debug_x3_operand, bit
    for bit, at the byte addresses include/sbo.h documents (n = 300: twelve
    packed tiles; padding rows and columns are zero)."""
    r = lab.run("a300", 20)
    md, x3 = r["model"], r["x3"].view(np.uint16)
    nI = md.nI
    tiles = 2 * nI * (nI + 1)
    assert x3.size * 2 == tiles * 98304
    R, rb, h, g, rr, j = np.meshgrid(np.arange(2), np.arange(8), np.arange(2), np.arange(4), np.arange(16),
                                     np.arange(8), indexing="ij")
    row, col = (16 * (8 * R + rb) + rr).ravel(), (32 * h + 8 * g + j).ravel()
    byte = (R * 49152 + (2 * rb + h) * 1024 + (16 * g + rr) * 16 + 2 * j).ravel()
    n = md.n
    seen = 0
    for I in range(nI):
        for t in range(4 * (I + 1)):
            T = 2 * I * (I + 1) + t
            rw, cl = 256 * I + row, 64 * t + col
            ok = (rw < n) & (cl < n)
            for p in range(3):
                want = np.zeros(row.size, np.uint16)
                want[ok] = PM.bf16_bits(md.a[p][rw[ok], cl[ok]])
                have = x3[(T * 98304 + p * 16384 + byte) // 2]
                # (+0 and -0 pieces are the same value: compare them as +0)
                want[want == 0x8000] = 0
                have = np.where(have == 0x8000, 0, have)
                assert np.array_equal(want, have), (I, t, p, int(np.sum(want != have)))
                seen += int(np.count_nonzero(want))
    assert seen > 3 * 300 * 300 // 4


@pytest.mark.parametrize("B", BUDGETS)
@pytest.mark.parametrize("case", list(CASES))
def test_budget_holds_exactly(lab, case, B):
    """Every case, every B: |dV(q)|_2 <= tau2, |dvar(q)| <= 2^-B sf2 and
    |dmu(q)| <= 2^-B sqrt(sf2) for every query, in the f64 model of the
    device's plan -- no allowance but the model's own rounding.

    Measured on an MI355X (profiles/plan_budget.log): |dV| / tau2 0.08 to 0.30
    on (a) - (f) and 0.56 to 0.93 on (g); dvar at most 0.027 ((g): 0.049) and
    dmu at most 0.003 of their budgets."""
    r = lab.run(case, B)
    for k in ("V", "var", "mu"):
        assert r[k][0] <= 1.0 + RTOL, (case, B, k, r[k])


@pytest.mark.parametrize("B", [b for b in BUDGETS if b <= 20])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_is_not_vacuous(lab, case, B):
    """For B <= 20 the records hold tiles at levels 1 and 2 (variant 22 runs
    every kept tile at six products: drops only; the lattice case is held to
    level 2 alone, see LEVELS), a near tile is absent (a
    pair whose K* is not all zero in f32 and whose omission moves V), and the
    last row block lost a tile to the mean's own cutoff in some block."""
    r = lab.run(case, B)
    e, md = r["effect"], r["model"]
    if LEVELS[case] == "all":
        assert r["levels"][1] > 0 and r["levels"][2] > 0, r["levels"]
    elif LEVELS[case] == "far":
        assert r["levels"][2] > 0, r["levels"]
    else:
        assert r["levels"][1] == 0 and r["levels"][2] == 0 and r["levels"][0] > 0
    lv = PM.plan_levels(r["rec"], r["nI"], r["nQ"])
    near_absent = 0
    for qb in range(r["nQ"]):
        kq = md.k32[:, qb * 128:(qb + 1) * 128].max(1)
        for t in range((md.n + 63) // 64):
            if kq[t * 64:(t + 1) * 64].max() > 0 and np.any(lv[t // 4:, qb, t] == PM.DROPPED):
                near_absent += 1
    assert near_absent > 0
    assert np.sqrt(e["dV2"].max()) > 0
    assert e["mean_lost"].max() >= 1 and np.abs(e["dmu"]).max() > 0


def _kmax(md, nQ):
    """[k-tile, query block] largest K* entry."""
    nt = (md.n + 63) // 64
    out = np.zeros((nt, nQ))
    for qb in range(nQ):
        kq = md.k32[:, qb * 128:(qb + 1) * 128].max(1)
        for t in range(nt):
            out[t, qb] = kq[t * 64:(t + 1) * 64].max()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_checker_fails_a_doctored_plan(lab, case):
    """The device's plan at B = 20 with each non-empty item's nearest kept
    tile (the largest K* entry) removed, and with every kept tile one level
    lower (a level-2 tile dropped): the checker reports a ratio above 1 for
    both, in every case."""
    r = lab.run(case, 20)
    md, rec, nI, nQ = r["model"], r["rec"], r["nI"], r["nQ"]
    km = _kmax(md, nQ)
    keep = np.ones(rec.shape[0], bool)
    for I in range(nI):
        for qb in range(nQ):
            idx = np.flatnonzero((rec[:, 0] == I) & (rec[:, 1] == qb) & (rec[:, 2] < km.shape[0]))
            if idx.size:
                keep[idx[np.argmax(km[rec[idx, 2], qb])]] = False
    worst = {}
    lowered = rec.copy()
    lowered[:, 3] += 1
    for name, doc in (("nearest removed", rec[keep]), ("one level lower", lowered[lowered[:, 3] <= 2])):
        c = PM.check(md, doc, nI, nQ, 20)
        worst[name] = max(c[k][0] for k in ("V", "var", "mu"))
        print(f"plan_budget: {case} B=20 doctored ({name}): |dV|/tau2 {c['V'][0]:.3g} dvar {c['var'][0]:.3g} "
              f"dmu {c['mu'][0]:.3g}")
    assert all(w > 1.0 for w in worst.values()), worst


@pytest.mark.parametrize("case", list(CASES))
def test_sweep_executes_the_plan(lab, case):
    """B = 10: the kept f64 sigma^2 and mu of a first sbo_tick_stream under
    the plan and under SBO_OPT_TILE_SKIP 0 differ by the model's dvar and dmu,
    within twice the sweep's own f32 accumulation noise -- measured per case
    as max_q |device dense - model all-six| (the device against the f64
    reference), once for each of the two device runs.  The tick's
    tiles_by_level are the records' level counts.

    Measured on an MI355X (profiles/plan_budget.log), sigma^2: noise 1.2e-6
    (a1100, b1100, e320, a4100) to 1.5e-6 (a300, b300, d320, f300), 2.7e-6
    (c300) and 3.2e-6 (c1100); device minus model 2.4e-7 (a1100_v22) to
    2.1e-6 (a1100, against 2 x 1.21e-6); the model's largest dvar 5.5e-6
    (a4100) to 6.0e-5 (d320).  mu: noise 1e-7 (b) to 4.8e-6, 1.0e-4 and
    3.2e-4 on c300 / c1100 (|sf2 alpha|_1 is large under noise 0.01); device
    minus model 4e-9 to 1.2e-7."""
    r = lab.run(case, 10)
    md, e = r["model"], r["effect"]
    mu6, var6 = md.dense_posterior(M0)
    noise_var = np.abs(r["var_d"] - var6).max()
    noise_mu = np.abs(r["mu_d"] - mu6).max()
    err_var = np.abs((r["var_p"] - r["var_d"]) - e["dvar"]).max()
    err_mu = np.abs((r["mu_d"] - r["mu_p"]) - e["dmu"]).max()
    print(f"plan_budget: {case} B=10 dense-sweep noise var {noise_var:.3g} mu {noise_mu:.3g}; device minus model "
          f"dvar {err_var:.3g} dmu {err_mu:.3g}; largest model dvar {np.abs(e['dvar']).max():.3g} "
          f"dmu {np.abs(e['dmu']).max():.3g}; swept six/three/one {r['swept']}")
    assert r["swept"] == r["levels"]
    assert noise_var < 1e-5 * SF2                                           # the reference is the sweep's (the contract)
    assert err_var <= 2.0 * noise_var and err_mu <= 2.0 * noise_mu
    assert np.abs(e["dvar"]).max() > 2.0 * noise_var                        # the plan's effect stands above it


@pytest.mark.parametrize("B", [20, 27, 34])
def test_precise_sweep_drops_within_budget(lab, B):
    """SBO_OPT_PRECISION 1, n = 700 on the lpsc box, 40 x 30 queries: the
    precise sweep's partials are f64, so the device result itself is held
    pointwise -- the kept sigma^2 and mu of the skipping tick against the
    dense tick's within 2^-B (smallest probe variance) and 2^-B sqrt(sf2),
    plus a relative 1e-9 for the f64 summation order."""
    wl = synthetic_box(700, 40, 30, seed=700)
    gm = TerrainMapper(0, wl.hyper, ctx=lab.ctx)
    # On the box's own grid nothing is negligible at these budgets (the box is
    # 2.5 x 6.25 l): the 40 x 30 raster runs from the box's middle to 8 l above
    # its top edge, rows of 40 across x, so the far blocks lose tiles.
    ell = wl.hyper.length_scale
    gy, gx = np.meshgrid(np.linspace(1.25, 2.5 + 8.0 * ell, 30), np.linspace(0.0, 1.0, 40), indexing="ij")
    qx, qy = f32(gx.reshape(-1)), f32(gy.reshape(-1))
    try:
        gm.set_option(N.SBO_OPT_PRECISION, 1)
        gm.set_option(N.SBO_OPT_QUERY_ORDER, 0)
        gm.set_option(N.SBO_OPT_SKIP_BUDGET, B)
        gm.fit(wl.x, wl.y, wl.obs)
        precise, _, vmin, _ = gm.precision()
        assert precise and 0.0 < vmin <= wl.hyper.sf2
        nI, nQ, items, rec = debug_plan(gm, qx, qy)
        # (k-tiles of padding columns alone do not count)
        dropped = int((PM.plan_levels(rec, nI, nQ)[:, :, :(700 + 63) // 64] == PM.DROPPED).sum())
        mu_p, var_p, _ = stream_state(gm, qx, qy)
        gm.set_option(N.SBO_OPT_TILE_SKIP, 0)
        mu_d, var_d, _ = stream_state(gm, qx, qy)
    finally:
        gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
        gm.set_option(N.SBO_OPT_SKIP_BUDGET, 20)
        gm.set_option(N.SBO_OPT_QUERY_ORDER, 1)
        gm.set_option(N.SBO_OPT_PRECISION, -1)
    dvar = np.abs(var_p - var_d)
    dmu = np.abs(mu_p - mu_d)
    print(f"plan_budget: precise n=700 B={B} probe var min {vmin:.3g} dropped {dropped} kept {rec.shape[0]} "
          f"dvar/budget {dvar.max() / (2.0 ** -B * vmin):.3g} dmu/budget {dmu.max() / (2.0 ** -B * np.sqrt(wl.hyper.sf2)):.3g}")
    if B == 20:
        assert dropped > 0
    assert np.all(dvar <= 2.0 ** -B * vmin + 1e-9 * np.abs(var_d))
    assert np.all(dmu <= 2.0 ** -B * np.sqrt(wl.hyper.sf2) + 1e-9 * np.abs(mu_d))
