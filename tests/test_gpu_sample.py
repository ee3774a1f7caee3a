"""sbo_sample: posterior sample paths on the kept grid, their Thompson keys and
counts (include/sbo.h, csrc/sample.hip) through the C ABI on cuda:0, against
tests/sample_model.py.

The rig and the three fits are test_gpu_whatif's: a 37 x 29 raster grid
(m = 1073, no multiple of 128); n = 333 reached as fit(300) + append(33) (a
k-tile tail, an unsorted appended tail), n = 1061 on a 24 l x 24 l box (the
cutoff bites), n = 700 on the lpsc box with the precise sweep.  S = 1, 17 and
150 samples (150 > 128: a second pass of the sample blocking, and a partial
last block); F = 1, 37 and 256 features (37 is no multiple of 4; 1 is a single
step).

The model works from the device factor (factor(), order()), the kept mean
(stream_state(m)) and the device's own standard normals (sample_draws), which
test_draws_follow_the_specification holds to terrain.normal on their own: the
device's log / cospi and numpy's differ in the last places.  So what is
compared is the feature walk, the weights, the contraction and the epilogue;
every comparison is normwise (max |d| / max |ref|) over all entries, and runs
the dense call (SBO_OPT_TILE_SKIP 0).  What the cutoff does is held to its own
rigorous bound (test_cutoff).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import TerrainMapper  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from tests import sample_model as SM  # noqa: E402
from tests.test_gpu_stream_tick import BETA, Rig, nrel, same  # noqa: E402
from tests.test_gpu_whatif import SHAPES, Case, status_of  # noqa: E402

# 16 x the worst normwise error of `paths` measured over the 27 cases below
# (3.33e-14: 150 samples at 256 features on the lpsc box; 6.7e-15 .. 2.7e-14
# elsewhere; |w|_1 1.6e-15 and kernel_err 5.6e-17 at worst): the
# paths are f64, the margin covers run-to-run differences in rocBLAS blocking.
# It must itself stay below 1e-9.
WORST = 3.33e-14
TOL = 16 * WORST
SS = (1, 17, 150)
FS = (1, 37, 256)
SEED = 7
GRID_W, GRID_H = 37, 29


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class SampleCase(Case):
    """test_gpu_whatif's Case with the sampler's calls and the model's results (computed once, never changed)."""

    def __init__(self, dev, **kw):
        super().__init__(dev, **kw)
        self.order = self.rig.gm.order()
        self._draws, self._dense, self._mdl = {}, {}, {}

    def call(self, S, F, device=False, **kw):
        r = self.rig
        kw.setdefault("paths", True)
        out = r.gm.sample(S, SEED, BETA, r.f_min, features=F, device=r.dev if device else None, **kw)
        if device:
            torch.cuda.synchronize()
            out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
        return out

    def dense(self, S, F):
        if (S, F) not in self._dense:
            gm = self.rig.gm
            try:
                gm.set_option(N.SBO_OPT_TILE_SKIP, 0)
                self._dense[S, F] = self.call(S, F)
            finally:
                gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
        return self._dense[S, F]

    def draws(self, S, F):
        if (S, F) not in self._draws:
            self._draws[S, F] = self.rig.gm.sample_draws(S, SEED, features=F)
        return self._draws[S, F]

    def model(self, S, F):
        if (S, F) not in self._mdl:
            hy = self.rig.hyper
            self._mdl[S, F] = SM.sample(self.L, self.x, self.y, self.order, self.s, hy.length_scale, hy.sigma_f,
                                        self.rig.qx, self.rig.qy, self.mu, SEED, 0, S, F, given=self.draws(S, F))
        return self._mdl[S, F]


@pytest.fixture(scope="module")
def cases(dev):
    return {k: SampleCase(dev, **v) for k, v in SHAPES.items()}


def same_sample(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("scores", "idx", "count_above")) and \
        (a["paths"] is None or b["paths"] is None or np.array_equal(a["paths"], b["paths"]))


def own_keys(w, safe, f_min, index_offset=0):
    """The call's keys and counts are exactly those of its own paths."""
    scores, idx = SM.keys(w["paths"], safe, index_offset)
    assert np.array_equal(w["idx"], idx), (w["idx"], idx)
    assert np.array_equal(w["scores"], scores)
    assert np.array_equal(w["count_above"], (w["paths"] > f_min).sum(axis=1))


def test_draws_follow_the_specification(dev, cases):
    c = cases["appended333"]
    gm, n = c.rig.gm, c.rig.n
    worst = 0.0
    for first, S, F in ((0, 150, 37), (17, 5, 256), (1000000, 3, 1)):
        nu, ab, eps = gm.sample_draws(S, SEED, features=F, first=first)
        mnu, mab, meps = SM.draws(SEED, first, S, F, n)
        worst = max(worst, np.abs(nu - mnu).max(), np.abs(ab - mab).max(), np.abs(eps - meps).max())
    print(f"draws: max |device - terrain.normal| {worst:.2e}")
    assert worst <= 1e-13
    # eps goes with the caller's index of a training point, whatever the internal order
    r0 = Rig(dev, 333, options=((N.SBO_OPT_SPATIAL_ORDER, 0),))
    r0.fit(333)
    assert np.array_equal(r0.gm.order(), np.arange(333)) and not np.array_equal(c.order, np.arange(333))
    a, b = r0.gm.sample_draws(17, SEED, features=37), gm.sample_draws(17, SEED, features=37)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_accuracy_given_the_device_factor(cases, shape, S, F):
    c = cases[shape]
    w, mdl = c.dense(S, F), c.model(S, F)
    assert (w["samples"], w["first"], w["m"], w["n"], w["features"]) == (S, 0, c.rig.m, c.rig.n, F)
    assert w["cutoff_log2"] == 0 and w["err_path"] == 0.0 and w["tiles_kept"] == w["tiles_total"]
    err = nrel(w["paths"], mdl["paths"])
    # (against the prior part alone the error would hide behind mu: hold path - mu to the same absolute error)
    kerr = abs(w["kernel_err"] - mdl["kernel_err"])
    print(f"{shape} S {S} F {F}: paths {err:.2e} kernel_err {w['kernel_err']:.4f} (model {kerr:.1e}) "
          f"w_l1 {nrel(w['w_l1_max'], mdl['w_l1'].max()):.1e} ms {w['ms']:.3f}")
    assert TOL < 1e-9
    assert err <= TOL, err
    assert kerr <= 1e-12
    assert nrel(w["w_l1_max"], mdl["w_l1"].max()) <= TOL


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_keys_and_counts_are_those_of_the_calls_own_paths(cases, shape, S, F):
    c = cases[shape]
    own_keys(c.dense(S, F), c.h["safe"], c.rig.f_min)


def test_keys_against_the_model(cases):
    left_out = total = 0
    for shape, c in cases.items():
        for S in SS:
            for F in FS:
                w, mdl = c.dense(S, F), c.model(S, F)
                scores, idx = SM.keys(mdl["paths"], c.h["safe"])
                clear = SM.top_two_gap(mdl["paths"], c.h["safe"]) > 100.0 * TOL * np.abs(mdl["paths"]).max()
                left_out += int((~clear).sum())
                total += S
                assert np.array_equal(w["idx"][clear], idx[clear]), (shape, S, F)
                assert np.abs(w["scores"][clear] - scores[clear]).max() <= TOL * np.abs(mdl["paths"]).max()
        distinct = np.unique(c.dense(150, 256)["idx"]).size
        print(f"{shape}: the 150 keys at F 256 take {distinct} distinct indices")
        assert distinct >= 10
    print(f"keys: {left_out} of {total} samples inside the gap band")
    assert left_out <= 0.02 * total


def test_index_offset_and_an_empty_safe_set(cases):
    c = cases["box24l"]
    r = c.rig
    gm = r.gm
    off = c.call(17, 37, index_offset=5000)
    own_keys(off, c.h["safe"], r.f_min, 5000)
    assert np.all(off["idx"] >= 5000)
    # nothing is safe under a high f_min: idx -1, score 0, no query above it
    none = gm.sample(17, SEED, BETA, 1e9, features=37, index_offset=5000, paths=True)
    assert np.all(none["idx"] == -1) and np.all(none["scores"] == 0.0) and np.all(none["count_above"] == 0)
    # f_min = -inf: the unconstrained maximiser, every query counted
    free = gm.sample(17, SEED, BETA, -np.inf, features=37, paths=True)
    own_keys(free, np.ones(r.m, bool), -np.inf)
    assert np.array_equal(free["idx"], np.argmax(free["paths"], axis=1)) and np.all(free["count_above"] == r.m)
    assert np.array_equal(free["paths"], off["paths"])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cutoff(cases, shape):
    c, S, F = cases[shape], 17, 37
    gm = c.rig.gm
    auto, dense = c.call(S, F), c.dense(S, F)
    try:
        gm.set_option(N.SBO_OPT_TILE_SKIP, 160)
        l160 = c.call(S, F)
    finally:
        gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
    assert l160["cutoff_log2"] == 160 and same_sample(l160, dense)
    assert 16 <= auto["cutoff_log2"] <= 150
    bmean = gm.stream_info()["budget_mean"]
    assert (auto["cutoff_log2"], auto["err_path"]) == SM.cutoff([auto["w_l1_max"]], c.rig.hyper.sf2, bmean)
    d = np.abs(auto["paths"] - dense["paths"]).max()
    print(f"{shape}: auto L {auto['cutoff_log2']} tiles {auto['tiles_kept']}/{auto['tiles_total']} "
          f"|paths - dense| {d:.2e} err_path {auto['err_path']:.2e} w_l1_max {auto['w_l1_max']:.3g}")
    assert d <= auto["err_path"]
    own_keys(auto, c.h["safe"], c.rig.f_min)
    if shape == "box24l":
        assert auto["tiles_kept"] < auto["tiles_total"]


@pytest.mark.parametrize("shape", ["appended333", "lpsc700precise"])
def test_state_and_determinism(cases, shape):
    c, S, F = cases[shape], 150, 37
    r = c.rig
    a = c.call(S, F)
    # the kept state and the next streaming tick are bit for bit what they were
    mu, var = r.gm.stream_state(r.m)
    assert np.array_equal(mu, c.mu) and np.array_equal(var, c.var)
    assert same(r.tick(), c.tick)
    # two calls; host and device pointers; a call after sbo_trim
    assert same_sample(c.call(S, F), a)
    assert same_sample(c.call(S, F, device=True), a)
    r.gm.trim()
    assert same_sample(c.call(S, F), a)
    # a range of samples cut into two calls
    lo, hi = c.call(17, F), c.call(133, F, first=17)
    for k in ("scores", "idx", "count_above", "paths"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k]), k
    # without the paths the keys and counts are the same
    assert same_sample(c.call(S, F, paths=False), a)


@pytest.mark.parametrize("shape", ["appended333", "lpsc700precise"])
def test_statistics_on_the_device(cases, shape):
    """tests/test_sample_model.py's two conditions on seed 7, against the tick's own mu and sd."""
    c, S, F = cases[shape], 256, 1024
    w = c.call(S, F)
    mu, sd = c.h["mu"].astype(np.float64), c.h["sd"].astype(np.float64)
    dev_ = w["paths"] - mu[None, :]
    rms = float(np.sqrt(np.mean((dev_ / sd[None, :]) ** 2)))
    mean_err = float(np.abs(dev_.mean(axis=0)).max() / (sd.max() / np.sqrt(S)))
    print(f"{shape}: rms {rms:.3f} mean {mean_err:.2f} sd_max/sqrt(S) kernel_err {w['kernel_err']:.4f} ms {w['ms']:.3f}")
    assert 0.93 <= rms <= 1.07
    assert mean_err <= 4.0
    assert w["kernel_err"] <= 4.0 / np.sqrt(2.0 * F)


def test_shards_draw_the_same_global_paths(dev, cases):
    """Two further rigs with the same training data hold the grid's first 15 and last 14 rows: each draws
    the whole grid's paths on its rows, and the keys combine to the whole grid's."""
    c, S, F = cases["appended333"], 17, 37
    whole = c.dense(S, F)
    cut = (GRID_H - 14) * GRID_W
    scale = np.abs(whole["paths"]).max()
    keys, safe = [], []
    for a, b in ((0, cut), (cut, c.rig.m)):
        r = Rig(dev, 333, options=((N.SBO_OPT_TILE_SKIP, 0),))
        r.set_queries(c.rig.qx[a:b], c.rig.qy[a:b])
        r.fit(300)
        r.tick()
        r.append(33)
        h, _ = r.tick()
        part = r.gm.sample(S, SEED, BETA, r.f_min, features=F, index_offset=a, paths=True)
        kept_mu, _ = r.gm.stream_state(r.m)
        d = np.abs((part["paths"] - kept_mu[None, :]) - (whole["paths"][:, a:b] - c.mu[None, a:b])).max()
        print(f"rows {a}:{b}: |(paths - kept mean) - whole grid's| {d / scale:.2e}")
        assert d <= TOL * scale
        keys.append(part["keys"])
        safe.append(h["safe"])
    safe = np.concatenate(safe).astype(bool)
    # The combined key is the maximiser of the whole grid's path over the parts' safe sets: the whole grid's key
    # whenever that lies in a safe row of its part and no row is safe in a part only.  (The parts' ticks plan
    # other query blocks: their f32 mu agrees with the whole grid's to the tick's 1e-5 normwise contract, so a
    # maximiser is only decided where the top two safe values differ by more.)
    scores, idx = SM.keys(whole["paths"], safe)
    clear = SM.top_two_gap(whole["paths"], safe) > 1e-4 * scale
    print(f"safe sets equal: {np.array_equal(safe, c.h['safe'].astype(bool))}, decided samples {clear.sum()} of {S}")
    assert clear.sum() >= S // 2
    for j in np.flatnonzero(clear):
        got_score, got_idx = c.rig.gm.ctx.reduce_keys(np.stack([keys[0][j], keys[1][j]]))
        assert got_idx == idx[j] and abs(got_score - scores[j]) <= 1e-4 * scale, (j, got_idx, idx[j])
        if np.array_equal(safe, c.h["safe"].astype(bool)):
            assert got_idx == whole["idx"][j]


def test_status_codes(dev):
    E_STATE, E_INVAL = N.SBO_E_STATE, 1
    r = Rig(dev, 333)
    call = lambda gm=r.gm, S=3, F=8: gm.sample(S, SEED, BETA, r.f_min, features=F)  # noqa: E731
    r.fit(300)
    assert status_of(call) == E_STATE            # no kept posterior
    r.tick()
    assert call()["samples"] == 3
    r.append(33)
    assert status_of(call) == E_STATE            # an append without a following tick
    r.tick()
    assert call()["n"] == 333
    r.fit(300)
    assert status_of(call) == E_STATE            # another fit epoch
    r.tick()
    # samples 0 and 1025, features 0 and 4097, first out of range, a NULL keys
    for S, F in ((0, 8), (1025, 8), (3, 0), (3, 4097)):
        assert status_of(lambda: call(S=S, F=F)) == E_INVAL
    assert status_of(lambda: r.gm.sample(3, SEED, BETA, r.f_min, features=8, first=-1)) == E_INVAL
    assert status_of(lambda: r.gm.sample(3, SEED, BETA, r.f_min, features=8, first=(1 << 20) - 2)) == E_INVAL
    assert N.lib().sbo_sample(r.gm.ctx.handle, SEED, 0, 3, 8, BETA, r.f_min, 0, None, None, None, None, 0) == E_INVAL
    assert call(S=1024, F=1)["samples"] == 1024 and call(S=1, F=4096)["features"] == 4096
    # an imported state has no factor and no inverse
    g2 = TerrainMapper(0, r.hyper)
    g2.import_state(r.gm.export_state())
    g2.tick_stream(r.dqx, r.dqy, BETA, r.f_min)
    assert status_of(lambda: call(g2)) == E_STATE
    # an f32 inverse
    r32 = Rig(dev, 333, options=((N.SBO_OPT_INVERSE_BITS, 32),))
    r32.fit(333)
    r32.tick()
    assert status_of(lambda: call(r32.gm)) == E_STATE


def test_thompson_subgoal(cases):
    c = cases["box24l"]
    r = c.rig
    got = r.gm.thompson_subgoal(BETA, r.f_min, SEED, features=256)
    assert 0 <= got < r.m and c.h["safe"][got]
    assert got == int(r.gm.sample(1, SEED, BETA, r.f_min, features=256)["idx"][0])
    # other seeds look elsewhere
    assert len({r.gm.thompson_subgoal(BETA, r.f_min, s, features=256) for s in range(8)}) > 1
