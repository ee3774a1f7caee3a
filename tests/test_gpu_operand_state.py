"""Which parts of a context's model are valid after each call (sbo_debug_state),
and that the two derived operands -- the split bf16 operand and the precise
one -- hold the same bytes whichever way they were brought up to date: eagerly
beside a fit or an append, lazily at a tick, in one piece or row block by row
block, before or after a change of layout.

N = 300 is two row blocks of 256 rows, the second ragged; one more point stays
inside it (row block 1 repacked), 250 more open a third.  SBO_OPT_RESORT 0
keeps every append a block update.  Contexts that must not derive an operand
at the fit also set SBO_OPT_PRECISION 0: the automatic probe sweeps with both.
"""
import ctypes

import numpy as np
import pytest

from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import Hyper, more_points

FIELDS = ("n", "npad", "fitted", "has_factor", "inv_rows", "z_rows", "probe_n", "split", "split_layout", "precise",
          "precise_layout", "in_flight", "fit_epoch")
N0 = 300
WL = synthetic(N0, 20, 15, seed=11)
MORE = more_points(WL, 251)
ROW_HALF = 2          # the product sweep's split-operand layout (sbo::x3_layout)
INT8 = 1              # SBO_OPT_PRECISE_KERNEL 1 and 3 share it; 0 (f64 tiles) is layout 0


def f32(a):
    return np.ascontiguousarray(a, np.float32)


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def state(gm):
    out = (ctypes.c_int64 * len(FIELDS))()
    gm.ctx.check(N.lib().sbo_debug_state(gm.ctx.handle, out, len(FIELDS)))
    s = dict(zip(FIELDS, (int(v) for v in out)))
    print(s)
    return s


def expect(gm, **want):
    s = state(gm)
    got = {k: s[k] for k in want}
    assert got == want
    return s


def mapper(*options, hyper=None):
    gm = TerrainMapper(0, hyper or WL.hyper)
    gm.set_option(N.SBO_OPT_RESORT, 0)
    for k, v in options:
        gm.set_option(k, v)
    return gm


def fit(gm):
    gm.fit(f32(WL.x), f32(WL.y), f32(WL.obs))


def append(gm, lo, hi):
    gm.append(*(f32(a[lo:hi]) for a in MORE))


def predict(gm):
    mu, sd = gm.predict(f32(WL.qx), f32(WL.qy))
    return np.asarray(mu).copy(), np.asarray(sd).copy()


def same(a, b):
    return all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(a, b))


def x3_bytes(gm):
    lib, nb = N.lib(), ctypes.c_int64(0)
    gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, None, 0, ctypes.byref(nb)))
    buf = np.empty(nb.value, np.uint8)
    gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, buf.ctypes.data, buf.size, ctypes.byref(nb)))
    return buf


def twin_predictions(kernel):
    """fit 300, append 1, append 250 with every option set before the fit."""
    gm = mapper((N.SBO_OPT_PRECISION, 1), (N.SBO_OPT_PRECISE_KERNEL, kernel))
    try:
        fit(gm)
        append(gm, 0, 1)
        append(gm, 1, 251)
        return predict(gm)
    finally:
        gm.close()


@pytest.mark.gpu
def test_eager_context_and_import(dev):
    gm, imp = mapper((N.SBO_OPT_PRECISION, 0)), None
    try:
        expect(gm, n=0, fitted=0, split=0, split_layout=-1, precise=0, in_flight=0)
        fit(gm)
        expect(gm, n=N0, npad=512, fitted=1, has_factor=1, inv_rows=N0, z_rows=N0, probe_n=0, split=-1,
               split_layout=ROW_HALF, precise=0)
        append(gm, 0, 1)
        expect(gm, n=N0 + 1, inv_rows=N0 + 1, z_rows=N0 + 1, split=-1, split_layout=ROW_HALF, precise=0)
        gm.set_option(N.SBO_OPT_PRECISION, 1)                 # the probe's reference sweep derives the operand
        expect(gm, precise=-1, precise_layout=INT8, in_flight=0, probe_n=N0 + 1)
        append(gm, 1, 251)                                    # both eager; the precise pack outlives the call
        expect(gm, n=N0 + 251, npad=768, inv_rows=N0 + 251, z_rows=N0 + 251, split=-1, split_layout=ROW_HALF,
               precise=-1, precise_layout=INT8, in_flight=1, probe_n=N0 + 251)
        got = {3: predict(gm)}
        gm.set_option(N.SBO_OPT_PRECISE_KERNEL, 0)            # another layout: all of it
        expect(gm, precise=0)
        got[0] = predict(gm)
        expect(gm, precise=-1, precise_layout=0, in_flight=0)
        gm.set_option(N.SBO_OPT_PRECISE_KERNEL, 1)
        expect(gm, precise=0)
        got[1] = predict(gm)
        expect(gm, precise=-1, precise_layout=INT8)
        gm.set_option(N.SBO_OPT_PRECISE_KERNEL, 3)            # the same layout
        expect(gm, precise=-1, precise_layout=INT8)
        again = predict(gm)
        for k in (3, 0, 1):
            assert same(got[k], twin_predictions(k)), k
        assert same(again, got[3])

        # an imported state ticks with the fast sweep: compare under SBO_OPT_PRECISION 0
        gm.set_option(N.SBO_OPT_PRECISION, 0)
        fast = predict(gm)
        epoch = expect(gm, split=-1, split_layout=ROW_HALF)["fit_epoch"]
        blob = gm.export_state()
        imp = mapper()
        imp.import_state(blob)
        expect(imp, n=N0 + 251, npad=768, fitted=1, has_factor=0, inv_rows=0, split=0, split_layout=-1)
        assert same(predict(imp), fast)
        expect(imp, split=-1, split_layout=ROW_HALF)
        assert state(gm)["fit_epoch"] == epoch                # (an export is no event of the exporter's model)
    finally:
        gm.close()
        if imp is not None:
            imp.close()


@pytest.mark.gpu
def test_lazy_context_derives_from_the_first_stale_row_block(dev):
    """SBO_OPT_CHOLESKY 0 from the start: no second stream, so the split operand
    is derived at the tick.  One context ticks between the fit and two appends
    (its operand is then stale from row block 1), its twin does not (stale
    from 0): the same bytes."""
    lazy = ((N.SBO_OPT_CHOLESKY, 0), (N.SBO_OPT_PRECISION, 0))
    gm, tw = mapper(*lazy), mapper(*lazy)
    try:
        fit(gm)
        expect(gm, split=0, split_layout=-1, inv_rows=N0)
        predict(gm)
        expect(gm, split=-1, split_layout=ROW_HALF)
        append(gm, 0, 1)
        expect(gm, split=1)
        append(gm, 1, 2)
        expect(gm, split=1, n=N0 + 2)
        got = predict(gm)
        expect(gm, split=-1, split_layout=ROW_HALF)

        fit(tw)
        append(tw, 0, 1)
        append(tw, 1, 2)
        expect(tw, split=0, split_layout=-1, n=N0 + 2)
        assert same(predict(tw), got)
        expect(tw, split=-1, split_layout=ROW_HALF)
        assert np.array_equal(x3_bytes(gm), x3_bytes(tw))
    finally:
        gm.close()
        tw.close()


@pytest.mark.gpu
def test_f32_inverse_refreshes_in_full(dev):
    gm = mapper((N.SBO_OPT_INVERSE_BITS, 32))
    try:
        fit(gm)
        expect(gm, n=N0, fitted=1, has_factor=1, inv_rows=0, split=0, precise=0)
        append(gm, 0, 1)
        expect(gm, n=N0 + 1, fitted=1, has_factor=1, inv_rows=0, split=0, precise=0)
    finally:
        gm.close()


# the lattice of tests/test_gpu_fit_commit.py: 300 points 1.25 length scales
# apart factor cleanly with zero noise; with point 1 moved onto point 0 the
# second pivot is exactly 0
HYPER0 = Hyper(noise_level=0.0)


def lattice(duplicate=False):
    gy, gx = np.meshgrid(np.arange(15) * 0.5, np.arange(20) * 0.5, indexing="ij")
    x, y = f32(gx.reshape(-1)), f32(gy.reshape(-1))
    obs = f32(np.sin(1.3 * x) + np.cos(0.9 * y))
    if duplicate:
        x[1], y[1] = x[0], y[0]
    return x, y, obs


@pytest.mark.gpu
def test_failed_fit_unfits_everything_derived(dev):
    gm, fresh = mapper(hyper=HYPER0), mapper(hyper=HYPER0)
    try:
        gm.fit(*lattice())
        before = expect(gm, fitted=1, inv_rows=N0, split=-1)
        with pytest.raises(N.NotSPDError):
            gm.fit(*lattice(duplicate=True))
        # (the factorization fails before the refresh says what changed: it is
        # unfit() that marks both operands stale; before it existed they were
        # left as the last fit had them, which the next fit's full refresh undid)
        after = expect(gm, fitted=0, inv_rows=0, split=0, precise=0)
        assert after["fit_epoch"] > before["fit_epoch"]
        gm.fit(*lattice())
        fresh.fit(*lattice())
        a, b = state(gm), state(fresh)
        assert a["fit_epoch"] > b["fit_epoch"]
        a.pop("fit_epoch"), b.pop("fit_epoch")
        assert a == b
    finally:
        gm.close()
        fresh.close()
