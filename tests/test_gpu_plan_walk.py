"""The persistent item walk of the predictive sweeps (csrc/plan_walk.hpp) over
a plan that makes one workgroup reuse both slots of each LDS window pair.

One fit of n = 1100 points (five row blocks, the last ragged) and a 59 x 57
query grid (27 query blocks, the last ragged) under the dense plan
(SBO_OPT_TILE_SKIP 0): 135 items and 1620 tile-list entries.  With
SBO_OPT_SWEEP_GROUPS 1 a single workgroup walks all of them, across two
descriptor-window (64 items) and three list-window (512 entries) boundaries.

For the fast variants 0 and 1 and the precise kernels 0, 1, 3 and 4: predict is
bitwise the same for 0 (one workgroup per CU), 1 and 7 sweep workgroups, as
sbo.h promises of SBO_OPT_SWEEP_GROUPS, and agrees with the fp64 oracle given
the device's factor within test_gpu_parity.py's tolerances for that kernel."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import TerrainMapper, synthetic  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402

from test_gpu_parity import PRECISE_TOL, REL_TOL, nrel, oracle_given_factor, oracle_given_factor64  # noqa: E402
from test_gpu_plan_front import debug_plan  # noqa: E402

GROUPS = (0, 1, 7)
# (SBO_OPT_PRECISION, SBO_OPT_KERNEL_VARIANT or SBO_OPT_PRECISE_KERNEL)
KERNELS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 3), (1, 4)]


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    wl = synthetic(1100, 59, 57, seed=1100)
    gm = TerrainMapper(0, wl.hyper)
    gm.set_option(N.SBO_OPT_PRECISION, 1)      # (the fit keeps its f64 inverse for the precise kernels)
    gm.fit(wl.x, wl.y, wl.obs)
    gm.set_option(N.SBO_OPT_PRECISION, -1)
    oracle = {0: oracle_given_factor(gm, wl), 1: oracle_given_factor64(gm, wl)}
    yield gm, wl, oracle
    gm.close()


def test_plan_crosses_both_window_kinds(rig):
    gm, wl, _ = rig
    gm.set_option(N.SBO_OPT_TILE_SKIP, 0)
    gm.set_option(N.SBO_OPT_KERNEL_VARIANT, 0)
    try:
        nI, nQ, items, rec = debug_plan(gm, wl.qx, wl.qy)
    finally:
        gm.set_option(N.SBO_OPT_KERNEL_VARIANT, 3)
        gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
    print(f"plan: {nI} row blocks x {nQ} query blocks, {int((items[:, :, 1] > 0).sum())} items, {rec.shape[0]} entries")
    assert (nI, nQ) == (5, 27)
    assert int((items[:, :, 1] > 0).sum()) == 135 and rec.shape[0] == 1620


@pytest.mark.parametrize("precision,kernel", KERNELS, ids=[f"p{p}k{k}" for p, k in KERNELS])
def test_walk_is_partition_independent_and_matches_oracle(rig, precision, kernel):
    gm, wl, oracle = rig
    kernel_opt = N.SBO_OPT_PRECISE_KERNEL if precision else N.SBO_OPT_KERNEL_VARIANT
    res = {}
    try:
        gm.set_option(N.SBO_OPT_TILE_SKIP, 0)
        gm.set_option(kernel_opt, kernel)
        gm.set_option(N.SBO_OPT_PRECISION, precision)
        assert gm.precision()[0] == bool(precision)
        for groups in GROUPS:
            gm.set_option(N.SBO_OPT_SWEEP_GROUPS, groups)
            res[groups] = gm.predict(wl.qx, wl.qy)
    finally:
        gm.set_option(N.SBO_OPT_SWEEP_GROUPS, 0)
        gm.set_option(N.SBO_OPT_PRECISION, -1)
        gm.set_option(N.SBO_OPT_PRECISE_KERNEL, 3)
        gm.set_option(N.SBO_OPT_KERNEL_VARIANT, 3)
        gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
    mu, sd = res[0]
    for groups in GROUPS[1:]:
        assert np.array_equal(res[groups][0], mu) and np.array_equal(res[groups][1], sd), groups
    omu, ovar = oracle[precision]
    emu, evar = nrel(mu, omu), nrel(sd.astype(np.float64) ** 2, ovar)
    tmu, tvar = PRECISE_TOL[kernel] if precision else (REL_TOL, REL_TOL)
    print(f"precision {precision} kernel {kernel}: mu {emu:.2e} var {evar:.2e} (bounds {tmu:.0e}, {tvar:.0e})")
    assert emu < tmu and evar < tvar
