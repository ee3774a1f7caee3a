"""The streaming tick's identity in numpy f64 (tests/stream_model.py) against
the fp64 oracle, and the new entry points' null-context behaviour (no device)."""
import ctypes

import numpy as np
import pytest

from tests import stream_model as SM
from oracle import oracle as O
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import uniform, normal, smooth_field

ELL, SF2, SN2, M0 = 0.4, 1.0, 0.1, 0.25


def box_case(n, x_range, y_range, seed):
    (x0, x1), (y0, y1) = x_range, y_range
    u = uniform(seed, 2 * n)
    x = (x0 + u[0::2] * (x1 - x0)).astype(np.float32)
    y = (y0 + u[1::2] * (y1 - y0)).astype(np.float32)
    obs = (smooth_field(x, y, max(x1 - x0, y1 - y0), ELL, seed) + np.sqrt(SN2) * normal(seed + 1, n)).astype(np.float32)
    gx = np.linspace(x0 - 0.3, x1 + 0.3, 23)
    gy = np.linspace(y0 - 0.3, y1 + 0.3, 19)
    QY, QX = np.meshgrid(gy, gx, indexing="ij")
    return x, y, obs, QX.reshape(-1).astype(np.float32), QY.reshape(-1).astype(np.float32)


@pytest.mark.parametrize("cuts,xr,yr", [((200, 207, 214, 221), (0.0, 2.0), (0.0, 2.0)),
                                        ((500, 516, 533, 550), (0.0, 1.0), (0.0, 2.5))])
def test_update_identity_matches_oracle(cuts, xr, yr):
    """Three block appends, each applied as v = L^-1[new rows] k*, var -= |v|^2,
    mu += v.z on the posterior of the leading n0 points, against the oracle's
    predict on the grown factor: 1e-12 normwise on mu and on sigma^2."""
    n1 = cuts[-1]
    x, y, obs, qx, qy = box_case(n1, xr, yr, seed=11)
    Lcm, alpha = O.fit(x, y, obs, ELL, SF2, SN2, M0)
    L = O.lower_from_colmajor(Lcm)
    n0 = cuts[0]
    L0 = L[:n0, :n0]
    a0 = O.chol_solve(O.colmajor_from_lower(L0), obs[:n0].astype(np.float64) - M0)
    mu, var = O.predict(O.colmajor_from_lower(L0), a0, x[:n0], y[:n0], qx, qy, ELL, SF2, M0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        dvar, dmu, _, _ = SM.update(L[:b, :b], x[:b], y[:b], obs[:b], M0, a, qx, qy, ELL, SF2)
        var = var + dvar
        mu = mu + dmu
    omu, ovar = O.predict(Lcm, alpha, x, y, qx, qy, ELL, SF2, M0)
    emu = np.abs(mu - omu).max() / np.abs(omu).max()
    evar = np.abs(var - ovar).max() / np.abs(ovar).max()
    print(f"n {n0} -> {n1}: mu {emu:.2e} var {evar:.2e}")
    assert emu < 1e-12 and evar < 1e-12, (emu, evar)


def test_linv_rows_are_the_inverse_rows():
    x, y, obs, _, _ = box_case(96, (0.0, 2.0), (0.0, 2.0), seed=3)
    L = O.lower_from_colmajor(O.fit(x, y, obs, ELL, SF2, SN2, 0.0)[0])
    R = SM.linv_rows(L, 80, 96)
    assert np.abs(R @ L - np.eye(96)[80:96]).max() < 1e-12


def test_stream_entry_points_reject_null_context_without_device():
    lib = N.lib()
    assert lib.sbo_tick_stream(None, None, None, 0, 2.0, 0.0, 0, 0, None, None, None, None, None, None, 0) == 1
    info = N.sbo_stream_info()
    info.struct_size = ctypes.sizeof(info)
    assert lib.sbo_get_stream(None, ctypes.byref(info)) == 1
    assert lib.sbo_stream_reset(None) == 1
    assert lib.sbo_debug_stream_state(None, None, None, 0) == 1
    # the header's struct and the binding's agree on the size the library writes
    assert ctypes.sizeof(N.sbo_stream_info) == 96
