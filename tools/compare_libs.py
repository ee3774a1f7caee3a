"""Bitwise A/B of two libsbo builds on the same ticks (GPU): each library runs
in its own process (SBO_LIB), writes the fit's tile bounds, mu/sd/lo/hi/S and the key of a few
workloads, and the outputs are compared element by element.

  python tools/compare_libs.py LIB_A LIB_B [--configs C4 C2 box]
  python tools/compare_libs.py LIB_A LIB_B --factor-matrix   (fits under the Cholesky's options, appends)
  python tools/compare_libs.py LIB_A LIB_B --inverse-matrix  (fits under the f64 inverse's options, appends)
  python tools/compare_libs.py LIB_A LIB_B --readers-matrix  (the streaming update, sbo_whatif, sbo_sample and sbo_evidence)"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import CONFIGS, synthetic_box
out = {{}}
dev = torch.device("cuda:0")
for name in {configs!r}:
    if name == "box":
        wl = synthetic_box(4096, 256, 256, seed=1)
    else:
        n, gw, gh = CONFIGS[name]
        wl = synthetic(n, gw, gh, seed=0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    gm = TerrainMapper(0, wl.hyper)
    gm.fit(t(wl.x), t(wl.y), t(wl.obs))
    nI = (gm.n + 255) // 256
    b = np.empty(8 * sum(4 * (I + 1) for I in range(nI)), np.float32)   # the plan's tile bounds
    gm.ctx.check(N.lib().sbo_get_tile_bounds(gm.ctx.handle, b.ctypes.data, b.size))
    out[name + "_tile_bounds"] = b
    m = wl.qx.size
    o = dict(mu=torch.empty(m, device=dev), sd=torch.empty(m, device=dev),
             lo=torch.empty(m, dtype=torch.float64, device=dev), hi=torch.empty(m, dtype=torch.float64, device=dev),
             safe=torch.empty(m, dtype=torch.uint8, device=dev))
    k = gm.tick(t(wl.qx), t(wl.qy), wl.beta, wl.f_min, outputs=o).clone()
    torch.cuda.synchronize()
    for kk, v in o.items():
        out[name + "_" + kk] = v.cpu().numpy()
    out[name + "_key"] = k.cpu().numpy()
    gm.close()
np.savez({path!r}, **out)
print("ok", N.LIB_PATH)
'''

# --factor-matrix: the factorization's options and the append paths.  Per case L, alpha, the f32 view of
# the inverse (sbo_get_inverse), mu and sd.  Compare a build with itself first: the rocBLAS paths count as
# evidence only where they repeat.
FACTOR_CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, {root!r})
from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N
out = {{}}
DEFAULTS = ((N.SBO_OPT_CHOLESKY, 1), (N.SBO_OPT_CHOL_OUTER, 1024), (N.SBO_OPT_CHOL_GEMM, 4), (N.SBO_OPT_INV_OVERLAP, 0),
            (N.SBO_OPT_CHOL_RESERVE, 0), (N.SBO_OPT_RESORT, 25))
gm = None
def record(name, wl):
    L, alpha = gm.factor()
    A = np.zeros((gm.n, gm.n), np.float32)
    gm.ctx.check(N.lib().sbo_get_inverse(gm.ctx.handle, A.ctypes.data))
    mu, sd = gm.predict(wl.qx, wl.qy)
    for k, v in (("L", L), ("alpha", alpha), ("inv", A), ("mu", mu), ("sd", sd)):
        v = np.ascontiguousarray(v)     # (arrays past 1 MiB: their SHA-256)
        out[name + "_" + k] = v if v.nbytes <= 1 << 20 else np.frombuffer(hashlib.sha256(v).digest(), np.uint8)
def fit(name, wl, n, options):
    for k, v in DEFAULTS + tuple(options):
        gm.set_option(k, v)
    gm.fit(wl.x[:n], wl.y[:n], wl.obs[:n])
    record(name, wl)
# the option list of tests/test_gpu_parity.py::test_blocked_cholesky_matches_spotrf: (CHOLESKY, CHOL_OUTER, CHOL_GEMM)
CHOL = [(0, 1024, 0), (2, 1024, 0), (1, 128, 0), (1, 256, 0), (1, 512, 0), (1, 1024, 0), (1, 512, 1), (1, 512, 2),
        (1, 512, 4), (1, 512, 5), (1, 128, 4), (1, 256, 4), (1, 1024, 4), (1, 1024, 0)]
for n in (129, 300, 2048, 4100):
    wl = synthetic(n, 24, 20, seed=n + 3)
    gm = TerrainMapper(0, wl.hyper)      # one context per size: every case after the first runs on used streams
    for i, (ch, outer, gemm) in enumerate(CHOL):
        fit(f"n{{n}}_{{i:02d}}_chol{{ch}}_outer{{outer}}_gemm{{gemm}}", wl, n,
            ((N.SBO_OPT_CHOLESKY, ch), (N.SBO_OPT_CHOL_OUTER, outer), (N.SBO_OPT_CHOL_GEMM, gemm)))
    if n == 4100:
        for ov in (0, 32, 0):
            fit(f"n{{n}}_overlap{{ov}}", wl, n, ((N.SBO_OPT_INV_OVERLAP, ov),))
    for j, rs in enumerate((0, 8, 0)):
        for gemm in (0, 2, 4):
            fit(f"n{{n}}_reserve{{j}}_{{rs}}_gemm{{gemm}}", wl, n,
                ((N.SBO_OPT_CHOL_OUTER, 128), (N.SBO_OPT_CHOL_GEMM, gemm), (N.SBO_OPT_CHOL_RESERVE, rs)))
    gm.close()
wl = synthetic(6401, 24, 20, seed=6410)     # rocBLAS trailing updates on both sides of the ssyrk / sgemm switch at 6144 rows
gm = TerrainMapper(0, wl.hyper)
for gemm in (0, 1):
    fit(f"n6401_outer128_gemm{{gemm}}", wl, 6401, ((N.SBO_OPT_CHOL_OUTER, 128), (N.SBO_OPT_CHOL_GEMM, gemm)))
gm.close()
wl = synthetic(600, 24, 20, seed=11)
for b, resort in ((1, 0), (200, 0), (200, 25)):     # (200 of 300 with SBO_OPT_RESORT 25: the re-sort)
    for ch in (1, 0):
        gm = TerrainMapper(0, wl.hyper)
        fit(f"append{{b}}_resort{{resort}}_chol{{ch}}_fit", wl, 300, ((N.SBO_OPT_CHOLESKY, ch), (N.SBO_OPT_RESORT, resort)))
        gm.append(wl.x[300:300 + b], wl.y[300:300 + b], wl.obs[300:300 + b])
        record(f"append{{b}}_resort{{resort}}_chol{{ch}}", wl)
        out[f"append{{b}}_resort{{resort}}_chol{{ch}}_order"] = gm.order()
        gm.close()
np.savez({path!r}, **out)
print("ok", N.LIB_PATH, len(out), "arrays")
'''

# --inverse-matrix: the f64 inverse's options at sizes that give its tree every shape (base 1024 and 2048: a
# one-column block, two levels, the smallest sliced top, a split lower-right block, a sliced second level),
# then the append paths.  Per case L, alpha, the f32 view of the inverse, mu and sd, as --factor-matrix, and the
# tile bounds (bits32: the norms alone over the packed tiles; the appends: the row blocks past the kept ones).
INVERSE_CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, {root!r})
from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N
out = {{}}
DEFAULTS = ((N.SBO_OPT_INVERSE, 1), (N.SBO_OPT_INVERSE_BITS, 64), (N.SBO_OPT_INV_LEAVES, 2), (N.SBO_OPT_INV_PANELS, 16),
            (N.SBO_OPT_INV_OZ, 6), (N.SBO_OPT_INV_OZ_MIN, 0), (N.SBO_OPT_INV_OVERLAP, 0), (N.SBO_OPT_INV_CHECK, 1))
CASES = [("default", ()), ("inverse0", ((N.SBO_OPT_INVERSE, 0),)),
         ("leaves0", ((N.SBO_OPT_INV_LEAVES, 0),)), ("leaves1", ((N.SBO_OPT_INV_LEAVES, 1),)),
         ("leaves2", ((N.SBO_OPT_INV_LEAVES, 2),)), ("panels4", ((N.SBO_OPT_INV_PANELS, 4),)),
         ("oz0", ((N.SBO_OPT_INV_OZ_MIN, 2048), (N.SBO_OPT_INV_OZ, 0))),
         ("oz5", ((N.SBO_OPT_INV_OZ_MIN, 2048), (N.SBO_OPT_INV_OZ, 5))),
         ("oz6", ((N.SBO_OPT_INV_OZ_MIN, 2048), (N.SBO_OPT_INV_OZ, 6))),
         ("overlap32", ((N.SBO_OPT_INV_OVERLAP, 32),)), ("overlap32_oz0", ((N.SBO_OPT_INV_OVERLAP, 32), (N.SBO_OPT_INV_OZ, 0))),
         ("check2", ((N.SBO_OPT_INV_CHECK, 2),)), ("bits32", ((N.SBO_OPT_INVERSE_BITS, 32),)), ("default_again", ())]
gm = None
def record(name, wl):
    L, alpha = gm.factor()
    A = np.zeros((gm.n, gm.n), np.float32)
    gm.ctx.check(N.lib().sbo_get_inverse(gm.ctx.handle, A.ctypes.data))
    mu, sd = gm.predict(wl.qx, wl.qy)
    b = np.empty(8 * sum(4 * (I + 1) for I in range((gm.n + 255) // 256)), np.float32)   # the plan's tile bounds
    gm.ctx.check(N.lib().sbo_get_tile_bounds(gm.ctx.handle, b.ctypes.data, b.size))
    for k, v in (("L", L), ("alpha", alpha), ("inv", A), ("mu", mu), ("sd", sd), ("tile_bounds", b)):
        v = np.ascontiguousarray(v)     # (arrays past 1 MiB: their SHA-256)
        out[name + "_" + k] = v if v.nbytes <= 1 << 20 else np.frombuffer(hashlib.sha256(v).digest(), np.uint8)
for n in (1025, 2049, 3000, 3073, 4100, 9000):
    wl = synthetic(n, 24, 20, seed=n + 3)
    for base in (1024, 2048):
        gm = TerrainMapper(0, wl.hyper)      # one context per tree: every case after the first runs on used streams
        gm.set_option(N.SBO_OPT_INV_BASE, base)
        for name, options in CASES:
            for k, v in DEFAULTS + tuple(options):
                gm.set_option(k, v)
            gm.fit(wl.x, wl.y, wl.obs)
            record(f"n{{n}}_base{{base}}_{{name}}", wl)
        gm.close()
wl = synthetic(6600, 24, 20, seed=17)
for base in (1024, 2048):
    gm = TerrainMapper(0, wl.hyper)
    gm.set_option(N.SBO_OPT_INV_BASE, base)
    gm.fit(wl.x[:4352], wl.y[:4352], wl.obs[:4352])
    a = 4352
    for b in (1, 300, 1900):
        gm.append(wl.x[a:a + b], wl.y[a:a + b], wl.obs[a:a + b])
        a += b
        record(f"append{{b}}_base{{base}}", wl)
    gm.close()
np.savez({path!r}, **out)
print("ok", N.LIB_PATH, len(out), "arrays")
'''

# --readers-matrix: the readers of the fitted state (the streaming update, sbo_whatif, sbo_sample, sbo_evidence) at their
# tests' shapes, one context per shape.  Timings (ms) are left out.
READERS_CHILD = r'''
import ctypes, sys, numpy as np, torch
sys.path.insert(0, {root!r})
from safe_bayesian_optimization_amd import TerrainMapper
from safe_bayesian_optimization_amd import _native as N
from tests import evidence_model as EM
from tests import test_gpu_evidence as TE
from tests import test_gpu_sample as TS
from tests import test_gpu_whatif as TW
from tests.test_gpu_stream_tick import WIDE_SHAPES, Rig, wide_options
out = {{}}
dev = torch.device("cuda:0")
def put(name, d, skip=("ms",)):
    for k, v in d.items():
        if k in skip:
            continue
        out[name + "_" + k] = np.frombuffer(v.encode(), np.uint8) if isinstance(v, str) else np.asarray(v)
# stream: per skip setting a refit, the full tick that keeps its posterior, the append, the update
def stream(name, r, n0, b, skips):
    for skip in skips:
        r.gm.set_option(N.SBO_OPT_TILE_SKIP, skip)
        r.fit(n0)
        r.tick()
        r.append(b)
        h, key = r.tick()
        info = r.gm.stream_info()
        assert (info["path"], info["rows"]) == (1, b), info
        mu, var = r.gm.stream_state(r.m)
        tag = f"stream_{{name}}_skip{{skip}}"
        put(tag, h)
        put(tag, dict(key=np.array(key, np.float64), state_mu=mu, state_var=var))
        put(tag, {{k: info[k] for k in ("cutoff_log2", "tiles_kept", "tiles_total", "reason", "err_var", "err_mean")}})
for n0, b in [(250, 1), (250, 17), (250, 33)] + WIDE_SHAPES:
    r = Rig(dev, n0 + b, seed=3 * n0 + b, options=wide_options(b))
    stream(f"n{{n0}}_b{{b}}", r, n0, b, (-1, 0, 200))
    r.gm.close()
r = Rig(dev, 516, seed=17, x_range=(0.0, 1.0), y_range=(0.0, 2.5), options=[(N.SBO_OPT_PRECISION, 1)])
stream("precise_n500_b16", r, 500, 16, (-1,))
r.gm.close()
# what-if
for shape, kw in TW.SHAPES.items():
    c = TW.Case(dev, **kw)
    for gemm in (0, 1):
        for skip in (-1, 0):
            c.rig.gm.set_option(N.SBO_OPT_WHATIF_GEMM, gemm)
            c.rig.gm.set_option(N.SBO_OPT_TILE_SKIP, skip)
            for p in TW.PS:
                for device in (False, True):
                    put(f"whatif_{{shape}}_p{{p}}_gemm{{gemm}}_skip{{skip}}_{{'dev' if device else 'host'}}",
                        c.call(p, device=device, cov=True, lo_new=True))
    c.rig.gm.close()
# sample paths
for shape, kw in TW.SHAPES.items():
    c = TS.SampleCase(dev, **kw)
    for skip in (-1, 0):
        c.rig.gm.set_option(N.SBO_OPT_TILE_SKIP, skip)
        for S in TS.SS:
            for F in TS.FS:
                for device in (False, True):
                    put(f"sample_{{shape}}_S{{S}}_F{{F}}_skip{{skip}}_{{'dev' if device else 'host'}}",
                        c.call(S, F, device=device))
    c.rig.gm.close()
# evidence
def evidence(name, gm):
    for budget in (20, 0):
        gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, budget)
        st, info, mean, var = TE.call(gm)
        assert st == 0
        put(f"evidence_{{name}}_budget{{budget}}_host", TE.as_dict(info, mean, var))
        dm, dv = (torch.full((gm.n,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        st, info, _, _ = TE.call(gm, flags=N.SBO_DEVICE_PTRS, mean=dm, var=dv)
        assert st == 0
        torch.cuda.synchronize()
        put(f"evidence_{{name}}_budget{{budget}}_dev", TE.as_dict(info, dm.cpu().numpy(), dv.cpu().numpy()))
for name, (n, xr, yr) in TE.CASES.items():
    x, y, obs = EM.case_data(n, xr, yr, TE.ELL, TE.HYPER.noise_level)
    gm = TerrainMapper(0, TE.HYPER)
    gm.fit(x, y, obs)
    evidence(name, gm)
    gm.close()
x, y, obs = EM.case_data(1027, (0.0, 12 * TE.ELL), (0.0, 12 * TE.ELL), TE.ELL, TE.HYPER.noise_level, seed=5)
gm = TerrainMapper(0, TE.HYPER)
gm.fit(x[:1000], y[:1000], obs[:1000])
gm.append(x[1000:], y[1000:], obs[1000:])      # 1000 -> 1027: across the k-tile boundary at 1024
evidence("append1027", gm)
gm.close()
np.savez({path!r}, **out)
print("ok", N.LIB_PATH, len(out), "arrays")
'''


def run(lib, configs, path, child=CHILD):
    env = dict(os.environ, SBO_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, "-c", child.format(root=ROOT, configs=configs, path=path)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{lib}: {r.stderr[-3000:]}")
    print(r.stdout.strip().splitlines()[-1])
    return dict(np.load(path))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("lib_a")
    p.add_argument("lib_b")
    p.add_argument("--configs", nargs="+", default=["C4", "C2", "box"])
    p.add_argument("--factor-matrix", action="store_true",
                   help="the factorization's option matrix and the append paths instead of the ticks")
    p.add_argument("--inverse-matrix", action="store_true",
                   help="the f64 inverse's option matrix and the append paths instead of the ticks")
    p.add_argument("--readers-matrix", action="store_true",
                   help="the streaming update, sbo_whatif, sbo_sample and sbo_evidence at their tests' shapes instead of "
                        "the ticks")
    a = p.parse_args()
    child = FACTOR_CHILD if a.factor_matrix else INVERSE_CHILD if a.inverse_matrix else \
        READERS_CHILD if a.readers_matrix else CHILD
    a.factor_matrix |= a.inverse_matrix | a.readers_matrix      # (reported alike)
    A = run(a.lib_a, a.configs, os.environ.get("CMP_OUT", "/tmp") + "/cmp_a.npz", child)
    B = run(a.lib_b, a.configs, os.environ.get("CMP_OUT", "/tmp") + "/cmp_b.npz", child)
    same = sorted(A) == sorted(B)
    for k in sorted(A):
        eq = k in B and A[k].shape == B[k].shape and np.array_equal(A[k], B[k])
        d = "" if eq or k not in B or A[k].shape != B[k].shape else \
            f" max|d| {np.abs(A[k].astype(np.float64) - B[k].astype(np.float64)).max():.3e}, " \
            f"{np.count_nonzero(A[k] != B[k])} of {A[k].size} differ"
        if not (a.factor_matrix and eq):     # (the matrix: hundreds of arrays, only the different ones by name)
            print(f"{k:14s} {'bitwise equal' if eq else 'DIFFERENT'}{d}")
        same &= eq
    print(f"{len(A)} arrays: " + ("ALL BITWISE EQUAL" if same else "OUTPUTS DIFFER"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
