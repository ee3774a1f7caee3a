"""Device time of sbo_sample beside sbo_whatif's sweep of as many columns, and
the resource usage of its kernels.

    python tools/sample_timing.py [--n 16384] [--reps 3]  > profiles/sample.log
    python tools/sample_timing.py --resources            >> profiles/sample.log

Every line of profiles/sample.log is this tool's output, the headers included.

Two settings of n points, as tools/whatif_timing.py: bench.py's C4 synthetic
domain on a 1000 x 1000 grid, and config/lpsc.yaml's own box [0, 1] x [0, 2.5]
on the mapper's 300 x 120 grid.  Per setting: fit n points, sbo_tick_stream
(the full sweep, kept), then per repetition sbo_sample (keys and counts, no
paths) for S = 16 and 64 samples at F = 256 and 1024 features: the weights'
time (the draws, the feature walk over the training points, the two triangular
products in 128-row chunks, the sums, kernel_err) and the sweep's time
(sample_kernel and the key reduction), both from sbo_profile's events, the
tiles kept and the cutoff L.  Beside each S, sbo_whatif's sweep for p = S
candidates uniform over the data box on the same state: the same k-tile walk
without the feature walk (its cutoff differs: both L are printed).  F = 4 gives
the sweep with next to no feature work, so the split between the K* part and
the feature part can be read off.  Medians over the repetitions after one
warm-up repetition.

--resources needs no GPU: it compiles csrc/sample.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage and prints each kernel's registers,
scratch, occupancy and LDS.
"""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profile_ms(gm, fn):
    """(predict ms, fill ms) of sbo_profile's events round the launches fn makes."""
    from safe_bayesian_optimization_amd import _native as N
    lib = N.lib()
    gm.ctx.check(lib.sbo_profile(gm.ctx.handle, 1))
    out = fn()
    pm, fm = ctypes.c_double(), ctypes.c_double()
    pc, fc = ctypes.c_int64(), ctypes.c_int64()
    gm.ctx.check(lib.sbo_profile_read(gm.ctx.handle, ctypes.byref(pm), ctypes.byref(pc), ctypes.byref(fm),
                                      ctypes.byref(fc)))
    gm.ctx.check(lib.sbo_profile(gm.ctx.handle, 0))
    return pm.value, fm.value, out


def run(name, wl, reps):
    import torch

    from safe_bayesian_optimization_amd import TerrainMapper
    from safe_bayesian_optimization_amd.terrain import uniform
    dev = torch.device("cuda:0")
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32), device=dev)  # noqa: E731
    n = wl.x.size
    X, Y, OBS, QX, QY = f32(wl.x), f32(wl.y), f32(wl.obs), f32(wl.qx), f32(wl.qy)
    m = QX.numel()
    outs = dict(mu=torch.empty(m, device=dev), sd=torch.empty(m, device=dev),
                lo=torch.empty(m, dtype=torch.float64, device=dev), hi=torch.empty(m, dtype=torch.float64, device=dev),
                safe=torch.empty(m, dtype=torch.uint8, device=dev))
    gm = TerrainMapper(0, wl.hyper)
    gm.fit(X, Y, OBS)
    gm.tick_stream(QX, QY, wl.beta, wl.f_min, outputs=outs)
    rows, wrows = {}, {}
    for rep in range(reps + 1):
        for S in (16, 64):
            for F in (4, 256, 1024):
                sweep, weights, w = profile_ms(gm, lambda: gm.sample(S, 7, wl.beta, wl.f_min, features=F, device=dev))
                if rep:
                    rows.setdefault((S, F), []).append((weights, sweep, w))
            u = uniform(7 + S, 2 * S)
            cx = f32(wl.x.min() + u[0::2] * (wl.x.max() - wl.x.min()))
            cy = f32(wl.y.min() + u[1::2] * (wl.y.max() - wl.y.min()))
            sweep, weights, w = profile_ms(gm, lambda: gm.whatif(cx, cy, wl.beta, wl.f_min))
            if rep:
                wrows.setdefault(S, []).append((weights, sweep, w))
    print(f"{name}: n={n} m={m}", flush=True)
    for (S, F), v in sorted(rows.items()):
        wms, sms = float(np.median([a[0] for a in v])), float(np.median([a[1] for a in v]))
        w = v[-1][2]
        idx = w["idx"].cpu().numpy()
        print(f"{name}: sample S={S} F={F} weights_ms={wms:.3f} sweep_ms={sms:.3f} tiles_kept={w['tiles_kept']} "
              f"tiles_total={w['tiles_total']} L={w['cutoff_log2']} err_path={w['err_path']:.3e} "
              f"w_l1_max={w['w_l1_max']:.4g} kernel_err={w['kernel_err']:.4f} distinct_keys={np.unique(idx).size}",
              flush=True)
    for S, v in sorted(wrows.items()):
        wms, sms = float(np.median([a[0] for a in v])), float(np.median([a[1] for a in v]))
        w = v[-1][2]
        print(f"{name}: whatif p={S} weights_ms={wms:.3f} sweep_ms={sms:.3f} tiles_kept={w['tiles_kept']} "
              f"tiles_total={w['tiles_total']} L={w['cutoff_log2']}", flush=True)
    gm.close()


def resources():
    pkg = os.path.join(ROOT, "safe_bayesian_optimization_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--offload-arch=gfx950",
           "-I/opt/rocm/include", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(pkg, "csrc", "sample.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    print("# tools/sample_timing.py --resources: csrc/sample.hip for gfx950 (-O3), -Rpass-analysis=kernel-resource-usage")
    cur, want = None, ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
    for line in err.splitlines():
        f = re.search(r"remark: Function Name: (\S+)", line)
        if f:
            name = subprocess.run(["c++filt", f.group(1)], capture_output=True, text=True).stdout.strip() or f.group(1)
            name = re.sub(r"\(.*", "", name.replace("sbo::(anonymous namespace)::", "").replace("void ", ""))
            cur = {"name": name}
            continue
        v = re.search(r"remark:\s+(.+?): (\d+)", line)
        if cur is not None and v and v.group(1) in want:
            cur[v.group(1)] = int(v.group(2))
            if len(cur) == len(want) + 1:
                print(f"{cur['name']}: vgprs={cur['VGPRs']} agprs={cur['AGPRs']} "
                      f"scratch_bytes_per_lane={cur['ScratchSize [bytes/lane]']} "
                      f"occupancy_waves_per_simd={cur['Occupancy [waves/SIMD]']} "
                      f"lds_bytes_per_block={cur['LDS Size [bytes/block]']}")
                cur = None


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--n", type=int, default=16384)
    a.add_argument("--reps", type=int, default=3)
    a.add_argument("--resources", action="store_true")
    a = a.parse_args()
    if a.resources:
        return resources()
    print(f"# tools/sample_timing.py --n {a.n} --reps {a.reps}: medians of {a.reps} warm repetitions, 1 GPU",
          flush=True)
    from safe_bayesian_optimization_amd.terrain import synthetic, synthetic_box
    run("C4 synthetic 1000x1000", synthetic(a.n, 1000, 1000, seed=0, name="C4"), a.reps)
    run("lpsc box 300x120", synthetic_box(a.n, 300, 120, seed=0), a.reps)


if __name__ == "__main__":
    main()
