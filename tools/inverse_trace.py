"""The f64 inverse's launches under a kernel trace, N = 4352 (the top splits at
2048 + 2304 at base 1024 and at 4096 + 256 at base 2048), per base: a default
fit; refits with SBO_OPT_INVERSE 0; SBO_OPT_INV_LEAVES 0, 1, 2; SBO_OPT_INV_PANELS
4; SBO_OPT_INV_OZ 0, 5, 6 with SBO_OPT_INV_OZ_MIN 2048; SBO_OPT_INV_OVERLAP 32;
SBO_OPT_INV_CHECK 2; SBO_OPT_INVERSE_BITS 32; then appends of 1, 300 and 1900
points.  Run once per build (SBO_LIB) and compare the lists:
    rocprofv3 --kernel-trace -d D -o run --output-format csv -- python3 tools/inverse_trace.py
    python tools/inverse_trace.py --list D profiles/<name>.txt"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from tick_trace import listing  # noqa: E402  (the per-queue listing, with this run's header)

HEADER = """\
# Kernel launches of one traced run at N = 4352, at SBO_OPT_INV_BASE 1024 and then 2048: a default fit; refits with INVERSE 0;
# INV_LEAVES 0, 1, 2; INV_PANELS 4; INV_OZ 0, 5, 6 with INV_OZ_MIN 2048; INV_OVERLAP 32; INV_CHECK 2; INVERSE_BITS 32; appends of
# 1, 300 and 1900 points.
# Per queue (numbered by first launch), the kernels in start order as ids of the legend below (ids by first appearance, queue by queue);
# names longer than 120 characters are cut, with 8 hex digits of the full name's SHA-1.
"""


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--list":
        return listing(sys.argv[2], sys.argv[3], HEADER)
    import numpy as np
    import torch
    from safe_bayesian_optimization_amd import TerrainMapper, synthetic
    from safe_bayesian_optimization_amd import _native as N
    from safe_bayesian_optimization_amd.terrain import more_points
    wl = synthetic(4352, 64, 64, seed=0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)  # noqa: E731
    x, y, obs = t(wl.x), t(wl.y), t(wl.obs)
    ax, ay, ao = more_points(wl, 1 + 300 + 1900, seed=2024)
    for base in (1024, 2048):
        gm = TerrainMapper(0, wl.hyper)
        gm.set_option(N.SBO_OPT_INV_BASE, base)

        def refit(*options):
            for k, v in options:
                gm.set_option(k, v)
            gm.fit(x, y, obs)
            torch.cuda.synchronize()

        refit()
        refit((N.SBO_OPT_INVERSE, 0))
        refit((N.SBO_OPT_INVERSE, 1), (N.SBO_OPT_INV_LEAVES, 0))
        refit((N.SBO_OPT_INV_LEAVES, 1))
        refit((N.SBO_OPT_INV_LEAVES, 2))
        refit((N.SBO_OPT_INV_PANELS, 4))
        refit((N.SBO_OPT_INV_PANELS, 16), (N.SBO_OPT_INV_OZ_MIN, 2048), (N.SBO_OPT_INV_OZ, 0))
        refit((N.SBO_OPT_INV_OZ, 5))
        refit((N.SBO_OPT_INV_OZ, 6))
        refit((N.SBO_OPT_INV_OZ_MIN, 0), (N.SBO_OPT_INV_OVERLAP, 32))
        refit((N.SBO_OPT_INV_OVERLAP, 0), (N.SBO_OPT_INV_CHECK, 2))
        refit((N.SBO_OPT_INV_CHECK, 1), (N.SBO_OPT_INVERSE_BITS, 32))
        refit((N.SBO_OPT_INVERSE_BITS, 64))
        a = 0
        for b in (1, 300, 1900):
            gm.append(t(ax[a:a + b]), t(ay[a:a + b]), t(ao[a:a + b]))
            torch.cuda.synchronize()
            a += b
        assert gm.n == 4352 + a
        gm.close()


if __name__ == "__main__":
    main()
