"""The factorization's launches under a kernel trace, N = 4352 throughout (the
inverse splits at 4096; five outer panels at 1024, the last one on the rocBLAS
fallback): a default fit; refits with (SBO_OPT_CHOL_OUTER 512, SBO_OPT_CHOL_GEMM
0), CHOL_GEMM 1, 2 and 5; SBO_OPT_CHOLESKY 2, 0 and back to 1; SBO_OPT_INV_OVERLAP
32; SBO_OPT_CHOL_RESERVE 8; then appends of 1 point, of 300 with SBO_OPT_RESORT 0
(the block path: blocked_potrf on L22), of 1900 (past the capacity of 6528) and
one that triggers the re-sort.  Run once per build (SBO_LIB) and compare the lists:
    rocprofv3 --kernel-trace -d D -o run --output-format csv -- python3 tools/factor_trace.py
    python tools/factor_trace.py --list D profiles/<name>.txt"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from tick_trace import listing  # noqa: E402  (the per-queue listing, with this run's header)

HEADER = """\
# Kernel launches of one traced run at N = 4352: a default fit; refits with (CHOL_OUTER 512, CHOL_GEMM 0), CHOL_GEMM 1, 2, 5
# (outer panel 1024 again); SBO_OPT_CHOLESKY 2, 0, 1; INV_OVERLAP 32; CHOL_RESERVE 8; appends of 1, 300 (RESORT 0), 1900 (past
# the capacity) points and one that triggers the re-sort.
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
    gm = TerrainMapper(0, wl.hyper)

    def refit(*options):
        for k, v in options:
            gm.set_option(k, v)
        gm.fit(x, y, obs)
        torch.cuda.synchronize()

    refit()
    refit((N.SBO_OPT_CHOL_OUTER, 512), (N.SBO_OPT_CHOL_GEMM, 0))
    refit((N.SBO_OPT_CHOL_OUTER, 1024), (N.SBO_OPT_CHOL_GEMM, 1))
    refit((N.SBO_OPT_CHOL_GEMM, 2))
    refit((N.SBO_OPT_CHOL_GEMM, 5))
    refit((N.SBO_OPT_CHOL_GEMM, 4), (N.SBO_OPT_CHOLESKY, 2))
    refit((N.SBO_OPT_CHOLESKY, 0))
    refit((N.SBO_OPT_CHOLESKY, 1))
    refit((N.SBO_OPT_INV_OVERLAP, 32))
    refit((N.SBO_OPT_INV_OVERLAP, 0), (N.SBO_OPT_CHOL_RESERVE, 8))
    gm.set_option(N.SBO_OPT_CHOL_RESERVE, 0)
    ax, ay, ao = more_points(wl, 1 + 300 + 1900 + 1, seed=2024)
    a = 0
    for b, resort in ((1, 25), (300, 0), (1900, 0), (1, 25)):
        gm.set_option(N.SBO_OPT_RESORT, resort)
        gm.append(t(ax[a:a + b]), t(ay[a:a + b]), t(ao[a:a + b]))
        torch.cuda.synchronize()
        a += b
    assert gm.n == 4352 + a
    gm.close()


if __name__ == "__main__":
    main()
