"""The launches of the four readers of the fitted state under a kernel trace, at
the shapes of their tests: a stream sequence (fit 250, tick, appends of 1, 17
and 33 with a tick each; fit 300 + 65 and fit 650 + 150 under
SBO_OPT_STREAM_MAX_ROWS 256), sbo_evidence on the three cases of
tests/test_gpu_evidence.py (default budget and dense, LOO to the host),
sbo_whatif on the three shapes of tests/test_gpu_whatif.py at p = 1, 17, 150
(dtrmm and dgemm weights), and sbo_sample on the same shapes at S = 1, 17, 150
and F = 1, 37, 256 (tests/test_gpu_sample.py).  Run once per build (SBO_LIB) and compare the lists:
    rocprofv3 --kernel-trace -d D -o run --output-format csv -- python3 tools/readers_trace.py
    python tools/readers_trace.py --list D profiles/<name>.txt"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from tick_trace import listing  # noqa: E402  (the per-queue listing, with this run's header)

HEADER = """\
# Kernel launches of one traced run of the readers of the fitted state at their tests' shapes.  Stream: fit 250, tick, appends
# of 1, 17, 33 with a tick each; fit 300 + append 65 and fit 650 + append 150 under STREAM_MAX_ROWS 256.  Evidence: one_tile_row,
# wide, lpsc_box at EVIDENCE_BUDGET 20 and 0 with LOO.  What-if: appended333, box24l, lpsc700precise at p = 1, 17, 150, cov and
# lo_new, WHATIF_GEMM 0 then 1.  Sample: the same shapes at S = 1, 17, 150 x F = 1, 37, 256 with paths.
# Per queue (numbered by first launch), the kernels in start order as ids of the legend below (ids by first appearance, queue by queue);
# names longer than 120 characters are cut, with 8 hex digits of the full name's SHA-1.
"""


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--list":
        return listing(sys.argv[2], sys.argv[3], HEADER)
    import torch
    from safe_bayesian_optimization_amd import _native as N
    from tests import test_gpu_evidence as TE
    from tests import test_gpu_sample as TS
    from tests import test_gpu_whatif as TW
    from tests.test_gpu_stream_tick import WIDE_SHAPES, Rig, wide_options
    dev = torch.device("cuda:0")
    r = Rig(dev, 250 + 1 + 17 + 33, seed=1)
    r.fit(250)
    r.tick()
    for b in (1, 17, 33):
        r.append(b)
        r.tick()
        assert r.gm.stream_info()["reason"] == "UPDATED"
    r.gm.close()
    for n0, b in WIDE_SHAPES:
        r = Rig(dev, n0 + b, seed=n0 + b, options=wide_options(b))
        r.fit(n0)
        r.tick()
        r.append(b)
        r.tick()
        assert r.gm.stream_info()["reason"] == "UPDATED"
        r.gm.close()
    for name in TE.CASES:
        c = TE.Case(name)      # (the default budget, then dense)
        c.gm.close()
    for shape, kw in TW.SHAPES.items():
        c = TW.Case(dev, **kw)
        for gemm in (0, 1):
            c.rig.gm.set_option(N.SBO_OPT_WHATIF_GEMM, gemm)
            for p in TW.PS:
                c.call(p, cov=True, lo_new=True)
        torch.cuda.synchronize()
        c.rig.gm.close()
    for shape, kw in TW.SHAPES.items():
        c = TS.SampleCase(dev, **kw)
        for S in TS.SS:
            for F in TS.FS:
                c.call(S, F)
        torch.cuda.synchronize()
        c.rig.gm.close()


if __name__ == "__main__":
    main()
