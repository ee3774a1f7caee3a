"""The tick pipeline's launches under a kernel trace: fit N = 4352, a fast tick
of 4096 queries, a precise tick of them with the K* table in four chunks
(SBO_OPT_TABLE_MB 20), a query-cost call, a one-point append, a tick again.
Switching to the precise sweep runs the probe first (a fast sweep and its
reference).  Run once per build (SBO_LIB) and compare the lists:
    rocprofv3 --kernel-trace -d D -o run --output-format csv -- python3 tools/tick_trace.py
    python tools/tick_trace.py --list D profiles/<name>.txt"""
import csv
import glob
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADER = """\
# Kernel launches of one traced run: fit N = 4352, a fast tick of 4096 queries, a precise tick of
# them with the K* table in chunks (SBO_OPT_TABLE_MB 20: four chunks), a query-cost call, append 1 point, tick again.
# Switching to the precise sweep runs the probe first (a fast sweep and its reference, two chunks), so the
# trace holds six chunks: 6 kstar_table_kernel / predict_oz_kernel pairs, 10 plans.
# Per queue (numbered by first launch), the kernels in start order as ids of the legend below (ids by first appearance, queue by queue);
# names longer than 120 characters are cut, with 8 hex digits of the full name's SHA-1.
"""


def listing(d, out, header=HEADER):
    """Per-queue kernel lists under `header`; ids do not depend on how concurrent queues interleave in time."""
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    queues = {}
    for r in rows:
        n = r["Kernel_Name"]
        if len(n) > 120:
            n = n[:120] + "...#" + hashlib.sha1(n.encode()).hexdigest()[:8]
        queues.setdefault(r["Queue_Id"], []).append(n)
    ids = {}
    for ks in queues.values():
        for n in ks:
            ids.setdefault(n, len(ids))
    with open(out, "w") as fo:
        fo.write(header)
        fo.write(f"# total kernels {len(rows)}, queues {len(queues)}, distinct kernels {len(ids)}\n")
        for i, ks in enumerate(queues.values()):
            fo.write(f"queue {i}: {len(ks)} kernels\n")
            for j in range(0, len(ks), 30):
                fo.write("  " + " ".join(str(ids[n]) for n in ks[j:j + 30]) + "\n")
        fo.write("legend\n")
        for n, i in ids.items():
            fo.write(f"  {i} {n}\n")


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--list":
        return listing(sys.argv[2], sys.argv[3])
    import numpy as np
    import torch
    from safe_bayesian_optimization_amd import TerrainMapper, synthetic
    from safe_bayesian_optimization_amd import _native as N
    from safe_bayesian_optimization_amd.terrain import more_points
    wl = synthetic(4352, 64, 64, seed=0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)  # noqa: E731
    gm = TerrainMapper(0, wl.hyper)
    gm.set_option(N.SBO_OPT_PRECISION, 0)
    gm.fit(t(wl.x), t(wl.y), t(wl.obs))
    qx, qy = t(wl.qx), t(wl.qy)
    m = wl.qx.size
    o = dict(mu=torch.empty(m, device=dev), sd=torch.empty(m, device=dev),
             lo=torch.empty(m, dtype=torch.float64, device=dev), hi=torch.empty(m, dtype=torch.float64, device=dev),
             safe=torch.empty(m, dtype=torch.uint8, device=dev))
    gm.tick(qx, qy, wl.beta, wl.f_min, outputs=o)
    torch.cuda.synchronize()
    gm.set_option(N.SBO_OPT_TABLE_MB, 20)     # npad 4608: 2.5 MB per query block, 8 per chunk
    gm.set_option(N.SBO_OPT_PRECISION, 1)
    gm.tick(qx, qy, wl.beta, wl.f_min, outputs=o)
    torch.cuda.synchronize()
    gm.query_cost(qx, qy)
    torch.cuda.synchronize()
    gm.set_option(N.SBO_OPT_PRECISION, 0)
    ax, ay, ao = more_points(wl, 1, seed=2024)
    gm.append(t(ax), t(ay), t(ao))
    gm.tick(qx, qy, wl.beta, wl.f_min, outputs=o)
    torch.cuda.synchronize()
    gm.close()


if __name__ == "__main__":
    main()
