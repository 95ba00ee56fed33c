"""Device time of tj_obstacle_windows (the count-only call, and the rows with cap = what the count-only call asks for) at dist = offset and dist = offset + 2 * margin on
the 64-UAV SCN-C state after 0 and after 20 iterations, beside tj_obstacle_approach at the same range, in one process with the device otherwise idle, with the clock of
tools/query_clock.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in
milliseconds; and the rows, their `windows`, `depth` and `leaves`.  No gate: the figures of DESIGN.md 3m.  Run from the repository root on the GPU: python tools/obstacle_windows_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
from pmc_traffic import source_id   # (the digest of bench.py:source_id: the build these times were measured on)
res = {"build": source_id()}
for iterations in (0, 20):
    slv, clock = scn_c_clock(iterations)
    def timed(fn): return clock(fn, reps=30)
    big = slv.params["offset"] + 2 * slv.params["margin"]
    for dist in (0.0, big):   # 0.0: the default, offset
        n = C.c_int(0)
        def call(rec, cap): return slv.lib.tj_obstacle_windows(slv._ctx, C.c_double(dist), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rec, C.c_int(cap), C.byref(n))
        def count(): slv._check(call(None, 0))
        a = slv.obstacle_windows(dist=dist or None)
        cap = max(len(a["robot"]), 1)
        rec = (pkg.TjObswinRow * cap)()
        def rows(): slv._check(call(rec, cap))
        r = {"count_only": timed(count), "rows": timed(rows), "python": timed(lambda: slv.obstacle_windows(dist=dist or None)),
             "obstacle_approach_same_range": timed(lambda: slv.obstacle_approach(range=dist or slv.params["offset"])), "n_rows": len(a["robot"]),
             "flags": np.bincount(a["flags"], minlength=64).tolist()}
        if len(a["robot"]):
            for f in ("windows", "depth", "leaves"):
                r[f] = [int(a[f].min()), float(np.median(a[f])), int(a[f].max())]
        res["it%d_%s" % (iterations, "offset" if dist == 0.0 else "dist_%g" % dist)] = r
    slv.close()
print(json.dumps(res))
