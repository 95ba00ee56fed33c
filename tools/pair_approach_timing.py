"""Device time of tj_pair_approach (the count-only call, and the rows at the defaults with cap = the count) beside tj_closest_approach and tj_audit_timed at level 0 on the
64-UAV SCN-C state after 50 iterations, in one process with the device otherwise idle, with the clock of tools/query_clock.py: a hipEvent pair on the context's stream
around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in milliseconds; and the number of listed pairs, their `windows` and `depth`.
The figures of DESIGN.md 3g.  Run from the repository root on the GPU: python tools/pair_approach_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
slv, clock = scn_c_clock(50)
def timed(fn): return clock(fn, reps=30)
n = C.c_int(0)
def count(): slv._check(slv.lib.tj_pair_approach(slv._ctx, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n)))
count()
rec = (pkg.TjPairRecord * max(n.value, 1))()
def rows(): slv._check(slv.lib.tj_pair_approach(slv._ctx, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rec, C.c_int(n.value), C.byref(n)))
res = {"pair_count_only": timed(count), "pair_rows": timed(rows), "pair_python": timed(lambda: slv.pair_approach()),
       "closest_default": timed(lambda: slv.closest_approach()), "audit_timed_L0": timed(lambda: slv.audit_timed(levels=0))}
a = slv.pair_approach()
res["listed"] = len(a["robot"]); res["flags"] = np.bincount(a["flags"], minlength=16).tolist()
if res["listed"]:
    res["windows"] = [int(a["windows"].min()), float(np.median(a["windows"])), int(a["windows"].max())]
    res["depth"] = np.bincount(a["depth"], minlength=1).tolist()
    res["width_max"] = float((a["hi"] - a["lo"]).max()); res["hi_min"] = float(a["hi"].min())
print(json.dumps(res))
slv.close()
