"""Device time of tj_path_crossings (the count-only call, and the rows at the defaults with cap = the count) beside tj_pair_approach on the 64-UAV SCN-C state after
20 iterations, and on the same state with z set to 0 through set_state, where every pair of paths crosses; in one process with the device otherwise idle, with the
clock of tools/query_clock.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30
in milliseconds; and the number of listed pairs, their flags, `windows` and `depth`.  The figures of DESIGN.md 3i.
Run from the repository root on the GPU: python tools/path_crossings_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=30)
n = C.c_int(0)
def call(rows, cap): slv._check(slv.lib.tj_path_crossings(slv._ctx, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rows, C.c_int(cap), C.byref(n)))
def measure():
    call(None, 0)
    rec = (pkg.TjCrossingRecord * max(n.value, 1))()
    cap = n.value
    res = {"crossings_count_only": timed(lambda: call(None, 0)), "crossings_rows": timed(lambda: call(rec, cap)), "crossings_python": timed(lambda: slv.path_crossings()),
           "pair_python": timed(lambda: slv.pair_approach())}
    a = slv.path_crossings()
    res["listed"] = len(a["robot"]); res["flags"] = np.bincount(a["flags"], minlength=64).tolist()
    if res["listed"]:
        res["windows"] = [int(a["windows"].min()), float(np.median(a["windows"])), int(a["windows"].max())]
        res["depth"] = np.bincount(a["depth"], minlength=1).tolist()
        res["width_max"] = float((a["hi"] - a["lo"]).max()); res["hi_min"] = float(a["hi"].min())
        res["gap_abs_min"] = float(np.abs(a["gap"][a["segment"] >= 0]).min()) if np.any(a["segment"] >= 0) else None
    return res
out = {"scn_c_20": measure()}
st = slv.get_state()
st["spline"][:, 2, :] = 0.0
slv.set_state(st)
out["scn_c_20_flat"] = measure()
print(json.dumps(out))
slv.close()
