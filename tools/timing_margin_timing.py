"""Device time of tj_timing_margin (the count-only call, and the rows at the defaults with cap = the count) on the 64-UAV SCN-C state after 20 iterations, and on the
same state with z set to 0 and piece_time[u] *= 1 + 0.03 * u through set_state, where every pair of paths crosses at its own time; beside Solver.path_crossings() on
the first state, which DESIGN.md 3i records; in one process with the device otherwise idle, with the clock of tools/query_clock.py: a hipEvent pair on the context's
stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in milliseconds; and the number of listed pairs, their flags,
`windows` and `depth`.  The figures of DESIGN.md 3j.
Run from the repository root on the GPU: python tools/timing_margin_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=30)
n = C.c_int(0)
def call(rows, cap): slv._check(slv.lib.tj_timing_margin(slv._ctx, C.c_double(0.0), C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rows, C.c_int(cap), C.byref(n)))
def measure():
    call(None, 0)
    rec = (pkg.TjMarginRecord * max(n.value, 1))()
    cap = n.value
    res = {"margin_count_only": timed(lambda: call(None, 0)), "margin_rows": timed(lambda: call(rec, cap)), "margin_python": timed(lambda: slv.timing_margin())}
    a = slv.timing_margin()
    res["listed"] = len(a["robot"]); res["flags"] = np.bincount(a["flags"], minlength=128).tolist()
    if res["listed"]:
        res["windows"] = [int(a["windows"].min()), float(np.median(a["windows"])), int(a["windows"].max())]
        res["depth"] = np.bincount(a["depth"], minlength=1).tolist()
        res["width_max"] = float(np.nanmax(a["hi"] - a["lo"])); res["hi_min"] = float(a["hi"].min()); res["hi_max"] = float(a["hi"].max())
    return res
out = {"scn_c_20": measure()}
out["scn_c_20"]["crossings_python"] = timed(lambda: slv.path_crossings())
st = slv.get_state()
st["spline"][:, 2, :] = 0.0
st["piece_time"] = st["piece_time"] * (1 + 0.03 * np.arange(len(st["piece_time"])))
slv.set_state(st)
out["scn_c_20_flat_staggered"] = measure()
print(json.dumps(out))
slv.close()
