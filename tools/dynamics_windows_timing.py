"""Device time of tj_dynamics_windows at the default gates, at six gates (0.9 and 0.5 of both limits ABOVE, 0.5 of both BELOW) and of the count-only call, beside
tj_peak_dynamics and tj_obstacle_windows at their defaults, on the 64-UAV SCN-C state after 20 iterations, in one process, with the clock of tools/query_clock.py: a
hipEvent pair on the context's stream around the whole C call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in milliseconds; and the rows,
`windows` and `depth` of that state.  The figures of DESIGN.md 3o.  Run from the repository root on the GPU: python tools/dynamics_windows_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=30)
v, a = slv.params["vel_limit"], slv.params["acc_limit"]
six = [("speed", "above", 0.9 * v), ("accel", "above", 0.9 * a), ("speed", "above", 0.5 * v), ("accel", "above", 0.5 * a), ("speed", "below", 0.5 * v), ("accel", "below", 0.5 * a)]
rec = (pkg.TjDynwinRow * 65536)()
def c_call(gates, out, cap):
    gl = pkg.dynwin_gates(gates) if gates is not None else None
    arr = None if gl is None else (pkg.TjDynGate * len(gl))(*[pkg.TjDynGate(l, q, s) for q, s, l in gl])
    n = C.c_int(0)
    def call():
        rc = slv.lib.tj_dynamics_windows(slv._ctx, arr, C.c_int(0 if gl is None else len(gl)), C.c_double(-1.0), C.c_int(-1), C.c_int(0), out, C.c_int(cap), C.byref(n))
        assert rc == 0, rc
    return call
res = {"default_gates": timed(c_call(None, rec, 65536)), "six_gates": timed(c_call(six, rec, 65536)), "count_only_six": timed(c_call(six, None, 0)),
       "peak_default": timed(lambda: slv.peak_dynamics()), "obstacle_windows_default": timed(lambda: slv.obstacle_windows())}
for name, gates in (("default", None), ("six", six)):
    r = slv.dynamics_windows(gates=gates)
    res[name + "_rows"] = len(r["robot"])
    res[name + "_flags"] = np.bincount(r["flags"], minlength=64).tolist() if len(r["flags"]) else []
    res[name + "_windows"] = [int(r["windows"].min()), int(r["windows"].max())] if len(r["robot"]) else []
    res[name + "_depth"] = [int(r["depth"].min()), int(r["depth"].max())] if len(r["robot"]) else []
    res[name + "_leaves_max"] = int(r["leaves"].max()) if len(r["robot"]) else 0
print(json.dumps(res))
slv.close()
