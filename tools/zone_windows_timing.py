"""Device time of tj_zone_windows at the measurement's 20 zones (tests/zone_windows_ref.py measurement_zones: two boxes, an altitude band, the 32-face prism and a
ball, each in both senses at levels 0 and -offset), at the prism alone, at the ball alone and of the count-only call, beside tj_dynamics_windows at six gates and
tj_obstacle_windows at its defaults, on the 64-UAV SCN-C state after 20 iterations, in one process, with the clock of tools/query_clock.py: a hipEvent pair on the
context's stream around the whole C call (uploads, memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in milliseconds; and the rows, `windows`
and `depth` of that state.  The figures of DESIGN.md 3p.  Run from the repository root on the GPU: python tools/zone_windows_timing.py"""
import ctypes as C
import json
import numpy as np
from query_clock import pkg, scn_c_clock
import zone_windows_ref as Z
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=30)
ref = Z.Ref(pkg, slv.get_state(), slv.P, slv.res)
zones = Z.measurement_zones(ref, slv.params["offset"])
prism, ball = zones[12:13], zones[16:17]
assert len(zones) == 20 and len(prism[0][3]) == 32 and ball[0][0] == Z.BALL
v, a = slv.params["vel_limit"], slv.params["acc_limit"]
six = [("speed", "above", 0.9 * v), ("accel", "above", 0.9 * a), ("speed", "above", 0.5 * v), ("accel", "above", 0.5 * a), ("speed", "below", 0.5 * v), ("accel", "below", 0.5 * a)]
rec = (pkg.TjZonewinRow * 65536)()
def c_call(zl, out, cap):
    arr, table = pkg.zonewin_pack(zl)
    n = C.c_int(0)
    def call():
        rc = slv.lib.tj_zone_windows(slv._ctx, arr, C.c_int(len(zl)), table.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(len(table)), C.c_double(-1.0), C.c_int(-1), C.c_int(0), out,
                                     C.c_int(cap), C.byref(n))
        assert rc == 0, rc
    return call
def dyn_call(gates, out, cap):
    gl = pkg.dynwin_gates(gates)
    arr = (pkg.TjDynGate * len(gl))(*[pkg.TjDynGate(l, q, s) for q, s, l in gl])
    n = C.c_int(0)
    def call():
        rc = slv.lib.tj_dynamics_windows(slv._ctx, arr, C.c_int(len(gl)), C.c_double(-1.0), C.c_int(-1), C.c_int(0), out, C.c_int(cap), C.byref(n))
        assert rc == 0, rc
    return call
dyn_rec = (pkg.TjDynwinRow * 65536)()
res = {"twenty_zones": timed(c_call(zones, rec, 65536)), "count_only_twenty": timed(c_call(zones, None, 0)), "prism_32_faces": timed(c_call(prism, rec, 65536)),
       "ball": timed(c_call(ball, rec, 65536)), "dynamics_windows_six_gates": timed(dyn_call(six, dyn_rec, 65536)),
       "obstacle_windows_default": timed(lambda: slv.obstacle_windows())}
for name, zl in (("twenty", zones), ("prism", prism), ("ball", ball)):
    r = slv.zone_windows(zl)
    res[name + "_rows"] = len(r["robot"])
    res[name + "_flags"] = np.bincount(r["flags"], minlength=64).tolist() if len(r["flags"]) else []
    res[name + "_windows"] = [int(r["windows"].min()), int(r["windows"].max())] if len(r["robot"]) else []
    res[name + "_depth"] = [int(r["depth"].min()), int(r["depth"].max())] if len(r["robot"]) else []
    res[name + "_leaves_max"] = int(r["leaves"].max()) if len(r["robot"]) else 0
print(json.dumps(res))
slv.close()
