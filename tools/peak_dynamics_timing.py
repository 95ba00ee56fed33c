"""Device time of tj_peak_dynamics at the defaults, at max_depth = 0 and at length_levels = 12 beside tj_obstacle_approach and tj_audit on the 64-UAV SCN-C state after 20
iterations, in one process, with the clock of tools/query_clock.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls,
then (median, min, max) of 30 in milliseconds; and the per-robot `windows` and `depth` of that state.  The figures of DESIGN.md 3k.  Run from the repository root on the
GPU: python tools/peak_dynamics_timing.py"""
import json
import numpy as np
from query_clock import scn_c_clock
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=30)
res = {"peak_default": timed(lambda: slv.peak_dynamics()), "peak_depth0": timed(lambda: slv.peak_dynamics(max_depth=0)), "peak_levels12": timed(lambda: slv.peak_dynamics(length_levels=12)),
       "obstacle_default": timed(lambda: slv.obstacle_approach()), "audit": timed(lambda: slv.audit())}
a, au = slv.peak_dynamics(), slv.audit()
for q in ("speed", "accel", "jerk"):
    res[q + "_windows"] = [int(a[q + "_windows"].min()), float(np.median(a[q + "_windows"])), int(a[q + "_windows"].max())]
    res[q + "_depth"] = [int(a[q + "_depth"].min()), int(a[q + "_depth"].max())]
    res[q + "_flags"] = np.bincount(a[q + "_flags"], minlength=16).tolist()
res["flags"] = np.bincount(a["flags"], minlength=16).tolist(); res["audit_flags"] = np.bincount(au["flags"], minlength=16).tolist()
res["time_scale"] = [float(a["time_scale"].min()), float(a["time_scale"].max())]
res["speed_hi_over_audit"] = [float((a["speed_hi"] / au["speed"]).min()), float((a["speed_hi"] / au["speed"]).max())]
res["accel_hi_over_audit"] = [float((a["accel_hi"] / au["accel"]).min()), float((a["accel_hi"] / au["accel"]).max())]
res["length_width_max"] = float(((a["length_hi"] - a["length_lo"]) / a["length_hi"]).max())
print(json.dumps(res))
slv.close()
