"""Device time of tj_obstacle_approach at the defaults and at max_depth = 0 beside tj_audit on the 64-UAV SCN-C state after 50 iterations, in one process, with the
clock of tools/query_clock.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in
milliseconds; and the per-robot `windows` and `depth` of that state.  The figures of DESIGN.md 3f.  Run from the repository root on the GPU: python tools/obstacle_approach_timing.py"""
import json
import numpy as np
from query_clock import scn_c_clock
slv, clock = scn_c_clock(50)
def timed(fn): return clock(fn, reps=30)
res = {"obstacle_default": timed(lambda: slv.obstacle_approach()), "obstacle_depth0": timed(lambda: slv.obstacle_approach(max_depth=0)), "audit": timed(lambda: slv.audit())}
a, au = slv.obstacle_approach(), slv.audit()
m = a["index"] >= 0
res["in_range"] = int(m.sum()); res["flags"] = np.bincount(a["flags"], minlength=16).tolist()
res["windows"] = [int(a["windows"].min()), float(np.median(a["windows"])), int(a["windows"].max())]
res["depth"] = np.bincount(a["depth"], minlength=1).tolist()
res["width_max"] = float((a["hi"] - a["lo"])[m].max()) if m.any() else 0.0
res["hi_min"] = float(a["hi"].min()); res["obs_clearance_min"] = float(au["obs_clearance"].min())
res["hi_minus_clearance"] = [float((a["hi"] - au["obs_clearance"])[m].min()), float((a["hi"] - au["obs_clearance"])[m].max())] if m.any() else []
print(json.dumps(res))
slv.close()
