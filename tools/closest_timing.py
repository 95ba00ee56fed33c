"""Device time of tj_closest_approach at the defaults beside tj_audit_timed at levels 6 and 1 on the 64-UAV SCN-C state after 50 iterations, in one process, with the
clock of tools/query_clock.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in
milliseconds; and the per-robot `windows` and `depth` of that state.  The figures of DESIGN.md 3e.  Run from the repository root on the GPU: python tools/closest_timing.py"""
import json
import numpy as np
from query_clock import scn_c_clock
slv, clock = scn_c_clock(50)
def timed(fn): return clock(fn, reps=30)
res = {"closest_default": timed(lambda: slv.closest_approach()), "closest_depth0": timed(lambda: slv.closest_approach(max_depth=0)),
       "audit_timed_L6": timed(lambda: slv.audit_timed(levels=6)), "audit_timed_L1": timed(lambda: slv.audit_timed(levels=1)), "audit_timed_L0": timed(lambda: slv.audit_timed(levels=0))}
a, t6 = slv.closest_approach(), slv.audit_timed(levels=6)
m = a["robot"] >= 0
res["in_range"] = int(m.sum()); res["flags"] = np.bincount(a["flags"], minlength=16).tolist()
res["windows"] = [int(a["windows"].min()), float(np.median(a["windows"])), int(a["windows"].max())]
res["depth"] = np.bincount(a["depth"], minlength=1).tolist()
res["width_max"] = float((a["hi"] - a["lo"]).max()); res["width_L6_max"] = float((t6["timed_hi"] - t6["timed_lo"]).max())
res["hi_min"] = float(a["hi"].min())
print(json.dumps(res))
slv.close()
