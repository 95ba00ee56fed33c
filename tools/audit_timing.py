"""Device time of tj_audit_timed (levels default, 0, 3, 6) and of tj_audit on the 64-UAV SCN-C state after 20 iterations, in one process: a hipEvent pair on the
context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 10 in milliseconds.  The figures of DESIGN.md 3d.
Run from the repository root on the GPU: python tools/audit_timing.py"""
import json
import numpy as np
from query_clock import scn_c_clock
slv, clock = scn_c_clock(20)
def timed(fn): return clock(fn, reps=10)
res = {}
for L in (None, 0, 3, 6):
    res["audit_timed_L%s" % ("default" if L is None else L)] = timed(lambda: slv.audit_timed(levels=L))
res["audit"] = timed(lambda: slv.audit())
a = slv.audit_timed()
res["flags"] = np.bincount(a["flags"], minlength=4).tolist(); res["lo_min"] = float(a["timed_lo"].min()); res["hi_min"] = float(a["timed_hi"].min())
print(json.dumps(res))
slv.close()
