"""Device time of tj_obstacle_approach at the defaults and at max_depth = 0 beside tj_audit on the 64-UAV SCN-C state after 50 iterations, in one process, with the
clock of tools/audit_timing.py: a hipEvent pair on the context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 30 in
milliseconds; and the per-robot `windows` and `depth` of that state.  The figures of DESIGN.md 3f.  Run from the repository root on the GPU: python tools/obstacle_approach_timing.py"""
import ctypes as C, importlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
pkg = importlib.import_module("traj-opt-admm_amd")
from conftest import hip_runtime
hip = hip_runtime()
slv = pkg.Solver(pkg.scenes.scn_c(), stop=0.0)
slv.iterate(50)
stream = C.c_void_p(slv.stream())
e0, e1 = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
def timed(fn, reps=30, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        assert hip.hipEventRecord(e0, stream) == 0
        fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        out.append(ms.value)
    return float(np.median(out)), float(min(out)), float(max(out))
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
