"""Device time of tj_audit_timed (levels default, 0, 3, 6) and of tj_audit on the 64-UAV SCN-C state after 20 iterations, in one process: a hipEvent pair on the
context's stream around the whole call (memsets, kernels, copies), 3 warm calls, then (median, min, max) of 10 in milliseconds.  The figures of DESIGN.md 3d.
Run from the repository root on the GPU: python tools/audit_timing.py"""
import ctypes as C, importlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
pkg = importlib.import_module("traj-opt-admm_amd")
from conftest import hip_runtime
hip = hip_runtime()
slv = pkg.Solver(pkg.scenes.scn_c(), stop=0.0)
slv.iterate(20)
stream = C.c_void_p(slv.stream())
e0, e1 = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
def timed(fn, reps=10, warm=3):
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
res = {}
for L in (None, 0, 3, 6):
    res["audit_timed_L%s" % ("default" if L is None else L)] = timed(lambda: slv.audit_timed(levels=L))
res["audit"] = timed(lambda: slv.audit())
a = slv.audit_timed()
res["flags"] = np.bincount(a["flags"], minlength=4).tolist(); res["lo_min"] = float(a["timed_lo"].min()); res["hi_min"] = float(a["timed_hi"].min())
print(json.dumps(res))
slv.close()
