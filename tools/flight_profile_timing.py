"""Device time of tj_flight_profile on SCN-C (64 UAVs, 100 000 points, after 20 iterations) and on SCN-D-tri (256 UAVs, 1 000 000 triangles, its initial state) at
K = 101 and K = 1001 samples on the default grid, in one process: a hipEvent pair on the context's stream around the whole call (the upload of the times, the memset of
the records, the two kernels, the copy of the records), 3 warm calls, then (median, min, max) of 20 in milliseconds, and the number of records.  Nothing exists to
compare against, so there is no threshold.  The figures of DESIGN.md 3h.  Run from the repository root on the GPU:
    python tools/flight_profile_timing.py
The kernels' own share comes from a run of its own under the profiler (the tool then makes 5 calls per case and takes no times itself):
    rocprofv3 --kernel-trace --stats -f csv -d OUT -o fp -- python tools/flight_profile_timing.py --calls 5
whose kernel statistics list k_profile_points and k_profile_nearest (summed over both scenes and both K)."""
import ctypes as C, importlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
pkg = importlib.import_module("traj-opt-admm_amd")
from conftest import hip_runtime

calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
hip = hip_runtime()
res = {}
for name, scene, iters in (("scn_c", pkg.scenes.scn_c, 20), ("scn_d_tri", pkg.scenes.scn_d_tri, 0)):
    slv = pkg.Solver(scene(), stop=0.0)
    if iters:
        slv.iterate(iters)
    stream = C.c_void_p(slv.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for K in (101, 1001):
        times = pkg.profile_grid(slv.piece_times(), slv.P, K)
        t = np.ascontiguousarray(times)
        rec = (pkg.TjProfileSample * (slv.U * K))()
        fn = lambda: slv._check(slv.lib.tj_flight_profile(slv._ctx, t.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(K), rec))   # the C call alone: no numpy conversion
        if calls:
            for _ in range(calls):
                fn()
            continue
        for _ in range(3):
            fn()
        out = []
        for _ in range(20):
            assert hip.hipEventRecord(e0, stream) == 0
            fn()
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            out.append(ms.value)
        a = np.frombuffer(rec, dtype=np.dtype(pkg.TjProfileSample), count=slv.U * K)
        res["%s_K%d" % (name, K)] = dict(ms=[float(np.median(out)), float(min(out)), float(max(out))], records=slv.U * K, primitives=slv.N,
                                          obs_distance=[float(a["obs_distance"].min()), float(a["obs_distance"].max())])
    slv.close()
print(json.dumps(res))
