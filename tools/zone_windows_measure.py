"""Prints the measured table of tj_zone_windows (include/trajadmm.h) from tests/zone_windows_ref.py default_tolerance -- the CPU restatement on the
four end-to-end fixtures' final and iteration-0 states at the 20 measurement zones -- the constant that follows, and the largest excess by which the polynomials'
real roots (mpmath) contradict a certified class on e2e_scn_a, e2e_scn_b and tiny()'s initial states (--all: on all four end states; minutes).  No GPU.
    python tools/zone_windows_measure.py [--all]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def table(per):
    out = [" *   state                    rows   uncertain   truncated   largest live set   largest leaf list   largest depth   widest bracket"]
    for label, v in per.items():
        out.append(" *   %-24s %-6d %-11d %-11d %-18d %-19d %-15d %.2e" % ((label,) + tuple(v)))
    return "\n".join(out)


if __name__ == "__main__":
    pkg = importlib.import_module("traj-opt-admm_amd")
    import audit_ref as R
    import audit_timed_ref as T
    import zone_windows_ref as Z
    frontier, per = Z.default_tolerance(pkg)
    print(table(per))
    print("TJ_ZONEWIN_FRONTIER", frontier, "(in use: %d)" % pkg.ZONEWIN_FRONTIER)
    names = [n for n, _ in Z.E2E] if "--all" in sys.argv else ["e2e_scn_a", "e2e_scn_b"]
    states = [(n,) + T.e2e_state(n) for n in names]
    states += [("tiny_mode%d" % m, R.port_state(pkg.scenes.tiny(mode=m), 0), pkg.scenes.tiny(mode=m)["P"], 8) for m in (0, 1, 2)]
    for s in states:
        cov, inn = Z.measured_excess(pkg, [s])
        print("%s: largest excess in eps = 2^-53 of the slot's scale: coverage %.3g, IN leaves %.3g" % (s[0], cov, inn), flush=True)
