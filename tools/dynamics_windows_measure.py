"""Prints the measured table of tj_dynamics_windows (include/trajadmm.h) from tests/dynamics_windows_ref.py default_tolerance -- the CPU restatement
on the four end-to-end fixtures' final and iteration-0 states at the 18 measurement gates -- the constant that follows, and the largest excess by which the
polynomial's real roots (mpmath) contradict a certified class on e2e_scn_b and tiny()'s initial states (--all: on all four end states; minutes).  No GPU.
    python tools/dynamics_windows_measure.py [--all]"""
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
    import dynamics_windows_ref as W
    frontier, per = W.default_tolerance(pkg)
    print(table(per))
    print("TJ_DYNWIN_FRONTIER", frontier, "(in use: %d)" % pkg.DYNWIN_FRONTIER)
    names = [n for n, _ in W.E2E] if "--all" in sys.argv else ["e2e_scn_b"]
    states = [(n,) + T.e2e_state(n) for n in names]
    states += [("tiny_mode%d" % m, R.port_state(pkg.scenes.tiny(mode=m), 0), pkg.scenes.tiny(mode=m)["P"], 8) for m in (0, 1, 2)]
    cov, inn = W.measured_excess(pkg, states)
    print("largest excess in eps = 2^-53 of the depth-0 ub: coverage %.3g, IN leaves %.3g (%s)" % (cov, inn, ", ".join(s[0] for s in states)))
