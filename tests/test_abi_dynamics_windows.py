"""CPU (-m "not gpu"): the host surface of tj_dynamics_windows that needs no GPU -- the row's and the gate's size on both sides of the ABI, the field order, the
flag values and constants against the header, the exported symbols, the null checks."""
import ctypes as C
import os
import re

import dynamics_windows_ref as W
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "trajadmm.h")).read()


def _declared(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n.strip()) for t, names in re.findall(r"\b(double|int)\s+([^;]+);", body) for n in names.split(",")]


def test_row_and_gate_size_and_fields(pkg):
    lib = pkg.load_library()
    assert lib.tj_dynwin_row_size() == C.sizeof(pkg.TjDynwinRow) == 96
    assert C.sizeof(pkg.TjDynGate) == 16
    assert [n for n, _ in pkg.TjDynwinRow._fields_] == list(W.FIELDS)
    assert _declared("tj_dynwin_row") == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjDynwinRow._fields_]
    assert _declared("tj_dyn_gate") == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjDynGate._fields_] == [("double", "level"), ("int", "quantity"), ("int", "sense")]


def test_flags_and_constants_are_the_headers(pkg):
    hdr = _header()
    assert pkg.DYNWIN_FLAGS == dict(certain=W.CERTAIN, uncertain=W.UNCERTAIN, at_start=W.AT_START, at_end=W.AT_END, resolved=W.RESOLVED, truncated=W.TRUNCATED)
    assert pkg.DYNWIN_FLAGS == pkg.OBSWIN_FLAGS                                                # the flags mirror tj_obstacle_windows'
    for n, v in pkg.DYNWIN_FLAGS.items():
        assert int(re.search(r"#define TJ_DYNWIN_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    for n, v in (("FRONTIER", pkg.DYNWIN_FRONTIER), ("MAX_DEPTH", pkg.DYNWIN_MAX_DEPTH), ("MAX_WINDOWS", pkg.DYNWIN_MAX_WINDOWS), ("MAX_GATES", pkg.DYNWIN_MAX_GATES),
                 ("SPEED", W.SPEED), ("ACCEL", W.ACCEL), ("JERK", W.JERK), ("ABOVE", W.ABOVE), ("BELOW", W.BELOW)):
        assert int(re.search(r"#define TJ_DYNWIN_%s\s+(\d+)" % n, hdr).group(1)) == v
    assert pkg.DYNWIN_QUANTITIES == dict(speed=W.SPEED, accel=W.ACCEL, jerk=W.JERK) == dict(speed=0, accel=1, jerk=2)
    assert pkg.DYNWIN_SENSES == dict(above=W.ABOVE, below=W.BELOW) == dict(above=0, below=1)
    assert (pkg.DYNWIN_MAX_DEPTH, pkg.DYNWIN_MAX_WINDOWS, pkg.DYNWIN_MAX_GATES) == (W.MAX_DEPTH, W.MAX_WINDOWS, W.MAX_GATES) == (40, 1024, 16)
    assert float(re.search(r"#define TJ_DYNWIN_TOL_FRACTION\s+(\S+)", hdr).group(1)) == pkg.DYNWIN_TOL_FRACTION == W.TOL_FRACTION == 0.01
    assert W.default_tol(2.0, 2.0) == 0.01                                                    # the shipped parameters
    assert re.search(r"#define TJ_DYNWIN_MAX_BYTES\s+\(1ll << 31\)", hdr)


def test_gates_by_name_or_number(pkg):
    assert pkg.dynwin_gates([("speed", "above", 2), (1, 1, 0.5), ("jerk", 0, 3.0)]) == [(0, 0, 2.0), (1, 1, 0.5), (2, 0, 3.0)]
    assert pkg.dynwin_gates([]) == []
    assert W.default_gates(2.0, 3.0) == [(W.SPEED, W.ABOVE, 2.0), (W.ACCEL, W.ABOVE, 3.0)]


def test_symbols_are_declared_exported_and_check_their_pointers(pkg):
    lib, hdr = pkg.load_library(), re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for s in ("tj_dynamics_windows", "tj_dynwin_row_size", "tj_group_dynamics_windows"):
        assert s in pkg.EXPORTS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg.Solver, "dynamics_windows") and hasattr(pkg.Group, "dynamics_windows")
    n = C.c_int(7)
    args = (None, C.c_int(0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n))
    assert lib.tj_dynamics_windows(None, *args) == -1 and lib.tj_group_dynamics_windows(None, *args) == -1 and n.value == 7
