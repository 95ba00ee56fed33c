"""CPU (-m "not gpu"): the host surface of tj_proximity_windows that needs no GPU -- the row's size on both sides of the ABI, the flag values and constants against
the header, the exported symbols, the null checks."""
import ctypes as C
import os
import re

import proximity_ref as X
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "trajadmm.h")).read()


def test_row_size_and_fields(pkg):
    lib = pkg.load_library()
    assert lib.tj_proximity_row_size() == C.sizeof(pkg.TjProximityRow) == 80
    assert [n for n, _ in pkg.TjProximityRow._fields_] == list(X.FIELDS)
    body = re.search(r"typedef struct tj_proximity_row \{(.*?)\} tj_proximity_row;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [(t, n.strip()) for t, names in re.findall(r"\b(double|int)\s+([^;]+);", body) for n in names.split(",")]
    assert declared == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjProximityRow._fields_]


def test_flags_and_constants_are_the_headers(pkg):
    hdr = _header()
    assert pkg.PROXIMITY_FLAGS == dict(certain=X.CERTAIN, uncertain=X.UNCERTAIN, at_start=X.AT_START, at_end=X.AT_END, resolved=X.RESOLVED, truncated=X.TRUNCATED)
    for n, v in pkg.PROXIMITY_FLAGS.items():
        assert int(re.search(r"#define TJ_PROXIMITY_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    for n, v in (("FRONTIER", pkg.PROXIMITY_FRONTIER), ("MAX_DEPTH", pkg.PROXIMITY_MAX_DEPTH), ("MAX_WINDOWS", pkg.PROXIMITY_MAX_WINDOWS)):
        assert int(re.search(r"#define TJ_PROXIMITY_%s\s+(\d+)" % n, hdr).group(1)) == v
    assert float(re.search(r"#define TJ_PROXIMITY_TOL_FRACTION\s+(\S+)", hdr).group(1)) == pkg.PROXIMITY_TOL_FRACTION == X.TOL_FRACTION


def test_symbols_are_declared_exported_and_check_their_pointers(pkg):
    lib, hdr = pkg.load_library(), re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for s in ("tj_proximity_windows", "tj_proximity_row_size", "tj_group_proximity_windows"):
        assert s in pkg.EXPORTS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg.Solver, "proximity_windows") and hasattr(pkg.Group, "proximity_windows")
    pairs, n = C.c_int(7), C.c_int(7)
    args = (C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(pairs), C.byref(n))
    assert lib.tj_proximity_windows(None, *args) == -1 and lib.tj_group_proximity_windows(None, *args) == -1 and (pairs.value, n.value) == (7, 7)
