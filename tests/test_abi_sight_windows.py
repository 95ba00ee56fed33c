"""CPU (-m "not gpu"): the host surface of tj_sight_windows that needs no GPU -- the row's size on both sides of the ABI, the field order, the flag values and
constants against the header, the exported symbols, the null checks."""
import ctypes as C
import os
import re

import sight_windows_ref as W
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "trajadmm.h")).read()


def test_row_size_and_fields(pkg):
    lib = pkg.load_library()
    assert lib.tj_sight_row_size() == C.sizeof(pkg.TjSightRow) == 88
    assert [n for n, _ in pkg.TjSightRow._fields_] == list(W.FIELDS)
    body = re.search(r"typedef struct tj_sight_row \{(.*?)\} tj_sight_row;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [(t, n.strip()) for t, names in re.findall(r"\b(double|int)\s+([^;]+);", body) for n in names.split(",")]
    assert declared == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjSightRow._fields_]


def test_flags_and_constants_are_the_headers(pkg):
    hdr = _header()
    assert pkg.SIGHT_FLAGS == dict(certain=W.CERTAIN, uncertain=W.UNCERTAIN, at_start=W.AT_START, at_end=W.AT_END, resolved=W.RESOLVED, truncated=W.TRUNCATED)
    assert pkg.SIGHT_FLAGS == pkg.OBSWIN_FLAGS                                                # the flags mirror tj_obstacle_windows'
    for n, v in pkg.SIGHT_FLAGS.items():
        assert int(re.search(r"#define TJ_SIGHT_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    for n, v in (("FRONTIER", pkg.SIGHT_FRONTIER), ("MAX_DEPTH", pkg.SIGHT_MAX_DEPTH), ("MAX_WINDOWS", pkg.SIGHT_MAX_WINDOWS), ("PROJECTIONS", pkg.SIGHT_PROJECTIONS)):
        assert int(re.search(r"#define TJ_SIGHT_%s\s+(\d+)" % n, hdr).group(1)) == v
    assert (pkg.SIGHT_MAX_DEPTH, pkg.SIGHT_MAX_WINDOWS) == (W.MAX_DEPTH, W.MAX_WINDOWS) == (40, 1024)
    assert float(re.search(r"#define TJ_SIGHT_TOL_FRACTION\s+(\S+)", hdr).group(1)) == pkg.SIGHT_TOL_FRACTION == W.TOL_FRACTION == 0.01
    assert re.search(r"#define TJ_SIGHT_MAX_BYTES\s+\(1ll << 31\)", hdr)


def test_default_links(pkg):
    assert pkg.sight_links(3, 2) == W.default_links(3, 2) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (0, -1), (0, -2), (1, -1), (1, -2), (2, -1), (2, -2)]
    assert pkg.sight_links(1, 1) == [(0, -1)] and pkg.sight_links(1, 0) == []


def test_symbols_are_declared_exported_and_check_their_pointers(pkg):
    lib, hdr = pkg.load_library(), re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for s in ("tj_sight_windows", "tj_sight_row_size", "tj_group_sight_windows"):
        assert s in pkg.EXPORTS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg.Solver, "sight_windows") and hasattr(pkg.Group, "sight_windows")
    n = C.c_int(7)
    links = (C.c_int * 2)(0, 1)
    args = (links, C.c_int(1), None, C.c_int(0), C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n))
    assert lib.tj_sight_windows(None, *args) == -1 and lib.tj_group_sight_windows(None, *args) == -1 and n.value == 7
