"""CPU (-m "not gpu"): the host surface of tj_zone_windows that needs no GPU -- the row's and the zone's size on both sides of the ABI, the field order, the flag
values and constants against the header, the helpers that build zones and pack them, the exported symbols, the null checks."""
import ctypes as C
import os
import re

import numpy as np

import zone_windows_ref as Z
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "trajadmm.h")).read()


def _declared(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n.strip()) for t, names in re.findall(r"\b(double|int)\s+([^;]+);", body) for n in names.split(",")]


def test_row_and_zone_size_and_fields(pkg):
    lib = pkg.load_library()
    assert lib.tj_zonewin_row_size() == C.sizeof(pkg.TjZonewinRow) == 96
    assert C.sizeof(pkg.TjZone) == 24
    assert [n for n, _ in pkg.TjZonewinRow._fields_] == list(Z.FIELDS)
    assert _declared("tj_zonewin_row") == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjZonewinRow._fields_]
    assert _declared("tj_zone") == [("double" if t is C.c_double else "int", n) for n, t in pkg.TjZone._fields_] == [
        ("double", "level"), ("int", "kind"), ("int", "sense"), ("int", "first"), ("int", "count")]


def test_flags_and_constants_are_the_headers(pkg):
    hdr = _header()
    assert pkg.ZONEWIN_FLAGS == dict(certain=Z.CERTAIN, uncertain=Z.UNCERTAIN, at_start=Z.AT_START, at_end=Z.AT_END, resolved=Z.RESOLVED, truncated=Z.TRUNCATED)
    assert pkg.ZONEWIN_FLAGS == pkg.OBSWIN_FLAGS                                               # the flags mirror tj_obstacle_windows'
    for n, v in pkg.ZONEWIN_FLAGS.items():
        assert int(re.search(r"#define TJ_ZONEWIN_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    for n, v in (("FRONTIER", pkg.ZONEWIN_FRONTIER), ("MAX_DEPTH", pkg.ZONEWIN_MAX_DEPTH), ("MAX_WINDOWS", pkg.ZONEWIN_MAX_WINDOWS), ("MAX_ZONES", pkg.ZONEWIN_MAX_ZONES),
                 ("MAX_PLANES", pkg.ZONEWIN_MAX_PLANES)):
        assert int(re.search(r"#define TJ_ZONEWIN_%s\s+(\d+)" % n, hdr).group(1)) == v
    for n, v in (("PLANES", Z.PLANES), ("BALL", Z.BALL), ("INSIDE", Z.INSIDE), ("OUTSIDE", Z.OUTSIDE)):
        assert int(re.search(r"#define TJ_ZONE_%s\s+(\d+)" % n, hdr).group(1)) == v
    assert pkg.ZONE_KINDS == dict(planes=Z.PLANES, ball=Z.BALL) == dict(planes=0, ball=1)
    assert pkg.ZONE_SENSES == dict(inside=Z.INSIDE, outside=Z.OUTSIDE) == dict(inside=0, outside=1)
    assert (pkg.ZONEWIN_MAX_DEPTH, pkg.ZONEWIN_MAX_WINDOWS, pkg.ZONEWIN_MAX_ZONES, pkg.ZONEWIN_MAX_PLANES) == (Z.MAX_DEPTH, Z.MAX_WINDOWS, Z.MAX_ZONES, Z.MAX_PLANES) == (40, 1024, 64, 32)
    assert float(re.search(r"#define TJ_ZONEWIN_TOL_FRACTION\s+(\S+)", hdr).group(1)) == pkg.ZONEWIN_TOL_FRACTION == Z.TOL_FRACTION == 0.01
    assert Z.default_tol(0.1, 2.0) == (0.01 * 0.1) / 2.0                                       # the shipped parameters
    assert re.search(r"#define TJ_ZONEWIN_MAX_BYTES\s+\(1ll << 31\)", hdr)


def test_zone_helpers_and_pack(pkg):
    kind, sense, level, rows = pkg.zone_box([1.0, 2.0, 3.0], [4.0, 5.0, 6.0])
    assert (kind, sense, level) == (Z.PLANES, Z.INSIDE, 0.0) and rows.shape == (6, 4)
    assert np.array_equal(rows, [[-1, 0, 0, -1], [1, 0, 0, 4], [0, -1, 0, -2], [0, 1, 0, 5], [0, 0, -1, -3], [0, 0, 1, 6]])
    assert np.array_equal(rows, Z.box_rows([1.0, 2.0, 3.0], [4.0, 5.0, 6.0]))
    x = np.array([2.0, 3.0, 4.0])
    assert np.all(rows[:, :3] @ x - rows[:, 3] < 0) and np.any(rows[:, :3] @ (x + 5) - rows[:, 3] > 0)      # n . x <= d inside
    ball = pkg.zone_ball([1.0, 2.0, 3.0], 0.5, "outside", -0.1)
    assert ball[:3] == (Z.BALL, Z.OUTSIDE, -0.1) and np.array_equal(ball[3], [[1.0, 2.0, 3.0, 0.5]])
    fence = pkg.zone_planes([[0.0, 0.0, 1.0, 2.0]], sense="outside", level=-0.25)
    assert fence[:3] == (Z.PLANES, Z.OUTSIDE, -0.25) and fence[3].shape == (1, 4)
    arr, table = pkg.zonewin_pack([(kind, sense, level, rows), ball, fence])
    assert [(z.kind, z.sense, z.level, z.first, z.count) for z in arr] == [(0, 0, 0.0, 0, 6), (1, 1, -0.1, 6, 1), (0, 1, -0.25, 7, 1)]
    assert table.shape == (8, 4) and table.flags["C_CONTIGUOUS"] and table.dtype == np.float64
    assert np.array_equal(table[:6], rows) and np.array_equal(table[6:7], ball[3]) and np.array_equal(table[7:], fence[3])
    arr, table = pkg.zonewin_pack([])
    assert table.shape == (0, 4)


def test_symbols_are_declared_exported_and_check_their_pointers(pkg):
    lib, hdr = pkg.load_library(), re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for s in ("tj_zone_windows", "tj_zonewin_row_size", "tj_group_zone_windows"):
        assert s in pkg.EXPORTS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hasattr(pkg.Solver, "zone_windows") and hasattr(pkg.Group, "zone_windows")
    n = C.c_int(7)
    args = (None, C.c_int(0), None, C.c_int(0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n))
    assert lib.tj_zone_windows(None, *args) == -1 and lib.tj_group_zone_windows(None, *args) == -1 and n.value == 7
