"""CPU: the audit query's ABI surface -- both libraries export it, the ctypes mirror of tj_audit_robot has the C record's size,
and include/trajadmm.h declares what the package lists."""
import ctypes as C
import os
import re

from conftest import ROOT

AUDIT = ("tj_audit", "tj_group_audit", "tj_audit_record_size")


def test_both_libraries_export_the_audit(pkg):
    for path in (pkg.LIB_PATH, pkg.KAT_LIB_PATH):
        assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
        lib = C.CDLL(path)
        for name in AUDIT:
            assert hasattr(lib, name), f"{name} not exported by {os.path.basename(path)}"
            assert name in pkg.EXPORTS


def test_record_size_equals_the_ctypes_mirror(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    assert lib.tj_audit_record_size() == C.sizeof(pkg.TjAuditRobot) == 72
    # no implicit padding: the fields are laid out back to back in the header's order
    off = 0
    for name, t in pkg.TjAuditRobot._fields_:
        assert getattr(pkg.TjAuditRobot, name).offset == off, name
        off += C.sizeof(t)


def test_header_declares_the_record_and_the_calls(pkg):
    txt = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in AUDIT:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared in include/trajadmm.h"
    m = re.search(r"typedef struct tj_audit_robot \{(.*?)\} tj_audit_robot;", code, flags=re.S)
    assert m, "tj_audit_robot not declared"
    fields = [f for decl in m.group(1).split(";") for f in re.sub(r"^\s*(double|int)\s+", "", decl.strip()).replace(" ", "").split(",") if f]
    assert fields == [n for n, _ in pkg.TjAuditRobot._fields_]
    flags = dict(re.findall(r"TJ_AUDIT_([A-Z_]+)\s*=\s*(\d+)", code))
    assert {k.lower(): int(v) for k, v in flags.items()} == pkg.AUDIT_FLAGS
