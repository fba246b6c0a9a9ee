"""Point validation, the parts that need no GPU: the symbols and constants the headers declare, the Python mirror, the documented
switch, and that the check kernels are part of the device code."""
import os
import re

import ultragroth_amd as ug
from ultragroth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_are_declared_listed_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ug.load()
    inner, outer = _header("ultragroth_hip.h"), _header("prover.h")
    for name in ("ug_points_check", "ug_ctx_check_points"):
        assert re.search(r"\b%s\s*\(" % name, inner) and name in _lib.INNER_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bug_zkey_check\s*\(", outer) and "ug_zkey_check" in _lib.OUTER_SYMBOLS and hasattr(lib, "ug_zkey_check")
    assert "ug_point_fault" in inner and "ug_zkey_fault" in outer


def test_constants_match_the_header():
    inner = _header("ultragroth_hip.h")
    for name in ("UG_POINT_OK", "UG_POINT_UNREDUCED", "UG_POINT_OFF_CURVE", "UG_POINT_OFF_SUBGROUP"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, inner)
        assert m and int(m.group(1)) == getattr(ug, name)
    assert (ug.UG_POINT_OK, ug.UG_POINT_UNREDUCED, ug.UG_POINT_OFF_CURVE, ug.UG_POINT_OFF_SUBGROUP) == (0, 1, 2, 3)


def test_fault_structs_have_the_c_layout():
    import ctypes as C
    assert C.sizeof(ug._PointFault) == 16 and ug._PointFault.reason.offset == 8
    assert C.sizeof(ug._ZkeyFault) == 24 and ug._ZkeyFault.index.offset == 8 and ug._ZkeyFault.reason.offset == 16


def test_mirror_and_switch_are_there():
    assert callable(ug.zkey_check) and callable(ug.Device.check_points) and callable(ug.Device.check_on_create)
    assert "ULTRAGROTH_VALIDATE" in _header("ultragroth_hip.h") and "ULTRAGROTH_VALIDATE" in _header("prover.h")
    assert "ULTRAGROTH_VALIDATE" in open(os.path.join(ROOT, "README.md")).read()
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"ULTRAGROTH_VALIDATE" in blob and b"check_g2_kernel" in blob and b"not in the subgroup of order r" in blob


def test_bad_arguments_fail_before_any_device_work():
    import ctypes as C
    lib = ug.load()
    fault = ug._ZkeyFault(7, 7, 7)
    err = C.create_string_buffer(256)
    assert lib.ug_zkey_check(None, 0, 0, 2, C.byref(fault), err, 255) == ug.PROVER_ERROR and b"Null zkey buffer" in err.value
    assert (fault.section, fault.index, fault.reason) == (0, 0, 0)
    zkey = open(os.path.join(ROOT, "tests", "golden", "circuit_final.zkey"), "rb").read()
    assert lib.ug_zkey_check(zkey, len(zkey), 0, 3, C.byref(fault), err, 255) == ug.PROVER_ERROR and b"level" in err.value
    assert lib.ug_zkey_check(zkey, 100, 0, 2, C.byref(fault), err, 255) == ug.PROVER_ERROR and fault.reason == 0
    pf = ug._PointFault()
    assert lib.ug_points_check(None, 0, zkey, 1, 1, C.byref(pf)) != 0
    assert lib.ug_ctx_check_points(None, 1) != 0
