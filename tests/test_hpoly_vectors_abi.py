"""The H-polynomial block for several witnesses per call (ug_hpoly_run_vectors and its three companions), the parts that need no
GPU: the prototypes in the header, the exported symbols, the Python mirror, the documented switch and the size of the workspaces."""
import os
import re

import ultragroth_amd as ug
from ultragroth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ug_hpoly_run_vectors", "ug_hpoly_reserve_vectors", "ug_hpoly_group", "ug_hpoly_vectors_bytes")


def _header():
    return open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()


def test_symbols_are_declared_listed_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ug.load()
    inner = _header()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, inner), name
        assert name in _lib.INNER_SYMBOLS and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", inner)
    assert ("int ug_hpoly_run_vectors(ug_hpoly* hp, const ug_dvec* witness, uint64_t witness_stride, int vectors, "
            "ug_dvec* h_out, uint64_t h_stride);") in flat
    assert "int ug_hpoly_reserve_vectors(ug_hpoly* hp, int group);" in flat
    assert "int ug_hpoly_group(const ug_hpoly* hp);" in flat
    assert "uint64_t ug_hpoly_vectors_bytes(uint32_t domain_size, int group);" in flat


def test_mirror_and_switch_are_there():
    assert callable(ug.HPoly.run_vectors) and callable(ug.HPoly.reserve_vectors) and isinstance(ug.HPoly.group, property)
    assert "ULTRAGROTH_BATCH_HPOLY" in _header()
    assert b"ULTRAGROTH_BATCH_HPOLY" in open(_lib.LIB_PATH, "rb").read()
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"matvec_tiled_vectors_kernel" in blob and b"matvec_vectors_kernel" in blob and b"h_final_vectors_kernel" in blob


def test_workspace_bytes_are_linear_in_the_group():
    """a, b, c, t, t2 per vector in flight: 5 x 32 bytes x domain"""
    lib = ug.load()
    for domain in (1, 2, 1 << 7, 1 << 13, 1 << 19, 1 << 27):
        one = lib.ug_hpoly_vectors_bytes(domain, 1)
        assert one == 5 * 32 * domain
        for group in range(1, 17):
            assert lib.ug_hpoly_vectors_bytes(domain, group) == group * one == ug.hpoly_vectors_bytes(domain, group)
    assert lib.ug_hpoly_vectors_bytes(1 << 27, 16) == 16 * 5 * 32 * (1 << 27)          # (above 2^32: no 32-bit arithmetic inside)


def test_null_handles_fail_without_a_device():
    lib = ug.load()
    assert lib.ug_hpoly_run_vectors(None, None, 0, 1, None, 0) != 0 and b"null argument" in lib.ug_last_error()
    assert lib.ug_hpoly_reserve_vectors(None, 2) != 0 and b"null argument" in lib.ug_last_error()
    assert lib.ug_hpoly_group(None) == 0
