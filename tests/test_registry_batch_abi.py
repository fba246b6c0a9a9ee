"""The registry's batched call and witness check, the batched witness check below them and the pass counters, the parts that need
no GPU: the exported symbols, the prototypes as plain C, and null arguments, which fail before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import ultragroth_amd as ug
from ultragroth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTER = ("ug_registry_prove_batch", "ug_registry_attach_r1cs", "ug_registry_attach_r1cs_file", "ug_registry_batch_info",
         "ug_prover_batch_info")
INNER = ("ug_r1cs_check_vectors_enqueue", "ug_r1cs_check_vectors")


def _lib_handle():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ug.load()


def test_symbols_are_declared_listed_and_exported():
    lib = _lib_handle()
    outer = open(os.path.join(ROOT, "include", "prover.h")).read()
    inner = open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()
    for name in OUTER:
        assert re.search(r"\bint %s\s*\(" % name, outer), name
        assert name in _lib.OUTER_SYMBOLS and hasattr(lib, name), name
    for name in INNER:
        assert re.search(r"\bint\s+%s\s*\(" % name, inner), name
        assert name in _lib.INNER_SYMBOLS and hasattr(lib, name), name
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"r1cs_check_vectors_kernel" in blob
    assert "UG_R1CS_VT" in inner and b"UG_R1CS_VT" in blob
    for cls, names in ((ug.Registry, ("prove_batch", "attach_r1cs", "batch_info")), (ug.Groth16Prover, ("batch_info",)),
                       (ug.UltraGrothProver, ("batch_info",)), (ug._R1cs, ("check_vectors",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_the_lists_of_unbatched_and_unchecked_handles_no_longer_name_the_registry():
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "prover.h")).read())
    assert "ULTRAGROTH_DEVICES provers of either protocol, sharded ranks." in flat
    assert "a sharded or ULTRAGROTH_DEVICES handle" in flat
    assert "registry circuits" not in flat and "or registry handle" not in flat


def test_prototypes_compile_as_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = """
#include "prover.h"
#include "ultragroth_hip.h"
int use(void *reg, void *prover, ug_r1cs *r, const ug_dvec *w, ug_ctx *via) {
    const void *wt[1] = {0}; unsigned long long ws[1] = {0}, ps[1] = {0}, qs[1] = {0}, passes = 0, witnesses = 0;
    char *pb[1] = {0}, *qb[1] = {0}, err[8];
    int width = 0;
    ug_r1cs_report reports[2];
    unsigned char masks[2];
    return ug_registry_prove_batch(reg, "c", 1, wt, ws, pb, ps, qb, qs, err, 7)
         + ug_registry_attach_r1cs(reg, "c", wt[0], 0, err, 7) + ug_registry_attach_r1cs_file(reg, "c", "c.r1cs", err, 7)
         + ug_registry_batch_info(reg, "c", &passes, &witnesses, &width) + ug_prover_batch_info(prover, &passes, &witnesses, &width)
         + ug_r1cs_check_vectors_enqueue(r, w, 0, 1, 2, 0, via) + ug_r1cs_check_vectors(r, w, 0, 1, 2, reports, masks);
}
"""
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_fail_without_a_device():
    lib = _lib_handle()
    err = C.create_string_buffer(256)
    one = (C.c_void_p * 1)()
    sizes = (C.c_ulonglong * 1)(0)
    assert lib.ug_registry_prove_batch(None, b"c", 1, one, sizes, one, sizes, one, sizes, err, 255) == ug.PROVER_ERROR
    assert err.value == b"Null registry object"
    assert lib.ug_registry_attach_r1cs(None, b"c", b"x", 1, err, 255) == ug.PROVER_ERROR and err.value == b"Null registry object"
    assert lib.ug_registry_attach_r1cs_file(None, b"c", b"x", err, 255) == ug.PROVER_ERROR and err.value == b"Null registry object"
    fake = C.c_void_p(1)                                             # never dereferenced: the arguments are looked at first
    assert lib.ug_registry_prove_batch(fake, None, 0, None, None, None, None, None, None, err, 255) == ug.PROVER_ERROR
    assert err.value == b"Null circuit name"
    assert lib.ug_registry_prove_batch(fake, b"c", 1, None, sizes, one, sizes, one, sizes, err, 255) == ug.PROVER_ERROR
    assert err.value == b"Null batch argument"
    assert lib.ug_registry_prove_batch(fake, b"c", 1, one, sizes, one, sizes, one, sizes, err, 255) == ug.PROVER_ERROR
    assert err.value == b"Null buffer of witness 0"
    assert lib.ug_registry_prove_batch(fake, b"c", -1, one, sizes, one, sizes, one, sizes, err, 255) == ug.PROVER_ERROR
    assert err.value == b"Negative witness count"
    assert lib.ug_registry_attach_r1cs(fake, None, b"x", 1, err, 255) == ug.PROVER_ERROR and err.value == b"Null circuit name"
    assert lib.ug_registry_attach_r1cs(fake, b"c", None, 1, err, 255) == ug.PROVER_ERROR and err.value == b"Null r1cs buffer"
    assert lib.ug_registry_attach_r1cs_file(fake, b"c", None, err, 255) == ug.PROVER_ERROR and err.value == b"Null r1cs path"
    assert lib.ug_registry_batch_info(None, b"c", None, None, None) == ug.PROVER_ERROR
    assert lib.ug_registry_batch_info(fake, None, None, None, None) == ug.PROVER_ERROR
    assert lib.ug_prover_batch_info(None, None, None, None) == ug.PROVER_ERROR
    assert lib.ug_r1cs_check_vectors_enqueue(None, None, 0, 0, 1, 0, None) != 0 and b"null argument" in lib.ug_last_error()
    assert lib.ug_r1cs_check_vectors(None, None, 0, 0, 1, None, None) != 0 and b"null argument" in lib.ug_last_error()
