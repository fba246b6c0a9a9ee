"""The batch planner with per-witness aux bytes (ug_plan_proof_batch_aux, include/ultragroth_hip.h) and the size of a vector
lookup call (ug_lookup_vectors_bytes): host only, no device needed.

An UltraGroth pass keeps more per witness than the signal and h vectors: the gathered round / final scalars and the lookup
staging. The new entry point counts V * aux bytes on top of ug_plan_proof_batch's memory model; ug_plan_proof_batch itself
answers as before."""
import os

import numpy as np
import pytest

import ultragroth_amd as ug
from ultragroth_amd import _lib

GiB = 1 << 30
PAIR_BYTES, BUCKET_BYTES = 64, 732


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ug.load()


def _windows(c):
    return (255 + c - 1) // c


def _bytes(schedules, n_vars, domain, v, aux=0):
    """the planner's memory model for table schedules, with the aux term"""
    b = v * (n_vars + domain) * 32 + v * aux
    for n, c, s in schedules:
        b += v * (n * _windows(c) * PAIR_BYTES + s * (1 << (c - 1)) * BUCKET_BYTES)
    return b


def _ultra_geometry(log):
    """the five schedules of an UltraGroth prover: witness, round aux, final aux, H, sparse B"""
    n = (1 << log) - 1
    n1 = (n - 3) // 4
    return [(n, 16, 1), (n1, 16, 1), (n - 3 - n1, 16, 1), (1 << log, 16, 1), (n // 2, 16, 1)], n, 1 << log


def test_zero_aux_is_the_existing_planner(lib):
    for log in (16, 20, 22):
        sch, nv, dom = _ultra_geometry(log)
        for free in (0, GiB, 7 * GiB, 200 * GiB):
            for k in (1, 2, 8, 16, 20):
                assert ug.plan_proof_batch_aux(sch, nv, dom, 0, free, k) == ug.plan_proof_batch(sch, nv, dom, free, k), (log, free, k)
    # inputs tests/test_batch_plan.py pins, through both entry points
    assert ug.plan_proof_batch([(1 << 24, 16, 1)], 0, 0, 1 << 62, 16) == ug.plan_proof_batch_aux([(1 << 24, 16, 1)], 0, 0, 0, 1 << 62, 16) == 4
    assert ug.plan_proof_batch([(1 << 14, 24, 11)], 0, 0, 1 << 62, 16) == ug.plan_proof_batch_aux([(1 << 14, 24, 11)], 0, 0, 0, 1 << 62, 16) == 11


def test_aux_bytes_are_counted(lib):
    sch, nv, dom = _ultra_geometry(20)
    aux = (sch[2][0] + sch[4][0]) * 32 + (nv * 4 + (1 << 16) * 68 + (nv // 8) * 12)
    prev = 1
    for free in [0, 1 << 20] + [g * GiB // 4 for g in range(1, 60)]:
        v = ug.plan_proof_batch_aux(sch, nv, dom, aux, free, 16)
        assert v >= prev                                               # more memory never gives fewer witnesses per pass
        assert v == 1 or _bytes(sch, nv, dom, v, aux) <= free
        assert v == 16 or _bytes(sch, nv, dom, v + 1, aux) > free      # ... and as many as fit, the aux buffers included
        assert v <= ug.plan_proof_batch(sch, nv, dom, free, 16)
        prev = v
    one = _bytes(sch, nv, dom, 1, aux)
    assert ug.plan_proof_batch_aux(sch, nv, dom, aux, 2 * one - 1, 8) == 1
    assert ug.plan_proof_batch_aux(sch, nv, dom, aux, 2 * one, 8) == 2
    assert ug.plan_proof_batch(sch, nv, dom, 2 * one - 1, 8) == 2      # (the aux term is what made the difference)
    # more aux bytes never give more witnesses per pass
    free = _bytes(sch, nv, dom, 8, aux)
    vs = [ug.plan_proof_batch_aux(sch, nv, dom, a, free, 16) for a in (0, aux // 2, aux, 2 * aux, 64 * aux, 1 << 60)]
    assert vs == sorted(vs, reverse=True) and vs[2] == 8 and vs[-1] == 1


def test_request_above_the_cap_is_split(lib):
    sch, nv, dom = _ultra_geometry(15)
    left, passes = 20, []
    while left:
        v = ug.plan_proof_batch_aux(sch, nv, dom, 1 << 20, 200 * GiB, left)
        passes.append(v)
        left -= v
    assert passes == [16, 4]


def test_bad_arguments(lib):
    with pytest.raises(ValueError):
        ug.plan_proof_batch_aux([(1 << 16, 15, 1)], 0, 0, 0, GiB, 4)          # table width below 16


def test_lookup_vectors_bytes(lib):
    """staging (lists, table, challenge, descriptor) plus one u32 of scratch per element of the vector, per witness"""
    u = lambda n: np.zeros(n, dtype=np.uint32)
    a = dict(freq=u(256), chunks=u(1000), w_idx=u(700), p_idx=u(700))
    b = dict(freq=u(1 << 16), chunks=u(5), w_idx=u(3), p_idx=u(3))
    stride = 4095
    for l in (a, b):
        L, n, nc = len(l["freq"]), len(l["w_idx"]), len(l["chunks"])
        got = ug.lookup_vectors_bytes(stride, [l])
        need = 4 * stride + 4 * (L + 2 * n + nc) + 32 * (1 + 2 * L) + 32
        assert need <= got <= need + 256
    assert ug.lookup_vectors_bytes(stride, [a, b]) == ug.lookup_vectors_bytes(stride, [a]) + ug.lookup_vectors_bytes(stride, [b])
    assert ug.lookup_vectors_bytes(stride, []) == 0
