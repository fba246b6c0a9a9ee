"""The batch planner (ug_plan_proof_batch, include/ultragroth_hip.h): host only, no device needed.

It gives the witnesses per device pass of a batched proof: at least 1, at most min(requested, 16), cut down by the pair limit
(V * scalars * windows <= 2^30), the bucket-id limit (< 2^31), one result block per product (<= 127 bucket sets) and the memory
of the V-fold buffers."""
import os

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


def _bytes(schedules, n_vars, domain, v):
    """the planner's memory model, restated for table schedules"""
    b = v * (n_vars + domain) * 32
    for n, c, s in schedules:
        b += v * (n * _windows(c) * PAIR_BYTES + s * (1 << (c - 1)) * BUCKET_BYTES)
    return b


def _geometry(log):
    n = (1 << log) - 1
    return [(n, 16, 1), (1 << log, 16, 1)], n, 1 << log


def test_within_bounds_and_deterministic(lib):
    sch, nv, dom = _geometry(20)
    for k in (0, 1, 2, 5, 8, 16, 17, 100):
        v = ug.plan_proof_batch(sch, nv, dom, 200 * GiB, k)
        assert 1 <= v <= min(max(k, 1), ug.BATCH_MAX), (k, v)
        assert v == ug.plan_proof_batch(sch, nv, dom, 200 * GiB, k)
    assert ug.plan_proof_batch(sch, nv, dom, 200 * GiB, 8) == 8


def test_memory_limit(lib):
    sch, nv, dom = _geometry(20)
    prev = 1
    for free in [0, 1 << 20] + [g * GiB // 4 for g in range(1, 40)]:
        v = ug.plan_proof_batch(sch, nv, dom, free, 16)
        assert v >= prev                                            # more memory never gives fewer witnesses per pass
        assert v == 1 or _bytes(sch, nv, dom, v) <= free
        assert v == 16 or _bytes(sch, nv, dom, v + 1) > free       # ... and as many as fit
        prev = v


def test_budget_for_one_witness_gives_one(lib):
    sch, nv, dom = _geometry(22)
    one = _bytes(sch, nv, dom, 1)
    assert ug.plan_proof_batch(sch, nv, dom, one, 8) == 1
    assert ug.plan_proof_batch(sch, nv, dom, 2 * one - 1, 8) == 1
    assert ug.plan_proof_batch(sch, nv, dom, 2 * one, 8) == 2


def test_pair_and_bucket_limits(lib):
    # pairs: 2^24 scalars at c = 16 (16 windows) are 2^28 pairs: four vectors reach 2^30
    assert ug.plan_proof_batch([(1 << 24, 16, 1)], 0, 0, 1 << 62, 16) == 4
    assert ug.plan_proof_batch([(1 << 26, 16, 1)], 0, 0, 1 << 62, 16) == 1
    # buckets: c = 24, stride 11 holds 11 * 2^23 per vector; 2^31 / (11 * 2^23) = 23.3 -> not binding below 16, but 2^14
    # scalars keep the pairs tiny; stride 11 over 2^14 scalars: the result block (11 sets per vector, <= 127) allows 11
    assert ug.plan_proof_batch([(1 << 14, 24, 11)], 0, 0, 1 << 62, 16) == 11
    # classic windows: one bucket set per window and vector
    v = ug.plan_proof_batch([(1 << 15, 0, 1)], 0, 0, 1 << 62, 16)
    assert 1 <= v < 16
    assert v == ug.plan_proof_batch([(1 << 15, 0, 1)], 0, 0, 1 << 62, v)


def test_request_above_the_cap_is_split(lib):
    sch, nv, dom = _geometry(18)
    left, passes = 20, []
    while left:
        v = ug.plan_proof_batch(sch, nv, dom, 200 * GiB, left)
        passes.append(v)
        left -= v
    assert passes == [16, 4]


def test_bad_arguments(lib):
    with pytest.raises(ValueError):
        ug.plan_proof_batch([(1 << 16, 15, 1)], 0, 0, GiB, 4)           # table width below 16
    with pytest.raises(ValueError):
        ug.plan_proof_batch([(1 << 16, 16, 17)], 0, 0, GiB, 4)          # stride above the windows
