"""The witness check of V witnesses in one launch (ultragroth_amd/csrc/r1cs.hip: r1cs_check_vectors_kernel through
Device.r1cs(...).check_vectors): every report and every status mask must be what ug_r1cs_check gives for that witness alone (the
single kernel) and what ug_witness_check gives on host threads (device=-1).

The circuits are built here so that every matrix meets rows of 0, 1, 4, 5 and 30 terms (30 crosses the contraction of matvec_row after
24 additions; 4 and 5 are the edges of its groups of four), the witnesses so that each has pool values of its own, among them values at
and above r and 2^256 - 1. References are computed once per witness and shared by the cases."""
import functools
import random

import pytest

import r1cs_cases as K
import ultragroth_amd as ug
from ultragroth_amd import synth

pytestmark = pytest.mark.gpu
R = K.R
LENS = (4, 0, 1, 5, 30)
POOL = 40
ROWS = (1, 255, 256, 257, 1000)          # one lane; below, at and above one block of 256; several blocks with a ragged last one
WIDTHS = (1, 2, 3, 4, 5, 8, 16)          # groups of two witnesses by default: full (2, 4, 8, 16) and partial (3, 5); one alone
KINDS = ("good", "row0", "last", "many")
PAD, FIRST = 3, 2                        # stride = n_wires + PAD, the first witness at element FIRST


@functools.lru_cache(maxsize=None)
def circuit(m):
    """(n_wires, rows, .r1cs bytes): row k has LENS[k % 5] terms in A, LENS[k // 5 % 5] in B, LENS[k // 25 % 5] in C, the last of
    C's on the row's own wire POOL + 1 + k; a row whose C is empty has an empty A"""
    rng = random.Random(0xC1C + m)

    def combination(n):
        return [(rng.randrange(0, POOL + 1), rng.choice((1, R - 1, 2, rng.randrange(R)))) for _ in range(n)]

    rows = []
    for k in range(m):
        na, nb, nc = LENS[k % 5], LENS[k // 5 % 5], LENS[k // 25 % 5]
        c = combination(max(nc - 1, 0)) + ([(POOL + 1 + k, rng.choice((1, R - 1)))] if nc else [])
        rows.append((combination(na if nc else 0), combination(nb), c))
    n = POOL + 1 + m
    return n, rows, synth.r1cs_file(n, 0, 0, rows)


@functools.lru_cache(maxsize=None)
def witness(m, v, kind):
    """witness v of circuit(m) -- its own pool values, satisfied by construction -- then broken as `kind` says"""
    n, rows, _ = circuit(m)
    rng = random.Random(0xA11CE * 1000 + m * 100 + v)
    special = [0, 1, R - 1, R, R + 5, (1 << 256) - 1]
    w = [1] + special + [rng.randrange(R) for _ in range(POOL - len(special))]
    for k, (a, b, c) in enumerate(rows):
        if not c:
            w.append(rng.randrange(R))
            continue
        rest = K.dot(c[:-1], w)
        value = (K.dot(a, w) * K.dot(b, w) - rest) * pow(c[-1][1], -1, R) % R
        w.append(value + R if rng.random() < 0.2 else value)         # sometimes the representative above r
    breakable = [k for k, row in enumerate(rows) if row[2]]
    broken = {"good": [], "row0": [0], "last": [m - 1], "many": sorted({0, m - 1} | set(rng.sample(breakable, min(3, len(breakable)))))}[kind]
    for k in broken:
        w[POOL + 1 + k] = (w[POOL + 1 + k] + 1 + v) % R
    return tuple(w), tuple(broken)


_REFERENCE = {}


def reference(device, cs, m, v, kind):
    """(failed, first, a, b, c, mask) of the witness by the single kernel, checked against the host threads' answer and the
    constraints that were broken; computed once"""
    key = (m, v, kind)
    if key not in _REFERENCE:
        w, broken = witness(m, v, kind)
        _, _, data = circuit(m)
        one = cs.check(device.dvec(len(w), b"".join(x.to_bytes(32, "little") for x in w)), want_mask=True)
        host = ug.witness_check(data, K.wtns_file(w), device=-1)
        if broken:
            assert host[:5] == (one["failed"], one["first"], one["a"], one["b"], one["c"])
            assert (one["failed"], one["first"]) == (len(broken), broken[0])
        else:
            assert host is None and one["failed"] == 0
        assert one["mask"] == bytes(1 if k in broken else 0 for k in range(m))
        _REFERENCE[key] = (one["failed"], one["first"], one["a"], one["b"], one["c"], one["mask"])
    return _REFERENCE[key]


def arrangements(V):
    bad = [KINDS[1 + v % 3] for v in range(V)]
    return {"all good": ["good"] * V, "last bad": ["good"] * (V - 1) + [bad[V - 1]], "all bad": bad}


def assert_vectors_match(device, cs, m, kinds, pad=PAD, first=FIRST):
    n = circuit(m)[0]
    V = len(kinds)
    stride = n + pad
    filler = (7).to_bytes(32, "little")
    blob = filler * first
    for v, kind in enumerate(kinds):
        blob += b"".join(x.to_bytes(32, "little") for x in witness(m, v, kind)[0]) + filler * pad
    got = cs.check_vectors(device.dvec(first + V * stride, blob), V, stride=stride, first=first, want_masks=True)
    assert len(got) == V
    for v, kind in enumerate(kinds):
        g = got[v]
        assert (g["failed"], g["first"], g["a"], g["b"], g["c"], g["mask"]) == reference(device, cs, m, v, kind), (m, V, v, kind)


@pytest.mark.parametrize("m", ROWS)
def test_every_width_and_outcome(device, m):
    cs = device.r1cs(circuit(m)[2])
    try:
        for V in WIDTHS:
            for name, kinds in arrangements(V).items():
                assert_vectors_match(device, cs, m, kinds)
        assert_vectors_match(device, cs, m, arrangements(5)["all bad"], pad=0, first=0)      # the witnesses back to back
    finally:
        cs.close()


@pytest.mark.parametrize("group", ["1", "2", "4"])
def test_every_group_size_full_and_partial(device, monkeypatch, group):
    """UG_R1CS_VT: the witnesses a lane takes. Every instantiation with full and partial groups, the same bytes from each."""
    monkeypatch.setenv("UG_R1CS_VT", group)
    m = 257
    cs = device.r1cs(circuit(m)[2])
    try:
        for V in (1, 2, 3, 4, 5, 8):
            assert_vectors_match(device, cs, m, arrangements(V)["all bad"])
            assert_vectors_match(device, cs, m, arrangements(V)["last bad"])
    finally:
        cs.close()


def test_arguments(device):
    m = 255
    n, _, data = circuit(m)
    cs = device.r1cs(data)
    try:
        vec = device.dvec(2 * n, b"".join(x.to_bytes(32, "little") for x in witness(m, 0, "good")[0] + witness(m, 1, "row0")[0]))
        assert [g["failed"] for g in cs.check_vectors(vec, 2)] == [0, 1]
        assert [g["failed"] for g in cs.check_vectors(vec, 2, stride=0, first=n)] == [1, 1]      # the same witness twice
        with pytest.raises(ug.DeviceError, match="shorter than first \\+ \\(count - 1\\) \\* stride \\+ n_wires"):
            cs.check_vectors(vec, 3)
        with pytest.raises(ug.DeviceError, match="shorter than first \\+ \\(count - 1\\) \\* stride \\+ n_wires"):
            cs.check_vectors(vec, 2, stride=n + 1)
        with pytest.raises(ug.DeviceError, match="shorter than first \\+ n_wires"):
            cs.check_vectors(vec, 1, first=n + 1)
        for count in (0, ug.BATCH_MAX + 1):
            with pytest.raises(ug.DeviceError, match="count outside 1 .. UG_BATCH_MAX"):
                cs.check_vectors(vec, count, stride=0)
        # the single check and the slots of a queued pass do not disturb each other
        assert cs.check(vec, first=n)["failed"] == 1
        assert [g["failed"] for g in cs.check_vectors(vec, 2)] == [0, 1]
    finally:
        cs.close()
