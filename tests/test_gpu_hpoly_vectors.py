"""The H-polynomial block for V witnesses per call (include/ultragroth_hip.h: ug_hpoly_run_vectors): one matrix-vector launch per
launch group that reads every coefficient once per tile of witnesses, one launch per NTT pass over all vectors of the group.

Inner ABI: slice v of the h buffer must equal what ug_hpoly_run writes for witness v, byte for byte, whatever the launch group; the
gaps of a strided h buffer keep their contents. Prover: a batch proves the same bytes with the vector call
(ULTRAGROTH_BATCH_HPOLY=1), with one call per witness (unset, the default, and 0) and in the oracle.

Batched passes are not recorded as launch sequences today (ULTRAGROTH_GRAPH=1 covers the single-proof path only), so no run here
is recorded: the single path's recording is covered by tests/test_gpu_graph.py and queues what it queued."""
import hashlib

import pytest

import oracle as O

pytestmark = pytest.mark.gpu

WITNESSES = 16
# the smallest sizes at which each path can go wrong: the one-point branch | the smallest transform | untiled matvec, one pass |
# first tiled matvec | largest single pass | two passes with a one-stage second pass (the a.j > s0 clamp) | two passes | three
# passes (10 + 5 + 4)
DOMAINS = [0, 1, 7, 8, 10, 11, 13, 19]
_CASES = {}


def _matrix(logn, nvars):
    """44-byte coefficient records of sparse A and B: empty rows, rows of 1, 4, 5 and 30 coefficients (30 > 24: the contraction
    path), signals repeated within a row and across rows; shuffled, as a zkey's section 4 is in no row order"""
    import numpy as np
    domain = 1 << logn
    counts = np.array([0, 1, 4, 5, 30, 2, 0, 9], dtype=np.int64)
    rows = np.arange(2 * domain, dtype=np.int64)                       # row r of matrix m: rows[m * domain + r]
    m, c = rows // domain, rows % domain
    n = counts[(c * 7 + m * 3 + 4) % 8]
    if logn > 13:                                                      # keep the large matrix small: the full pattern in 8 rows of 64
        n = np.where(c % 64 < 8, n, np.where(c % 3 == 0, 1, 0))
    if domain == 1:
        n = np.array([30, 5], dtype=np.int64)
    total = int(n.sum())
    row_of = np.repeat(rows, n)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)              # position within the row
    rec = np.zeros(total, dtype=[("m", "<u4"), ("c", "<u4"), ("s", "<u4"), ("v", "V32")])
    rec["m"], rec["c"] = row_of // domain, row_of % domain
    rec["s"] = (row_of * 5 + (k % 7) * 3) % nvars                      # k and k + 7 of a row: the same signal again
    vals = np.array([O.to_le((x * x * 0x9E3779B97F4A7C15 + 1) * pow(2, 512, O.R_MOD) % O.R_MOD) for x in range(1, 18)], dtype="V32")
    rec["v"] = vals[(row_of + 3 * k) % len(vals)]
    np.random.Generator(np.random.PCG64(0xC0EF + logn)).shuffle(rec)
    return rec.tobytes(), total


def _witness(v, nvars):
    """kinds by v mod 4: all zeros | values >= r, 2^256 - 1 among them | circom-like | uniform"""
    import numpy as np
    from ultragroth_amd import synth
    kind = v % 4
    if kind == 0 and v == 0:
        return bytes(32 * nvars)
    if kind == 1:
        a = synth.scalars(nvars, "U", 900 + v).copy()
        big = [(1 << 256) - 1, O.R_MOD, O.R_MOD + 12345 + v]
        for i in range(0, nvars, 3):
            a[i] = np.frombuffer(big[(i // 3) % 3].to_bytes(32, "little"), dtype=a.dtype, count=1)[0]
        return a.tobytes()
    return synth.scalars(nvars, "C" if kind == 2 else "U", 900 + v).tobytes()


def _case(device, logn):
    """the handle of a domain, its witnesses and what ug_hpoly_run gives for each (computed once per domain, never changed)"""
    if logn not in _CASES:
        domain = 1 << logn
        nvars = 41 if logn <= 13 else 5003
        coefs, ncoefs = _matrix(logn, nvars)
        hp = device.hpoly(coefs, ncoefs, domain, nvars)
        count = WITNESSES if logn <= 13 else 5
        wt = [_witness(v, nvars) for v in range(count)]
        single = [device.download(hp.run(device.dvec(nvars, w)), 0, domain) for w in wt]
        oracle = [O.hpoly(coefs, ncoefs, w, nvars, domain) for w in wt]            # (2^19: five witnesses, about 0.5 s each)
        _CASES[logn] = dict(hp=hp, domain=domain, nvars=nvars, coefs=coefs, ncoefs=ncoefs, wt=wt, single=single, oracle=oracle)
    return _CASES[logn]


def _sentinel(n):
    return (hashlib.sha256(b"gap").digest() * n)[:32 * n]


def _run(device, case, order, group, w_gap=3, h_gap=5):
    """run_vectors over the witnesses `order` stored w_gap elements apart into an h buffer full of a sentinel pattern, slices
    h_gap apart; checks the slices against ug_hpoly_run's bytes and the gaps against the pattern"""
    hp, domain, nvars = case["hp"], case["domain"], case["nvars"]
    V = len(order)
    w_stride, h_stride = nvars + w_gap, domain + h_gap
    wv = device.dvec(V * w_stride, b"".join(case["wt"][v] + b"\xab" * (32 * w_gap) for v in order))
    fill = _sentinel(V * h_stride)
    out = device.dvec(V * h_stride, fill)
    hp.reserve_vectors(group)
    got = device.download(hp.run_vectors(wv, w_stride, V, out=out, h_stride=h_stride), 0, V * h_stride)
    assert hp.group == min(group, V)
    for j, v in enumerate(order):
        lo = 32 * j * h_stride
        assert got[lo:lo + 32 * domain] == case["single"][v], (domain, V, group, j)
        assert got[lo + 32 * domain:lo + 32 * h_stride] == fill[lo + 32 * domain:lo + 32 * h_stride], (domain, V, group, j, "gap")


@pytest.mark.parametrize("logn", DOMAINS)
def test_vectors_equal_single_runs(device, logn):
    case = _case(device, logn)
    assert case["single"] == case["oracle"]
    assert case["single"][0] == bytes(32 * case["domain"])              # (the zero witness)
    for V in ((1, 2, 3, 5, 16) if logn <= 13 else (3, 5)):       # (5: a full tile of four witnesses and a second one)
        order = list(range(V)) if V > 1 else [1]                       # (a witness with values >= r alone)
        for group in sorted({1, V}):
            _run(device, case, order, group)
    # tightly packed vectors and the default output buffer
    hp, domain, nvars = case["hp"], case["domain"], case["nvars"]
    hp.reserve_vectors(3)
    wv = device.dvec(3 * nvars, b"".join(case["wt"][v] for v in (2, 1, 0)))
    got = device.download(hp.run_vectors(wv, nvars, 3), 0, 3 * domain)
    assert [got[32 * domain * j:32 * domain * (j + 1)] for j in range(3)] == [case["single"][v] for v in (2, 1, 0)]
    # the handle is as good as new for the single call, with the large workspaces and back at one vector
    w1 = device.dvec(nvars, case["wt"][1])
    assert device.download(hp.run(w1), 0, domain) == case["single"][1]
    hp.reserve_vectors(1)
    assert device.download(hp.run(w1), 0, domain) == case["single"][1]


@pytest.mark.parametrize("logn", [0, 7, 11])
def test_launch_groups(device, logn):
    """V = 5 in groups of 2 (2, 2, 1), of 4 (one full tile of witnesses and one more launch) and of 16 (one launch, two tiles)"""
    case = _case(device, logn)
    for group in (2, 4, 16):
        _run(device, case, [4, 3, 2, 1, 0], group)
    hp = case["hp"]
    hp.reserve_vectors(16)
    _run(device, case, list(range(16))[::-1], 16, w_gap=1, h_gap=1)
    if logn:                                                           # (ug_hpoly_debug_abc re-makes c from the twisted coefficients,
        a, b, c = hp.debug_abc()                                       # which a one-point domain never forms)
        abc = O.hpoly(case["coefs"], case["ncoefs"], case["wt"][15], case["nvars"], case["domain"], want_abc=True)[1]
        n = case["domain"] * 32
        assert a == abc[:n] and b == abc[n:2 * n] and c == abc[2 * n:]      # vector 0 of the last group: witness 15
    hp.reserve_vectors(1)


def test_rejections(device):
    import ultragroth_amd as ug
    case = _case(device, 7)
    hp, domain, nvars = case["hp"], case["domain"], case["nvars"]
    L = device._L
    wv, hv = device.dvec(4 * nvars + 2), device.dvec(4 * domain + 2)

    def refused(message, *args):
        assert L.ug_hpoly_run_vectors(hp.h, *args) != 0
        assert message in L.ug_last_error(), L.ug_last_error()

    refused(b"vectors outside 1 .. UG_BATCH_MAX", wv.h, nvars, 0, hv.h, domain)
    refused(b"vectors outside 1 .. UG_BATCH_MAX", wv.h, nvars, 17, hv.h, domain)
    refused(b"witness stride below nVars", wv.h, nvars - 1, 2, hv.h, domain)
    refused(b"h stride below the domain", wv.h, nvars, 2, hv.h, domain - 1)
    refused(b"witness vector shorter than its last slice", wv.h, nvars + 1, 4, hv.h, domain)
    refused(b"h vector shorter than its last slice", wv.h, nvars, 4, hv.h, domain + 1)
    refused(b"witness vector shorter than its last slice", wv.h, nvars, 5, hv.h, domain)
    refused(b"null argument", None, nvars, 1, hv.h, domain)
    assert L.ug_hpoly_run_vectors(hp.h, wv.h, nvars, 4, hv.h, domain) == 0             # (the largest that fits both)
    for bad in (0, 17, -1):
        with pytest.raises(ug.DeviceError, match="group outside 1 .. UG_BATCH_MAX"):
            hp.reserve_vectors(bad)
    # a reservation that fails half way (test hook: with three of the five new workspaces allocated) leaves the old one in use
    hp.reserve_vectors(2)
    ug.inject_fault(ug.FAULT_HPOLY_RESERVE)
    with pytest.raises(ug.DeviceError, match="injected fault"):
        hp.reserve_vectors(16)
    _run(device, case, [3, 2, 1], 2)                                    # (reserve_vectors(2) inside is a no-op: the old workspaces)
    hp.reserve_vectors(1)


# ---- the provers ----------------------------------------------------------------------------------------------------------------
# ULTRAGROTH_BATCH_HPOLY: 1 = the vector call, 0 = one call per witness, unset = the default (off)
@pytest.mark.parametrize("b_zero", [0.0, 0.5], ids=["dense", "sparseB"])
def test_groth16_batch_with_and_without_the_vector_block(device, monkeypatch, b_zero):
    import test_gpu_batch as B
    import ultragroth_amd as ug
    zkey, wtns, exp = B._circuit(device, b_zero)
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        launches = {}
        for setting in ("1", None, "0", "1"):
            if setting is None:
                monkeypatch.delenv("ULTRAGROTH_BATCH_HPOLY", raising=False)
            else:
                monkeypatch.setenv("ULTRAGROTH_BATCH_HPOLY", setting)
            p.kernel_stats(which=2, reset=True)
            p.kernel_stats(g2=True, reset=True)
            assert B._batch(p, wtns) == exp, setting
            launches[setting] = p.kernel_stats(which=2)[1]
            passes = p.kernel_stats(g2=True)[1]                         # (one B2 launch per device pass)
        # every NTT pass of the block: one launch per device pass instead of one per witness
        k = len(wtns)
        assert launches["0"] == launches[None] and passes < k and launches["0"] % k == 0
        assert launches["1"] == passes * (launches["0"] // k), (launches, passes)
        # passes of different sizes on one prover: the larger group's workspaces serve the smaller pass
        assert B._batch(p, wtns[:2]) == exp[:2] and B._batch(p, wtns) == exp
        monkeypatch.delenv("ULTRAGROTH_BATCH_HPOLY")
        assert B._single(p, wtns[3], 3) == exp[3]


def test_ultra_groth_batch_with_and_without_the_vector_block(device, monkeypatch):
    import test_gpu_ultra_batch as U
    import ultragroth_amd as ug
    zkey, wtns, exp = U._circuit(device, 0.0)
    monkeypatch.delenv("ULTRAGROTH_OVERLAP", raising=False)
    with ug.UltraGrothProver(zkey) as p:
        for setting in ("1", None, "0", "1"):
            if setting is None:
                monkeypatch.delenv("ULTRAGROTH_BATCH_HPOLY", raising=False)
            else:
                monkeypatch.setenv("ULTRAGROTH_BATCH_HPOLY", setting)
            assert U._batch(p, wtns[:5]) == exp[:5], setting
        assert U._single(p, wtns[2], 2) == exp[2]
