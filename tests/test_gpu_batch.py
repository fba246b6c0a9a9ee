"""Batched Groth16 proofs: V scalar vectors in one schedule (include/ultragroth_hip.h: ug_schedule_build_vectors) and
ug_groth16_prover_prove_batch on top of it.

Inner ABI: every record of a product over a V-vector schedule must equal the product over a single-vector schedule of that
vector. Prover: every batch proof must equal the oracle's proof for its witness and its blinding (r_b, s_b), byte for byte."""
import threading

import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SEED_A, SEED_B, SEED_C, SEED_G2 = 0x2234_0001, 0x2234_0003, 0x2234_0005, 0x2234_0007
N = (1 << 15) + 123


def _vector_scalars(v, n):
    """vector 0: zeros (every product is infinity), 1: circom-like (heavy buckets), 2: scalars >= r, others uniform"""
    import numpy as np
    from ultragroth_amd import synth
    if v == 0:
        return bytes(32 * n)
    if v == 1:
        return synth.scalars(n, "C", 501).tobytes()
    if v == 2:
        a = synth.scalars(n, "U", 502).copy()
        big = [O.R_MOD, O.R_MOD + 12345, (1 << 256) - 1]
        for i in range(0, n, 7):
            a[i] = np.frombuffer(big[(i // 7) % 3].to_bytes(32, "little"), dtype=a.dtype, count=1)[0]
        return a.tobytes()
    return synth.scalars(n, "U", 500 + v).tobytes()


@pytest.fixture(scope="module")
def pts(device):
    from ultragroth_amd import synth
    return {"A": bytes(synth.synth_points(device, N, SEED_A)), "B": bytes(synth.synth_points(device, N, SEED_B)),
            "C": bytes(synth.synth_points(device, N, SEED_C)), "G2": bytes(synth.synth_points(device, N, SEED_G2, g2=True))}


# (c = 20 and 22 take the first sort pass's instantiations with the window width as a constant: 13 and 12 windows per scalar)
@pytest.mark.parametrize("mode", [(0, 1), (16, 1), (16, 2), (16, 3), (20, 1), (22, 2)], ids=["classic", "full", "s2", "s3", "c20", "c22s2"])
def test_vector_schedule_matches_single_vectors(device, pts, mode):
    """V = 1, 3, 5 over count = 2^15 + 123 scalars (stored with a gap between the vectors): a G1 set, a G2 set and a 3-member
    group with a C shift; record v equals the product over a single-vector schedule of vector v"""
    c, s = mode
    n, shift, gap = N, 5, 77
    g1 = device.bases(pts["A"], n, table_c=c, table_stride=s)
    g2 = device.bases(pts["G2"], n, g2=True, table_c=c, table_stride=s)
    grp = device.bases_group([(pts["A"], n, 0), (pts["B"], n, 0), (pts["C"][:64 * (n - shift)], n - shift, shift)], 0, n,
                             table_c=c, table_stride=s)
    vecs = [_vector_scalars(v, n) for v in range(5)]
    single = []
    for sc in vecs:
        sch = device.schedule(device.dvec(n, sc), 0, n, table_c=c, table_stride=s)
        single.append((device.msm(g1, sch), device.msm(g2, sch, g2=True), device.msm_group(grp, sch)))
    assert single[0][0] == bytes(64) and single[0][1] == bytes(128)
    stride = n + gap
    for V in (1, 3, 5):
        order = list(range(V))[::-1] if V > 1 else [1]         # (the zero vector is not always first)
        data = b"".join(vecs[v] + bytes(32 * gap) for v in order)
        dv = device.dvec(stride * V, data)
        sch = device.schedule_vectors(dv, 0, n, V, stride, table_c=c, table_stride=s)
        r1, r2, rg = device.msm(g1, sch), device.msm(g2, sch, g2=True), device.msm_group(grp, sch)
        rb = device.msm_batch([(g1, False), (g2, True)], sch)
        for j, v in enumerate(order):
            assert r1[64 * j:64 * (j + 1)] == single[v][0], (mode, V, v)
            assert r2[128 * j:128 * (j + 1)] == single[v][1], (mode, V, v)
            assert rb[0][64 * j:64 * (j + 1)] == single[v][0] and rb[1][128 * j:128 * (j + 1)] == single[v][1], (mode, V, v)
            assert [m[64 * j:64 * (j + 1)] for m in rg] == list(single[v][2]), (mode, V, v)


def test_vector_schedule_against_the_walk(device, pts):
    """one record against the closed form of the generator walk, and the gather at an offset"""
    import numpy as np
    from ultragroth_amd import synth
    n = N
    sc = _vector_scalars(3, n)
    exp = O.g1_mul(synth.g1_generator_record(), O.fr_dot_walk(sc, n, SEED_A))
    src = device.dvec(n, sc)
    out = device.dvec(2 * n, bytes(64 * n))
    device.gather_index_at(out, n, src, np.arange(n, dtype=np.uint32))     # vector 1 = the scalars, vector 0 = zeros
    sch = device.schedule_vectors(out, 0, n, 2, n, table_c=16)
    got = device.msm(device.bases(pts["A"], n, table_c=16), sch)
    assert got[:64] == bytes(64) and got[64:] == exp


def test_vector_schedule_rejections(device, pts):
    import ultragroth_amd as ug
    n = 1 << 14
    dv = device.dvec(4 * n, bytes(32 * 4 * n))
    for bad in ((0, n), (17, n), (2, n - 1), (5, n)):
        with pytest.raises(ug.DeviceError):
            device.schedule_vectors(dv, 0, n, bad[0], bad[1])
    h = device.schedule(dv, 0, n, table_c=16, classes=(3, 0, 8, 0, 0, 0))
    assert device._L.ug_schedule_build_vectors(h.h, dv.h, 0, n, 2, n, 16, 1) != 0
    assert b"bucket classes" in device._L.ug_last_error()


# ---- the prover -------------------------------------------------------------------------------------------------------------
LOG = 15
_CIRCUITS = {}


def _rs(b):
    import hashlib
    return hashlib.sha256(b"r%d" % b).digest()[:31], hashlib.sha256(b"s%d" % b).digest()[:31]


def _circuit(device, b_zero, k=5):
    """zkey, k witnesses (mixed U / C), and the oracle's proof of witness b with blinding _rs(b)"""
    from ultragroth_amd import synth
    key = b_zero
    if key not in _CIRCUITS:
        zkey, _, _ = synth.build_circuit(device, LOG, mix="U", b_zero=b_zero)
        wtns = [synth.build_witness(LOG, "UC"[b % 2], seed=0x7000 + 16 * b) for b in range(k)]
        exp = []
        for b, w in enumerate(wtns):
            r, s = _rs(b)
            e = O.groth16_prove(zkey, w, int.from_bytes(r, "little"), int.from_bytes(s, "little"))
            exp.append((e[0], e[1]))
        _CIRCUITS[key] = (zkey, wtns, exp)
    return _CIRCUITS[key]


def _batch(p, wtns, first=0):
    import ultragroth_amd as ug
    ug.set_test_blinding(b"".join(a + b for a, b in (_rs(first + i) for i in range(len(wtns)))))
    try:
        return p.prove_batch(wtns)
    finally:
        ug.set_test_blinding(b"")


def _single(p, wtns, b):
    import ultragroth_amd as ug
    r, s = _rs(b)
    ug.set_test_blinding(r + s)
    try:
        return p.prove(wtns)
    finally:
        ug.set_test_blinding(b"")


@pytest.mark.parametrize("b_zero", [0.0, 0.5], ids=["dense", "sparseB"])
@pytest.mark.parametrize("tables", ["off", "on", "strided"])
def test_batch_prover_against_the_oracle(device, monkeypatch, b_zero, tables):
    import ultragroth_amd as ug
    zkey, wtns, exp = _circuit(device, b_zero)
    monkeypatch.delenv("ULTRAGROTH_TABLES_BUDGET", raising=False)
    monkeypatch.setenv("ULTRAGROTH_TABLES", "0" if tables == "off" else "1")
    if tables == "strided":
        with ug.Groth16Prover(zkey) as p:
            p.tables_ready(wait=True)
            full = p.table_plan()
        budget = min(b for _, _, b, _ in full if b) // 2
        monkeypatch.setenv("ULTRAGROTH_TABLES_BUDGET", "%.9f" % (budget / (1 << 30)))
    with ug.Groth16Prover(zkey) as p:
        if tables == "strided":
            assert any(c and st > 1 for c, st, _, _ in p.table_plan()), p.table_plan()
        for k in (1, 2, 5):                                     # (background tables: the first calls may run before them)
            assert _batch(p, wtns[:k]) == exp[:k], (tables, k)
        p.tables_ready(wait=True)
        p.kernel_stats(g2=True, reset=True)
        assert _batch(p, wtns) == exp
        assert p.kernel_stats(g2=True)[1] < len(wtns)           # several witnesses per device pass (one B2 launch per pass)
        for overlap in ("0", "1"):
            monkeypatch.setenv("ULTRAGROTH_OVERLAP", overlap)
            assert _batch(p, wtns) == exp, (tables, overlap)
        assert _single(p, wtns[3], 3) == exp[3]                 # the single path afterwards


def test_batch_split_into_passes(device):
    """k = 20 is above the cap of 16: split into passes, every proof equals the single proof with its blinding"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zkey, _, _ = _circuit(device, 0.0)
    wtns = [synth.build_witness(LOG, "UC"[b % 2], seed=0x9000 + 16 * b) for b in range(20)]
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        got = _batch(p, wtns)
        assert [_single(p, w, b) for b, w in enumerate(wtns)] == got


def test_batch_errors(device):
    import ultragroth_amd as ug
    zkey, wtns, exp = _circuit(device, 0.0)
    with ug.Groth16Prover(zkey) as p:
        from ultragroth_amd import synth
        bad = list(wtns[:4])
        bad[2] = synth.build_witness(LOG - 1, "U", seed=0x7100)          # a witness with fewer signals than the circuit
        with pytest.raises(ug.ProverError) as e:
            _batch(p, bad)
        assert e.value.code == ug.PROVER_INVALID_WITNESS_LENGTH and e.value.message.startswith("witness 2: Invalid witness length")
        bad[2] = wtns[2][:-32 * 100]                                     # cut short: the code and message of a single prove
        with pytest.raises(ug.ProverError) as single:
            p.prove(bad[2])
        with pytest.raises(ug.ProverError) as e:
            _batch(p, bad)
        assert e.value.code == single.value.code and e.value.message == "witness 2: " + single.value.message
        assert _batch(p, wtns[:2]) == exp[:2]
        with pytest.raises(ug.ProverError) as e:
            p.prove_batch(wtns[:3], proof_size=100)
        assert e.value.code == ug.PROVER_ERROR_SHORT_BUFFER
        assert all(sz >= 810 for sz in e.value.proof_sizes)
        assert _single(p, wtns[1], 1) == exp[1]


def test_batch_beside_a_concurrent_prove(device):
    import ultragroth_amd as ug
    zkey, wtns, exp = _circuit(device, 0.0)
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        ug.set_test_blinding(b"".join(a + b for a, b in (_rs(4) for _ in range(8))))     # every draw gives r4 or s4
        try:
            out = {}
            t = threading.Thread(target=lambda: out.__setitem__("single", [p.prove(wtns[4]) for _ in range(3)]))
            t.start()
            out["batch"] = p.prove_batch([wtns[4]] * 4)
            t.join()
        finally:
            ug.set_test_blinding(b"")
        assert out["batch"] == [exp[4]] * 4 and out["single"] == [exp[4]] * 3


def test_batch_at_2_22(device):
    """a batch of 8 equals 8 single proofs byte for byte"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zkey, _, _ = synth.build_circuit(device, 22, mix="U")
    wtns = [synth.build_witness(22, "UC"[b % 2], seed=0xA000 + 16 * b) for b in range(8)]
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        p.kernel_stats(g2=True, reset=True)
        got = _batch(p, wtns)
        assert p.kernel_stats(g2=True)[1] == 1                  # ONE device pass: one G2 accumulation launch for all eight
        assert [_single(p, w, b) for b, w in enumerate(wtns)] == got


def test_batch_on_other_handles(device, monkeypatch):
    """UltraGroth and ULTRAGROTH_DEVICES handles accept the call and prove one after the other"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zkey, uwtns, _ = synth.build_ultra_circuit(device, 15)
    rk, r, s = bytes(range(1, 32)), bytes(range(40, 71)), bytes(range(80, 111))
    with ug.UltraGrothProver(zkey) as p:
        ug.set_test_blinding(rk + r + s)
        try:
            assert p.prove_batch([uwtns, uwtns]) == [p.prove(uwtns)] * 2
        finally:
            ug.set_test_blinding(b"")
    zkey, wtns, exp = _circuit(device, 0.0)
    monkeypatch.setenv("ULTRAGROTH_DEVICES", "0,0")
    with ug.Groth16Prover(zkey) as p:
        assert _batch(p, wtns[:3]) == exp[:3]
