"""The witness check against a circuit's .r1cs on the device (ultragroth_amd/csrc/r1cs.hip): r1cs_check_kernel through
Device.r1cs(...).check and ug_witness_check(device=0), r1cs_match_kernel through .match. The reference is Python integers
(tests/r1cs_cases.py); the same cases run on host threads in tests/test_r1cs_host.py, and here device and host are compared."""
import struct

import pytest

import r1cs_cases as K
import ultragroth_amd as ug
from ultragroth_amd import synth

pytestmark = pytest.mark.gpu
R = K.R


def dvec_of(device, values):
    return device.dvec(len(values), b"".join(int(x).to_bytes(32, "little") for x in values))


def assert_device_matches_python(device, cs, rows, values, first=0, pad=0):
    failing, abc = K.reference(rows, values)
    got = cs.check(dvec_of(device, [7] * pad + list(values)), first=first, want_mask=True)
    assert got["mask"] == bytes(1 if k in set(failing) else 0 for k in range(len(rows)))
    assert got["failed"] == len(failing)
    if failing:
        assert (got["first"], got["a"], got["b"], got["c"]) == (failing[0],) + abc
    else:
        assert got["first"] is None and got["a"] is None


@pytest.mark.parametrize("m", K.CONSTRAINT_COUNTS)
def test_irregular_circuits(device, m):
    n, rows, good, bad, broken = K.irregular(m)
    data = synth.r1cs_file(n, 0, 0, rows)
    cs = device.r1cs(data)
    assert cs.info() == ug.r1cs_info(data)
    assert_device_matches_python(device, cs, rows, good)
    assert_device_matches_python(device, cs, rows, bad)
    assert_device_matches_python(device, cs, rows, bad, first=3, pad=3)      # the witness inside a longer vector
    with pytest.raises(ug.DeviceError, match="shorter than first \\+ n_wires"):
        cs.check(dvec_of(device, good), first=1)
    # the stand-alone call: device against host threads, both against Python
    _, abc = K.reference(rows, bad)
    on_device = ug.witness_check(data, K.wtns_file(bad), device=0)
    assert on_device == ug.witness_check(data, K.wtns_file(bad), device=-1)
    assert on_device == (len(broken), broken[0], abc[0], abc[1], abc[2], K.message(broken, m))
    assert ug.witness_check(data, K.wtns_file(good), device=0) is None
    cs.close()


def test_wrap_cases(device):
    n, rows, w = K.wrap_circuit()
    data = synth.r1cs_file(n, 0, 0, rows)
    cs = device.r1cs(data)
    assert_device_matches_python(device, cs, rows, w)
    assert ug.witness_check(data, K.wtns_file(w), device=0) is None
    for bad, failing in K.wrap_broken():
        assert_device_matches_python(device, cs, rows, bad)
        assert ug.witness_check(data, K.wtns_file(bad), device=0) == ug.witness_check(data, K.wtns_file(bad), device=-1)
    cs.close()


def test_trapdoor_circuit(device):
    mod, rows, data = K.trapdoor()
    w = K.wtns_values(K.golden("groth16.wtns"))
    cs = device.r1cs(data)
    assert_device_matches_python(device, cs, rows, w)
    w[mod.INV1] = (w[mod.INV1] + 1) % R
    assert K.reference(rows, w)[0] == [1, 429]
    assert_device_matches_python(device, cs, rows, w)
    assert ug.witness_check(data, K.wtns_file(w), device=0) == ug.witness_check(data, K.wtns_file(w), device=-1)
    cs.close()


# ---- the probe: is this .r1cs the circuit of that zkey? ----
def hpoly_of(device, zkey_name):
    mod = K.trapdoor_module()
    sec4 = dict(K.sections(K.golden(zkey_name)))[4]
    return device.hpoly(sec4[4:], struct.unpack_from("<I", sec4)[0], mod.N, mod.N_VARS)


def changed(rows, k, side, fn):
    rows = [tuple(dict(lc) for lc in row) for row in rows]
    fn(rows[k][side], rows)
    return rows


@pytest.mark.parametrize("zkey_name", ["groth16.zkey", "ultra.zkey"])
def test_match(device, zkey_name):
    mod, rows, data = K.trapdoor()
    hp = hpoly_of(device, zkey_name)
    n_pub = mod.N_PUBLIC

    def probe(r, n_public=n_pub):
        cs = device.r1cs(K.trapdoor_r1cs(r))
        try:
            return cs.match(hp, n_public)
        finally:
            cs.close()

    assert probe(rows) is None
    # one A coefficient changed
    assert probe(changed(rows, 5, 0, lambda lc, _: lc.update({mod.RHO: 2}))) == (0, 5)
    # one B term moved to the next row: rows 10 and 11 of B differ, the lower one is reported
    def move(lc, all_rows):
        wire, coef = lc.popitem()
        all_rows[11][1][wire] = (all_rows[11][1].get(wire, 0) + coef) % R
    assert probe(changed(rows, 10, 1, move)) == (1, 10)
    # one wire id changed
    def rewire(lc, _):
        lc[mod.C0 + 100] = lc.pop(mod.C0 + 19)
    assert probe(changed(rows, 20, 0, rewire)) == (0, 20)
    # the last constraint dropped: the zkey's row 429 is the lookup identity, the shorter circuit expects signal 0's public row there
    assert probe(rows[:-1]) == (0, len(rows) - 1)
    # a public count that is off by one: a public row too many in the zkey / one too few
    assert probe(rows, n_pub - 1) == (0, len(rows) + n_pub)
    assert probe(rows, n_pub + 1) == (0, len(rows) + n_pub + 1)
    # C is not in a zkey (its section 4 holds A and B only; the prover sets c = a o b itself): no probe of a zkey can see a wrong C,
    # so an .r1cs whose C differs still matches. What refuses such a file is the witness check itself: good witnesses fail under it.
    assert probe(changed(rows, 7, 2, lambda lc, _: lc.update({mod.ONE: 2}))) is None
    # sizes that cannot belong together are an error, not a verdict
    with pytest.raises(ug.DeviceError, match="not this circuit"):
        cs = device.r1cs(synth.r1cs_file(mod.N_VARS + 1, 1, 1, rows))
        cs.match(hp, n_pub)


def test_memory_returns(device):
    n, rows, good, bad, broken = K.irregular(257)
    data = synth.r1cs_file(n, 0, 0, rows)
    mod, trows, tdata = K.trapdoor()
    hp = hpoly_of(device, "groth16.zkey")

    def cycle():
        cs = device.r1cs(data)
        cs.check(dvec_of(device, bad), want_mask=True)
        cs.close()
        cs = device.r1cs(tdata)
        assert cs.match(hp, mod.N_PUBLIC) is None
        cs.close()

    cycle()                                              # (what the runtime and the context keep after a first use is there now)
    before = device.mem_info()
    cycle()
    assert device.mem_info() == before
    # a create that fails -- a wire out of range in the last constraint -- leaves nothing behind either
    broken_rows = rows[:-1] + [(rows[-1][0], rows[-1][1], {n: 1})]
    with pytest.raises(ug.DeviceError, match="constraint 256: wire %d out of range" % n):
        device.r1cs(synth.r1cs_file(n, 0, 0, broken_rows))
    assert device.mem_info() == before


# ---- provers with the circuit's .r1cs attached (fixed blinding: the process runs with ULTRAGROTH_TEST_HOOKS=1, conftest.py) ----
import hashlib      # noqa: E402
import os           # noqa: E402
import subprocess   # noqa: E402

from conftest import GOLDEN, ROOT  # noqa: E402

TD = os.path.join(GOLDEN, "trapdoor")
FAIL_1 = "witness: constraint 1 does not hold (2 of 430 fail)"      # inv1_0 changed: its own inverse constraint and the lookup identity


def _rs(b):
    return hashlib.sha256(b"r%d" % b).digest()[:31], hashlib.sha256(b"s%d" % b).digest()[:31]


def _with_blinding(data, fn):
    ug.set_test_blinding(data)
    try:
        return fn()
    finally:
        ug.set_test_blinding(b"")


def _single(p, wtns, b):
    return _with_blinding(b"".join(_rs(b)), lambda: p.prove(wtns))


def _batch(p, wtns):
    return _with_blinding(b"".join(a + b for a, b in (_rs(i) for i in range(len(wtns)))), lambda: p.prove_batch(wtns))


def _twin_witnesses(k):
    """k witnesses of the trapdoor circuit's Groth16 twin, one per challenge value, and witness 0 with inv1_0 changed"""
    mod = K.trapdoor_module()
    w1, chunks, freq = mod.first_round_witness()
    good = [mod.complete_witness(w1, chunks, freq, mod.det("r1cs test challenge %d" % b)) for b in range(k)]
    bad = list(good[0])
    bad[mod.INV1] = (bad[mod.INV1] + 1) % R
    return [K.wtns_file(w) for w in good], K.wtns_file(bad)


def test_groth16_prover_attached(device):
    mod, rows, data = K.trapdoor()
    zkey = K.golden("groth16.zkey")
    good, bad = _twin_witnesses(4)
    with ug.Groth16Prover(zkey) as plain, ug.Groth16Prover(zkey) as p:
        p.attach_r1cs(data)
        expected = [_single(plain, w, b) for b, w in enumerate(good)]
        assert _single(p, good[0], 0) == expected[0]                 # the good witness: the same bytes as without the check
        with pytest.raises(ug.ProverError) as e:
            _single(p, bad, 0)
        assert e.value.message == FAIL_1 and e.value.code == ug.PROVER_ERROR
        assert _single(p, good[1], 1) == expected[1]                 # the prover stays usable
        # the resident form
        p.load_witness(bad)
        with pytest.raises(ug.ProverError) as e:
            p.prove_resident()
        assert e.value.message == FAIL_1
        p.load_witness(good[2])
        assert _with_blinding(b"".join(_rs(2)), p.prove_resident) == expected[2]
        # batches: four good witnesses are four single proofs; one bad witness fails the call and names itself
        assert _batch(p, good) == expected
        with pytest.raises(ug.ProverError) as e:
            _batch(p, good[:2] + [bad] + good[3:])
        assert e.value.message == "witness 2: " + FAIL_1
        assert _batch(p, good) == expected
        # a proof in pieces would pass no check
        p.load_witness(good[0])
        with pytest.raises(ug.ProverError, match="not available while an .r1cs is attached"):
            load_err = ug.C.create_string_buffer(256)
            out = ug.C.create_string_buffer(ug.GROTH16_PARTIALS_SIZE)
            rc = ug.load().ug_groth16_prover_run_witness_msm(p._h, out, load_err, 255)
            if rc != ug.PROVER_OK:
                raise ug.ProverError(rc, load_err.value.decode())
        # detached, the bad witness proves again (a proof that will never verify: what the check is for)
        p.attach_r1cs(None)
        _single(p, bad, 0)


def test_attach_refuses_another_circuit(device):
    mod, rows, data = K.trapdoor()
    with ug.Groth16Prover(K.golden("groth16.zkey")) as p:
        twin = K.trapdoor_r1cs(changed(rows, 5, 0, lambda lc, _: lc.update({mod.RHO: 2})))
        with pytest.raises(ug.ProverError) as e:
            p.attach_r1cs(twin)
        assert e.value.message == "r1cs: not this circuit: matrix A row 5 differs from the zkey"
        good, bad = _twin_witnesses(1)
        _single(p, bad, 0)                                           # nothing was attached
        with pytest.raises(ug.ProverError, match="r1cs: not this circuit: nPubOut \\+ nPubIn 3, the zkey has nPublic 2"):
            p.attach_r1cs(synth.r1cs_file(mod.N_VARS, 1, 2, rows))
    with ug.UltraGrothProver(K.golden("ultra.zkey")) as p:
        twin = K.trapdoor_r1cs(changed(rows, 301, 1, lambda lc, _: lc.update({mod.INV2: 3})))
        with pytest.raises(ug.ProverError) as e:
            p.attach_r1cs(twin)
        assert e.value.message == "r1cs: not this circuit: matrix B row 301 differs from the zkey"
    zkey = synth.build_circuit(device, 10)[0]
    with ug.Groth16Prover(zkey) as p:
        with pytest.raises(ug.ProverError, match="r1cs: not this circuit: nWires 5, the zkey has nVars"):
            p.attach_r1cs(synth.r1cs_file(5, 0, 1, [({1: 1}, {2: 1}, {3: 1})]))


def test_ultra_groth_prover_attached(device):
    import json
    mod, rows, data = K.trapdoor()
    zkey, uwtns = K.golden("ultra.zkey"), K.golden("ultra.uwtns")
    vk = open(os.path.join(TD, "ultra_vkey.json")).read()
    with ug.UltraGrothProver(zkey) as p:
        p.attach_r1cs(data)
        proof, pub = p.prove(uwtns)
        assert ug.ultra_groth_verify(proof, pub, vk)
        # a round-1 signal outside the table's consistency: c_0 + 1 with `chunks` left alone. The lookup completion writes
        # inv1_0 = 1 / (chunks[0] + rho) whatever rho is drawn, so (c_0 + rho) * inv1_0 = 1 -- constraint 1 -- breaks, and only it.
        secs = K.sections(uwtns)
        values = K.wtns_values(uwtns)
        values[mod.C0] += 1
        bad = K.binfile(b"wtns", 2, [(i, b"".join(v.to_bytes(32, "little") for v in values) if i == 2 else s) for i, s in secs])
        with pytest.raises(ug.ProverError) as e:
            p.prove(bad)
        assert e.value.message == "witness: constraint 1 does not hold (1 of 430 fail)"
        with pytest.raises(ug.ProverError) as e:
            p.prove_batch([uwtns, bad])
        assert e.value.message == "witness 1: witness: constraint 1 does not hold (1 of 430 fail)"
        proof, pub = p.prove(uwtns)
        assert ug.ultra_groth_verify(proof, pub, vk)
        assert json.loads(pub)


def test_r1cs_from_the_environment(device, tmp_path, monkeypatch):
    mod, rows, data = K.trapdoor()
    good, bad = _twin_witnesses(1)
    r1cs_path = tmp_path / "circuit.r1cs"
    r1cs_path.write_bytes(data)
    (tmp_path / "good.wtns").write_bytes(good[0])
    (tmp_path / "bad.wtns").write_bytes(bad)
    prover = os.path.join(ROOT, "ultragroth_amd", "csrc", "prover")
    env = dict(os.environ, ULTRAGROTH_R1CS=str(r1cs_path))
    out = tmp_path / "good"
    out.mkdir()
    r = subprocess.run([prover, os.path.join(TD, "groth16.zkey"), str(tmp_path / "good.wtns"), str(out / "proof.json"), str(out / "public.json")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (out / "proof.json").exists()
    out = tmp_path / "bad"
    out.mkdir()
    r = subprocess.run([prover, os.path.join(TD, "groth16.zkey"), str(tmp_path / "bad.wtns"), str(out / "proof.json"), str(out / "public.json")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and FAIL_1 in r.stderr
    assert not (out / "proof.json").exists() and not (out / "public.json").exists()
    # the stand-alone tool on the same files
    tool = os.path.join(ROOT, "ultragroth_amd", "csrc", "wtns_check")
    r = subprocess.run([tool, str(r1cs_path), str(tmp_path / "good.wtns")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "witness ok: 430 constraints\n"
    r = subprocess.run([tool, str(r1cs_path), str(tmp_path / "bad.wtns")], capture_output=True, text=True, timeout=120)
    _, abc = K.reference(rows, K.wtns_values(bad))
    assert r.returncode == 1 and r.stderr == "Error: %s\nA.w = %d\nB.w = %d\nC.w = %d\n" % ((FAIL_1,) + abc)
    # in this process: the variable is read by every creation; a kind of prover that cannot check fails the creation
    zkey = K.golden("groth16.zkey")
    monkeypatch.setenv("ULTRAGROTH_R1CS", str(r1cs_path))
    with ug.Groth16Prover(zkey) as p:
        with pytest.raises(ug.ProverError) as e:
            _single(p, bad, 0)
        assert e.value.message == FAIL_1
    monkeypatch.setenv("ULTRAGROTH_DEVICES", "0")
    with pytest.raises(ug.ProverError) as e:
        ug.Groth16Prover(zkey)
    assert e.value.message == "witness check: not available on this kind of prover"
    monkeypatch.delenv("ULTRAGROTH_R1CS")
    with ug.Groth16Prover(zkey) as p:                                # a ULTRAGROTH_DEVICES handle takes no .r1cs afterwards either
        with pytest.raises(ug.ProverError) as e:
            p.attach_r1cs(data)
        assert e.value.message == "witness check: not available on this kind of prover"
    monkeypatch.setenv("ULTRAGROTH_R1CS", str(tmp_path / "missing.r1cs"))
    monkeypatch.delenv("ULTRAGROTH_DEVICES")
    with pytest.raises(ug.ProverError, match="ULTRAGROTH_R1CS: cannot read"):
        ug.Groth16Prover(zkey)


def test_attached_prover_with_recorded_launch_sequences(device, monkeypatch):
    """ULTRAGROTH_GRAPH=1: the check is queued eagerly, outside the recorded sequence -- the proofs are the same bytes, eager,
    recorded and replayed, and a bad witness still fails"""
    mod, rows, data = K.trapdoor()
    good, bad = _twin_witnesses(1)
    zkey = K.golden("groth16.zkey")
    with ug.Groth16Prover(zkey) as plain:
        expected = _single(plain, good[0], 0)
    monkeypatch.setenv("ULTRAGROTH_GRAPH", "1")
    with ug.Groth16Prover(zkey) as p:
        p.attach_r1cs(data)
        p.load_witness(good[0])
        for _ in range(3):                                           # eager, recorded + launched, replayed
            assert _with_blinding(b"".join(_rs(0)), p.prove_resident) == expected
        p.load_witness(bad)
        for _ in range(2):
            with pytest.raises(ug.ProverError) as e:
                p.prove_resident()
            assert e.value.message == FAIL_1
        p.load_witness(good[0])
        assert _with_blinding(b"".join(_rs(0)), p.prove_resident) == expected
