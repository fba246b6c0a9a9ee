"""The phase-2 setup from a prepared powers-of-tau file on host threads (device = -1): include/ultragroth_hip.h
ug_ptau_parse_info, ug_setup_ptau_*, ug_points_combine, ug_points_scale through ultragroth_amd.ptau_info / setup_from_ptau /
points_combine / points_scale, and the test writer synth.ptau_file. Every comparison is byte for byte: a .ptau synthesized from
the fixture's (tau, alpha, beta) must give the key dev_setup gives for the trapdoor (tau, alpha, beta, gamma = 1, delta)."""
import json
import os
import struct
import subprocess

import pytest

import oracle as O
from oracle import pairing
from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = SC.R
FIXED_DELTA = PC.FIXED_DELTA


def _ug():
    import ultragroth_amd as ug
    return ug


def _refused(fn, text):
    ug = _ug()
    with pytest.raises(ug.SetupError) as e:
        fn()
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------- writer and reader
def test_ptau_info_of_a_synthesized_file(tmp_path):
    ug = _ug()
    assert ug.ptau_info(PC.ptau(6)) == {"power": 6, "ceremony_power": 6, "prepared": True, "max_log_domain": 6}
    assert ug.ptau_info(PC.ptau(6, prepared=False)) == {"power": 6, "ceremony_power": 6, "prepared": False, "max_log_domain": 0}
    ids = [i for i, _ in RC.sections(PC.ptau(6))]
    assert ids == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    sizes = dict((i, len(p)) for i, p in RC.sections(PC.ptau(6)))
    assert sizes[2] == 64 * 127 and sizes[3] == 128 * 64 and sizes[4] == sizes[5] == 64 * 64 and sizes[6] == 128
    assert sizes[12] == 64 * (127 + 128) and sizes[13] == 128 * 127 and sizes[14] == sizes[15] == 64 * 127
    path = tmp_path / "p.ptau"
    path.write_bytes(PC.ptau(6))
    assert ug.ptau_info(str(path))["power"] == 6 and ug.ptau_info(memoryview(PC.ptau(6)))["prepared"]
    # a section 12 that lost its top levels serves a smaller domain
    cut = PC.with_sections(PC.ptau(6), {12: dict(RC.sections(PC.ptau(6)))[12][:64 * 127]})
    assert ug.ptau_info(cut)["max_log_domain"] == 5


def test_refusals():
    ug = _ug()
    _, _, r1cs = SC.odd_circuit(12, 0, 0)                    # domain 2^5
    good = PC.ptau(6)
    secs = dict(RC.sections(good))
    run = lambda ptau, **kw: ug.setup_from_ptau(r1cs, ptau, device=-1, **kw)
    assert SC.zkey_header(run(good)[0])[2] == 32
    _refused(lambda: run(PC.ptau(6, prepared=False)), "ptau: not prepared for phase 2")
    for sid in (12, 13, 14, 15):
        _refused(lambda: run(PC.with_sections(good, drop=(sid,))), "ptau: not prepared for phase 2")
    bad_prime = bytearray(secs[1]); bad_prime[4] ^= 1
    _refused(lambda: run(PC.with_sections(good, {1: bytes(bad_prime)})), "ptau: not over the BN254 base field")
    r_prime = secs[1][:4] + R.to_bytes(32, "little") + secs[1][36:]
    _refused(lambda: run(PC.with_sections(good, {1: r_prime})), "ptau: not over the BN254 base field")
    _refused(lambda: run(PC.with_sections(good, {1: struct.pack("<I", 31) + secs[1][4:]})), "ptau: n8 is 31, not 32")
    _refused(lambda: run(PC.with_sections(good, drop=(1,))), "ptau: section 1 (header) is missing")
    _refused(lambda: run(PC.with_sections(good, {1: secs[1][:3]})), "ptau: section 1 (header) is too short")
    _refused(lambda: run(PC.with_sections(good, {1: secs[1][:43]})), "ptau: section 1 (header) is too short")
    _refused(lambda: run(PC.with_sections(good, {1: secs[1][:36] + struct.pack("<II", 4, 6)})), "ptau: power 4 is below the circuit's 5")
    _refused(lambda: run(good, log_domain=7), "ptau: power 6 is below the circuit's 7")
    _refused(lambda: run(PC.with_sections(good, {1: secs[1][:36] + struct.pack("<II", 29, 29)})), "ptau: sizes that cannot be represented")
    _refused(lambda: run(PC.with_sections(good, {1: secs[1][:36] + struct.pack("<II", 0xffffffff, 6)})), "ptau: sizes that cannot be represented")
    # each section one record short of what a domain of 2^5 reads (section 12: levels 0 .. 6, the others 0 .. 5)
    need = {12: 64 * 127, 13: 128 * 63, 14: 64 * 63, 15: 64 * 63, 4: 64, 5: 64, 6: 128}
    for sid, size in need.items():
        _refused(lambda: run(PC.with_sections(good, {sid: secs[sid][:size - 1]})), "ptau: section %d is too short" % sid)
        assert run(PC.with_sections(good, {sid: secs[sid][:size]}))[0] == run(good)[0]
    for sid in (4, 5, 6):
        _refused(lambda: run(PC.with_sections(good, drop=(sid,))), "ptau: section %d is missing" % sid)
    _refused(lambda: run(b"zkey" + good[4:]), "ptau: Invalid file type")
    _refused(lambda: run(good[:-5]), "ptau: Section")
    _refused(lambda: run(good[:8]), "ptau: File is too short")
    # a section size that wraps
    at = good.index(struct.pack("<IQ", 12, len(secs[12])))
    _refused(lambda: run(good[:at + 4] + struct.pack("<Q", (1 << 64) - 8) + good[at + 12:]), "ptau: Section")
    # options and the circuit
    _refused(lambda: run(good, delta=0), "setup: delta is 0 mod r")
    _refused(lambda: run(good, delta=R), "setup: delta is not below the field modulus")
    _refused(lambda: run(good, delta="random"), "setup: delta is None")
    _refused(lambda: run(good, validate=3), "setup: validate 3")
    _refused(lambda: run(good, log_domain=4), "setup: log_domain 4 is too small")
    _refused(lambda: ug.setup_from_ptau(r1cs[:-5], good, device=-1), "setup: Section")
    _refused(lambda: ug.ptau_info(b"ptau" + bytes(3)), "ptau: File is too short")


def test_a_planted_bad_point_is_found_only_where_it_is_read():
    ug = _ug()
    _, _, r1cs = SC.odd_circuit(12, 0, 0)
    good = PC.ptau(6)
    secs = dict(RC.sections(good))
    run = lambda ptau, **kw: ug.setup_from_ptau(r1cs, ptau, device=-1, **kw)

    def planted(sid, record, size=64, word=0):
        p = bytearray(secs[sid])
        p[record * size + word] ^= 1
        return PC.with_sections(good, {sid: bytes(p)})

    _refused(lambda: run(planted(12, 31 + 7)), "ptau: section 12 point 38: not on the curve")          # level 5
    _refused(lambda: run(planted(12, 63 + 9)), "ptau: section 12 point 72: not on the curve")          # level 6, an odd record
    _refused(lambda: run(planted(13, 31 + 3, 128)), "ptau: section 13 point 34: not on the curve")
    _refused(lambda: run(planted(14, 31)), "ptau: section 14 point 31: not on the curve")
    _refused(lambda: run(planted(15, 62)), "ptau: section 15 point 62: not on the curve")
    _refused(lambda: run(planted(4, 0)), "ptau: section 4 point 0: not on the curve")
    _refused(lambda: run(planted(6, 0, 128)), "ptau: section 6 point 0: not on the curve")
    q_bytes = O.Q_MOD.to_bytes(32, "little")
    unreduced = bytearray(secs[12]); unreduced[64 * 40:64 * 40 + 32] = q_bytes
    _refused(lambda: run(PC.with_sections(good, {12: bytes(unreduced)})), "ptau: section 12 point 40: coordinate not below the field modulus")
    key = run(good)[0]
    for ptau in (planted(12, 15 + 2), planted(12, 63 + 8), planted(12, 127 + 5), planted(13, 70, 128), planted(4, 1), planted(2, 0)):
        assert run(ptau)[0] == key                             # other levels, an even record of level 6, unread records
    assert run(planted(12, 38), validate=0)[0] != key          # unchecked, the bad point goes into the key


# ------------------------------------------------------------------------------------------- the key
@pytest.mark.parametrize("power", [11, 13])
def test_key_equals_dev_setup(power):
    """the trapdoor fixture's circuit at log_domain 10; power 13 moves every level's offset"""
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    ptau = PC.ptau(power)
    zkey, vkey, ms = ug.setup_from_ptau(r1cs, ptau, delta=None, log_domain=10, device=-1)
    assert (zkey, vkey) == PC.dev_setup_key(r1cs, 1, 10)
    assert set(ms) == set(ug.SETUP_PTAU_PHASES)
    deltas = (FIXED_DELTA, 2, R - 1) if power == 11 else (FIXED_DELTA,)
    for d in deltas:
        zkey, vkey, _ = ug.setup_from_ptau(r1cs, ptau, delta=d, log_domain=10, device=-1)
        assert (zkey, vkey) == PC.dev_setup_key(r1cs, d, 10), "delta %d" % d


def test_smallest_domain_and_a_mapped_file(tmp_path):
    """log_domain 0: the fixture's 433 rows fit 2^9; the .ptau given as a path that the call maps"""
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    path = tmp_path / "p11.ptau"
    path.write_bytes(PC.ptau(11))
    zkey, vkey, _ = ug.setup_from_ptau(r1cs, str(path), delta=FIXED_DELTA, device=-1)
    assert SC.zkey_header(zkey)[2] == 1 << 9
    assert (zkey, vkey) == PC.dev_setup_key(r1cs, FIXED_DELTA, 0)


def test_power_equal_to_the_domain_uses_the_padded_level():
    """power 10 = n: H comes from section 12's extra level, made with infinity for the missing top power. Every section but H
    is dev_setup's, H differs, and a proof under the key verifies all the same (the quotient's degree is below 2N - 1)."""
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, _ = ug.setup_from_ptau(r1cs, PC.ptau(10), delta=FIXED_DELTA, log_domain=10, device=-1)
    want_zkey, want_vkey = PC.dev_setup_key(r1cs, FIXED_DELTA, 10)
    got, want = dict(RC.sections(zkey)), dict(RC.sections(want_zkey))
    assert sorted(got) == sorted(want) and vkey == want_vkey
    for sid in want:
        if sid != 9:
            assert got[sid] == want[sid], "section %d" % sid
    assert got[9] != want[9] and len(got[9]) == len(want[9])
    proof, pub = O.groth16_prove(zkey, RC.golden("groth16.wtns"), 12345, 67890)
    assert pairing.groth16_verify(vkey, pub, proof) and ug.groth16_verify(proof, pub, vkey)
    bad = json.dumps([str((int(json.loads(pub)[0]) + 1) % R)] + json.loads(pub)[1:])
    assert not ug.groth16_verify(proof, bad, vkey)


def test_a_drawn_delta_changes_only_what_delta_touches():
    ug = _ug()
    _, _, r1cs = SC.odd_circuit(12, 1, 2)
    a = dict(RC.sections(ug.setup_from_ptau(r1cs, PC.ptau(6), delta="draw", device=-1)[0]))
    b = dict(RC.sections(ug.setup_from_ptau(r1cs, PC.ptau(6), delta="draw", device=-1)[0]))
    for sid in (3, 4, 5, 6, 7):
        assert a[sid] == b[sid], "section %d" % sid
    assert a[2] != b[2] and a[8] != b[8] and a[9] != b[9]
    assert a[2][:-192] == b[2][:-192]                        # the header up to delta1 | delta2


@pytest.mark.parametrize("m,n_pub_out,n_pub_in", [(12, 0, 0), (12, 1, 2)], ids=["no-public", "three-public"])
def test_irregular_circuit_equals_dev_setup(m, n_pub_out, n_pub_in):
    """repeated wires, pairs that cancel, empty combinations, wires in no matrix, coefficients r - 1 and r - 2"""
    ug = _ug()
    _, _, r1cs = SC.odd_circuit(m, n_pub_out, n_pub_in)
    for d in (1, FIXED_DELTA):
        zkey, vkey, _ = ug.setup_from_ptau(r1cs, PC.ptau(6), delta=None if d == 1 else d, device=-1)
        assert (zkey, vkey) == PC.dev_setup_key(r1cs, d, 0)
    assert ug.setup_from_ptau(r1cs, PC.ptau(6), delta=FIXED_DELTA, device=-1, validate=2)[0] == zkey


# ------------------------------------------------------------------------------------------- the tooling calls
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_points_combine_on_host_threads(g2):
    ug = _ug()
    col_ptr, index, coefs = PC.host_case()
    got = ug.points_combine(col_ptr, index, coefs, PC.points(g2), g2=g2, device=-1)
    want = PC.combine_reference(PC.host_case(), g2)
    assert got == want
    zero = bytes(128 if g2 else 64)
    base = len(PC.COEFS)
    assert got[base + 3] == zero and got[base + 4] == zero and got[base + 5] == zero and got[base + 6] == zero
    assert ug.points_combine([0], [], [], [], g2=g2, device=-1) == []
    assert ug.points_combine([0, 0, 0], [], [], PC.points(g2), g2=g2, device=-1) == [zero, zero]
    _refused(lambda: ug.points_combine([0, 1], [len(PC.points(g2))], [1], PC.points(g2), g2=g2, device=-1), "setup: term 0: point")
    _refused(lambda: ug.points_combine([0, 1], [0], [R], PC.points(g2), g2=g2, device=-1), "setup: coefficient 0 is not below")
    _refused(lambda: ug.points_combine([0, 2, 1], [0, 0], [1, 1], PC.points(g2), g2=g2, device=-1), "setup: col_ptr descends")


@pytest.mark.parametrize("n", [1, 65])
def test_points_scale_on_host_threads(n):
    ug = _ug()
    _, pts = PC.scale_points(n)
    for s in PC.scale_scalars(n):
        assert ug.points_scale(s, pts, device=-1) == PC.scale_reference(n, s), "scalar %d" % s
    assert ug.points_scale(0, pts, device=-1) == [bytes(64)] * n
    assert ug.points_scale(5, [], device=-1) == []
    _refused(lambda: ug.points_scale(R, pts, device=-1), "setup: scalar is not below the field modulus")


# ------------------------------------------------------------------------------------------- native
@pytest.fixture(scope="module")
def fuzz_ptau(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz_ptau"), "fuzz_ptau", ["fuzz_ptau.cpp", "host_util.cpp"])


def test_mutated_ptau_never_crashes_the_reader(fuzz_ptau, tmp_path):
    """tests/native/fuzz_ptau.cpp: the .ptau reader alone under AddressSanitizer + UBSan, a stand-alone child process; after a
    parse that succeeds every byte of every slice is read, which is what trips the sanitizer if a size lies"""
    path = tmp_path / "p6.ptau"
    path.write_bytes(PC.ptau(6))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_ptau, str(path), "4000", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 crashed")
    parsed, rejected = int(r.stdout.split()[0]), int(r.stdout.split()[2])
    assert rejected > 1000 and parsed > 100 and parsed + rejected == 4000


def test_cli_warns_and_writes_the_key(tmp_path):
    """zkey_new <r1cs> <ptau> <zkey> <vkey> on host threads: without --delta it says that delta = 1, with --delta draw that this
    is a single-party phase 2; --delta <file> reproduces dev_setup's key"""
    _, _, r1cs = SC.odd_circuit(12, 1, 2)
    (tmp_path / "c.r1cs").write_bytes(r1cs)
    (tmp_path / "p.ptau").write_bytes(PC.ptau(6))
    (tmp_path / "d.bin").write_bytes(FIXED_DELTA.to_bytes(32, "little"))
    exe = os.path.join(CSRC, "zkey_new")
    base = [exe, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau")]
    run = lambda out, *more: subprocess.run(base + [str(tmp_path / (out + ".zkey")), str(tmp_path / (out + ".json")), "--device", "-1"] + list(more),
                                            capture_output=True, text=True, timeout=120)
    r = run("a")
    assert r.returncode == 0 and "delta = 1" in r.stderr and "forge" in r.stderr, r.stderr
    assert (tmp_path / "a.zkey").read_bytes() == PC.dev_setup_key(r1cs, 1, 0)[0]
    assert json.loads((tmp_path / "a.json").read_text()) == PC.dev_setup_key(r1cs, 1, 0)[1]
    r = run("b", "--delta", str(tmp_path / "d.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "b.zkey").read_bytes() == PC.dev_setup_key(r1cs, FIXED_DELTA, 0)[0]
    r = run("c", "--delta", "draw", "--validate", "2")
    assert r.returncode == 0 and "single-party phase 2" in r.stderr and "snarkjs zkey verify" in r.stderr, r.stderr
    assert (tmp_path / "c.zkey").read_bytes() != (tmp_path / "a.zkey").read_bytes()
    r = run("d", "--log-domain", "7")
    assert r.returncode == 1 and "Error: ptau: power 6 is below the circuit's 7" in r.stderr and not (tmp_path / "d.zkey").exists()
