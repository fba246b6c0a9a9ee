"""Preparing a powers-of-tau file for phase 2 on host threads (device = -1): include/ultragroth_hip.h ug_ptau_prepare_*,
ug_points_intt through ultragroth_amd.ptau_prepare / ptau_check / points_intt, the reader additions of host_util.cpp under a
sanitizer, and the ptau_prepare tool. Every comparison is byte for byte: a transform of k_j * G must give the oracle's multiples of
the transformed integers, and the prepared file of a synthesized unprepared one must be the file the test writer makes from
Lagrange values of the known tau."""
import os
import struct
import subprocess

import pytest

import oracle as O
from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ptau_prepare_cases as PP

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = SC.R
HOST_LOGS = (0, 1, 2, 3, 6)


def _ug():
    import ultragroth_amd as ug
    return ug


def _refused(fn, text):
    ug = _ug()
    with pytest.raises(ug.SetupError) as e:
        fn()
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------- one transform
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("log_n", HOST_LOGS)
def test_points_intt_against_the_integers(log_n, g2):
    ug = _ug()
    for name in PP.SETS:
        given, want = PP.case(name, log_n, g2)
        got = ug.points_intt(list(given), log_n, g2=g2, device=-1)
        assert got == list(want), (name, [i for i in range(len(want)) if got[i] != want[i]][:8])
    if log_n:                                    # the closed forms of two of the sets, read off the records themselves
        given, _ = PP.case("equal", log_n, g2)
        got = ug.points_intt(list(given), log_n, g2=g2, device=-1)
        assert got[0] == given[0] and all(r == bytes(len(r)) for r in got[1:])


def test_points_intt_refusals():
    ug = _ug()
    g = SC.oracle_mul(1, False)
    _refused(lambda: ug.points_intt([g, g, g], 1, device=-1), "setup: 3 points are more than 2^1")
    _refused(lambda: ug.points_intt([g[:63]], 1, device=-1), "setup: a point record of another size")
    _refused(lambda: ug.points_intt([g], 29, device=-1), "setup: log_n 29 is not in 0 .. 28")
    assert ug.points_intt([], 2, device=-1) == [bytes(64)] * 4


# ------------------------------------------------------------------------------------------- whole files
@pytest.mark.parametrize("power", [1, 4, 6])
def test_prepared_file_equals_the_writers(power):
    ug = _ug()
    ms = {}
    assert ug.ptau_prepare(PC.ptau(power, prepared=False), device=-1, timings=ms) == PC.ptau(power)
    assert set(ms) == set(ug.PTAU_PREPARE_PHASES)


def test_power_cuts_the_file_first():
    """6 cut to 4 is the writer's file of power 4 in everything but the header's ceremonyPower: the padded level comes from the cut
    section 2 with infinity in the last place, although the file has the real next power"""
    ug = _ug()
    got = RC.sections(ug.ptau_prepare(PC.ptau(6, prepared=False), power=4, device=-1))
    want = RC.sections(PC.ptau(4))
    assert [i for i, _ in got] == [i for i, _ in want] == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    for (sid, a), (_, b) in zip(got, want):
        if sid != 1:
            assert a == b, sid
    a, b = PP.header_fields(dict(got)[1]), PP.header_fields(dict(want)[1])
    assert a["ceremony_power"] == 6 and b["ceremony_power"] == 4 and a["power"] == b["power"] == 4
    for key in ("n8", "prime", "rest"):
        assert a[key] == b[key]
    # a prepared input is cut in the same way, and the same power is no cut
    assert ug.ptau_prepare(PC.ptau(6), power=4, device=-1) == ug.ptau_prepare(PC.ptau(6, prepared=False), power=4, device=-1)
    assert ug.ptau_prepare(PC.ptau(4, prepared=False), power=4, device=-1) == PC.ptau(4)


def test_preparing_a_prepared_file_gives_the_same_file():
    ug = _ug()
    assert ug.ptau_prepare(PC.ptau(4), device=-1) == PC.ptau(4)
    # sections keep the input's order, 12 - 15 go to the end, sections this code does not know are copied
    secs = RC.sections(PC.ptau(4))
    shuffled = RC.binfile(b"ptau", 1, [secs[8], secs[5], secs[0], (99, b"xyz"), secs[2], secs[1], secs[3], secs[4], secs[6]])
    out = RC.sections(ug.ptau_prepare(shuffled, device=-1))
    assert [i for i, _ in out] == [6, 1, 99, 3, 2, 4, 5, 7, 12, 13, 14, 15]
    assert dict(out) == dict(secs + [(99, b"xyz")])


def test_check_accepts_the_writers_file_and_names_a_planted_record():
    ug = _ug()
    good = PC.ptau(6)
    assert ug.ptau_check(good, device=-1) is None
    for sid, record in PP.plants(6):
        hit = ug.ptau_check(PP.planted(good, sid, record), device=-1)
        assert hit == (sid, record, "ptau: section %d point %d: does not match the powers" % (sid, record)), (sid, record, hit)
    # the first mismatch in section order, whatever the order of the work
    small = PC.ptau(4)
    both = PP.planted(PP.planted(small, 13, 12), 12, 40)
    assert ug.ptau_check(both, device=-1)[:2] == (12, 40)
    # doctored POWERS are a mismatch of the first record that depends on them: level 0 of section 14 is alpha * G itself
    assert ug.ptau_check(PP.planted(small, 4, 0), device=-1)[:2] == (14, 0)


def test_refusals():
    ug = _ug()
    raw = PC.ptau(6, prepared=False)
    good = PC.ptau(6)
    secs = dict(RC.sections(raw))
    run = lambda ptau, **kw: ug.ptau_prepare(ptau, device=-1, **kw)
    check = lambda ptau, **kw: ug.ptau_check(ptau, device=-1, **kw)
    # the header rules, as they are for setup_from_ptau
    bad_prime = bytearray(secs[1]); bad_prime[4] ^= 1
    _refused(lambda: run(PC.with_sections(raw, {1: bytes(bad_prime)})), "ptau: not over the BN254 base field")
    _refused(lambda: run(PC.with_sections(raw, {1: struct.pack("<I", 31) + secs[1][4:]})), "ptau: n8 is 31, not 32")
    _refused(lambda: run(PC.with_sections(raw, drop=(1,))), "ptau: section 1 (header) is missing")
    _refused(lambda: run(PC.with_sections(raw, {1: secs[1][:43]})), "ptau: section 1 (header) is too short")
    _refused(lambda: run(PC.with_sections(raw, {1: secs[1][:36] + struct.pack("<II", 29, 29)})), "ptau: sizes that cannot be represented")
    _refused(lambda: run(b"zkey" + raw[4:]), "ptau: Invalid file type")
    _refused(lambda: run(raw[:8]), "ptau: File is too short")
    _refused(lambda: run(raw[:-3]), "ptau: Section")
    # the power
    _refused(lambda: run(raw, power=7), "ptau: power 7 is above the file's 6")
    _refused(lambda: run(raw, power=1 << 32), "setup: power")
    # sections 2 - 5: each one record short of its count, then exactly at it; missing
    need = {2: 64 * 127, 3: 128 * 64, 4: 64 * 64, 5: 64 * 64}
    for sid, size in need.items():
        _refused(lambda: run(PC.with_sections(raw, {sid: secs[sid][:size - 1]})), "ptau: section %d is too short" % sid)
        _refused(lambda: run(PC.with_sections(raw, drop=(sid,))), "ptau: section %d is missing" % sid)
    # ... and of the cut's counts when the file is cut: a file that claims power 6 but holds the records of power 4 serves power 4
    short = PC.with_sections(raw, {2: secs[2][:64 * 31], 3: secs[3][:128 * 16], 4: secs[4][:64 * 16], 5: secs[5][:64 * 16]})
    _refused(lambda: run(short), "ptau: section 2 is too short")
    _refused(lambda: run(short, power=5), "ptau: section 2 is too short")
    assert RC.sections(run(short, power=4))[7:] == RC.sections(PC.ptau(4))[7:]
    # a header that claims more than the file holds: counts are compared, never multiplied up
    _refused(lambda: run(PC.with_sections(raw, {1: secs[1][:36] + struct.pack("<II", 27, 27)})), "ptau: section 2 is too short")
    # power 28: the padded level would be a transform of 2^29 points; the same header serves a cut
    claims28 = PC.with_sections(raw, {1: secs[1][:36] + struct.pack("<II", 28, 28)})
    _refused(lambda: run(claims28), "ptau: power 28: the padded level of section 12 would need a root of unity of order 2^29")
    _refused(lambda: check(PC.with_sections(good, {1: secs[1][:36] + struct.pack("<II", 28, 28)})), "ptau: power 28: the padded level")
    assert RC.sections(run(claims28, power=6))[1:] == RC.sections(PC.ptau(6))[1:]
    # the point check, over what is read
    def bad(sid, record, size=64):
        p = bytearray(secs[sid])
        p[record * size] ^= 1
        return PC.with_sections(raw, {sid: bytes(p)})
    _refused(lambda: run(bad(2, 126)), "ptau: section 2 point 126: not on the curve")
    _refused(lambda: run(bad(3, 63, 128)), "ptau: section 3 point 63: not on the curve")
    _refused(lambda: run(bad(4, 0)), "ptau: section 4 point 0: not on the curve")
    _refused(lambda: run(bad(5, 17)), "ptau: section 5 point 17: not on the curve")
    q_bytes = O.Q_MOD.to_bytes(32, "little")
    unreduced = bytearray(secs[2]); unreduced[64 * 40:64 * 40 + 32] = q_bytes
    _refused(lambda: run(PC.with_sections(raw, {2: bytes(unreduced)})), "ptau: section 2 point 40: coordinate not below the field modulus")
    assert run(bad(2, 31), power=4) == run(raw, power=4)             # beyond the cut: not read
    assert run(bad(2, 126), validate=0) != PC.ptau(6)                # unchecked, the bad point goes into the levels
    _refused(lambda: run(raw, validate=3), "setup: validate 3")
    # the check
    _refused(lambda: check(raw), "ptau: not prepared for phase 2")
    full = dict(RC.sections(good))
    for sid in PP.LAGRANGE_IDS:
        _refused(lambda: check(PC.with_sections(good, drop=(sid,))), "ptau: not prepared for phase 2")
        _refused(lambda: check(PC.with_sections(good, {sid: full[sid][:-1]})), "ptau: section %d is too short" % sid)
    _refused(lambda: check(good, validate=3), "setup: validate 3")


# ------------------------------------------------------------------------------------------- native
@pytest.fixture(scope="module")
def fuzz_prepare(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz_ptau_prepare"), "fuzz_ptau_prepare", ["fuzz_ptau_prepare.cpp", "host_util.cpp"])


def test_mutated_ptau_never_crashes_the_reader(fuzz_prepare, tmp_path):
    """tests/native/fuzz_ptau_prepare.cpp: what the preparation reads of a file, alone under AddressSanitizer + UBSan, a stand-alone
    child process; after a parse that succeeds every byte of every slice is read, which is what trips the sanitizer if a size lies"""
    path = tmp_path / "p6.ptau"
    path.write_bytes(PC.ptau(6, prepared=False))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_prepare, str(path), "4000", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 crashed")
    parsed, rejected = int(r.stdout.split()[0]), int(r.stdout.split()[2])
    assert rejected > 1000 and parsed > 100 and parsed + rejected == 4000


def test_cli_prepares_cuts_and_checks(tmp_path):
    """ptau_prepare <in> <out> and ptau_prepare --check on host threads, files mapped; a refusal leaves no output file"""
    (tmp_path / "raw.ptau").write_bytes(PC.ptau(4, prepared=False))
    (tmp_path / "six.ptau").write_bytes(PC.ptau(6, prepared=False))
    exe = os.path.join(CSRC, "ptau_prepare")
    run = lambda *args: subprocess.run([exe] + [str(a) for a in args] + ["--device", "-1"], capture_output=True, text=True, timeout=120)
    r = run(tmp_path / "raw.ptau", tmp_path / "out.ptau")
    assert r.returncode == 0 and "prepared file written" in r.stdout, r.stderr
    assert (tmp_path / "out.ptau").read_bytes() == PC.ptau(4)
    r = run(tmp_path / "six.ptau", tmp_path / "cut.ptau", "--power", "4", "--validate", "2")
    assert r.returncode == 0, r.stderr
    assert RC.sections((tmp_path / "cut.ptau").read_bytes())[1:] == RC.sections(PC.ptau(4))[1:]
    r = run("--check", tmp_path / "out.ptau")
    assert r.returncode == 0 and "are the Lagrange forms" in r.stdout, r.stderr
    (tmp_path / "bad.ptau").write_bytes(PP.planted(PC.ptau(4), 14, 30))
    r = run("--check", tmp_path / "bad.ptau")
    assert r.returncode == 1 and "Error: ptau: section 14 point 30: does not match the powers" in r.stderr, r.stderr
    r = run("--check", tmp_path / "raw.ptau")
    assert r.returncode == 1 and "Error: ptau: not prepared for phase 2" in r.stderr, r.stderr
    r = run(tmp_path / "raw.ptau", tmp_path / "raw.ptau")
    assert r.returncode == 1 and "the output is the input file" in r.stderr, r.stderr
    os.link(tmp_path / "raw.ptau", tmp_path / "same.ptau")
    r = run(tmp_path / "raw.ptau", tmp_path / "same.ptau")
    assert r.returncode == 1 and "the output is the input file" in r.stderr, r.stderr
    assert (tmp_path / "raw.ptau").read_bytes() == PC.ptau(4, prepared=False)
    r = run(tmp_path / "raw.ptau", tmp_path / "none.ptau", "--power", "5")
    assert r.returncode == 1 and "Error: ptau: power 5 is above the file's 4" in r.stderr and not (tmp_path / "none.ptau").exists()
