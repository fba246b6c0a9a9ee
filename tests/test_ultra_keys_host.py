"""UltraGroth keys from a prepared powers-of-tau file on host threads (device = -1): include/ultragroth_hip.h
ug_ultra_setup_ptau_*, ug_points_scale_segments through ultragroth_amd.ultra_setup_from_ptau / points_scale_segments and the
zkey_new_ultra tool. Every comparison is byte for byte: a .ptau synthesized from the fixture's (tau, alpha, beta) must give the
key dev_setup gives for protocol 1337 and the trapdoor (tau, alpha, beta, gamma = 1, delta_round, delta_final)."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ultra_keys_cases as UC

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = SC.R


def _ug():
    import ultragroth_amd as ug
    return ug


def _refused(fn, text):
    ug = _ug()
    with pytest.raises(ug.SetupError) as e:
        fn()
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------- the key
@pytest.mark.parametrize("d_round,d_final", UC.DELTA_PAIRS, ids=["ones", "round", "both"])
def test_key_equals_dev_setup(d_round, d_final):
    ug = _ug()
    r1cs, spec, power, log_domain = UC.fixture()
    zkey, vkey, ms = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta=UC.delta_arg(d_round, d_final), log_domain=log_domain, device=-1)
    assert (zkey, vkey) == UC.dev_key(r1cs, spec, d_round, d_final, log_domain)
    assert set(ms) == set(ug.SETUP_PTAU_PHASES)
    assert vkey["protocol"] == "ultragroth" and "vk_delta_c1_2" in vkey and "IC_rand" in vkey
    assert [i for i, _ in RC.sections(zkey)] == list(range(1, 14)) and dict(RC.sections(zkey))[13] == b""


@pytest.mark.parametrize("kind", ["alternating", "no-round", "no-final", "descending"])
def test_irregular_circuit_and_list_shapes(kind):
    """repeated wires, pairs that cancel, wires in no matrix; an empty list on either side; lists from the top down, which
    sections 8 - 11 must follow"""
    ug = _ug()
    r1cs, spec = UC.irregular(kind)
    for d_round, d_final in UC.DELTA_PAIRS:
        zkey, vkey, _ = ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta=UC.delta_arg(d_round, d_final), device=-1)
        assert (zkey, vkey) == UC.dev_key(r1cs, spec, d_round, d_final), "deltas %d %d" % (d_round, d_final)
    secs = dict(RC.sections(zkey))
    assert secs[10] == struct.pack("<%dI" % len(spec["round_signals"]), *spec["round_signals"])
    assert secs[11] == struct.pack("<%dI" % len(spec["final_signals"]), *spec["final_signals"])
    assert len(secs[8]) == 64 * len(spec["round_signals"]) and len(secs[9]) == 64 * len(spec["final_signals"])
    if kind == "descending":
        up = dict(RC.sections(ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), UC.irregular("alternating")[1], delta=(d_round, d_final), device=-1)[0]))
        recs = lambda b: [b[i:i + 64] for i in range(0, len(b), 64)]
        assert recs(secs[8]) == recs(up[8])[::-1] and recs(secs[9]) == recs(up[9])[::-1] and secs[8] != up[8]


def test_a_drawn_pair_changes_only_what_the_deltas_touch():
    ug = _ug()
    r1cs, spec = UC.irregular()
    a = dict(RC.sections(ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta="draw", device=-1)[0]))
    b = dict(RC.sections(ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta="draw", device=-1)[0]))
    for sid in (3, 4, 5, 6, 7, 10, 11):
        assert a[sid] == b[sid], "section %d" % sid
    for sid in (2, 8, 9, 12):
        assert a[sid] != b[sid], "section %d" % sid
    assert a[2][:-384] == b[2][:-384]                        # the header up to delta_c1 | delta_c2
    dc1, dc2 = a[2][-384:-192], a[2][-192:]
    assert dc1 != dc2 and dc1 != b[2][-384:-192] and dc2 != b[2][-192:]     # two draws per key, fresh ones per call


def test_refusals():
    ug = _ug()
    r1cs, spec = UC.irregular()
    good = PC.ptau(6)
    run = lambda s=spec, ptau=good, **kw: ug.ultra_setup_from_ptau(r1cs, ptau, s, device=-1, **kw)
    rs, fs = spec["round_signals"], spec["final_signals"]
    _refused(lambda: run(dict(spec, rand_indx=4)), "setup: rand_indx 4 is not a public signal")
    _refused(lambda: run(dict(spec, rand_indx=0)), "setup: rand_indx 0 is not a public signal")
    _refused(lambda: run(dict(spec, final_signals=fs[:-1] + [rs[0]])), "do not partition the private signals: signal %d" % rs[0])
    _refused(lambda: run(dict(spec, final_signals=fs[:-1] + [2])), "do not partition the private signals: signal 2")
    _refused(lambda: run(dict(spec, round_signals=rs[1:])), "setup: the round and final signal lists do not partition the private signals 4 .. ")
    _refused(lambda: run(dict(spec, final_signals=fs[:-1] + [1 << 31])), "do not partition the private signals: signal %d" % (1 << 31))
    _refused(lambda: run(delta=(0, 1)), "setup: delta_round is 0 mod r")
    _refused(lambda: run(delta=(1, 0)), "setup: delta_final is 0 mod r")
    _refused(lambda: run(delta=(R, 1)), "setup: delta_round is not below the field modulus")
    _refused(lambda: run(delta=(1, R + 5)), "setup: delta_final is not below the field modulus")
    _refused(lambda: run(delta="random"), "setup: delta is None")
    _refused(lambda: run(delta=5), "setup: delta is None")
    _refused(lambda: run(ptau=PC.ptau(6, prepared=False)), "ptau: not prepared for phase 2")
    _refused(lambda: run(log_domain=7), "ptau: power 6 is below the circuit's 7")
    _refused(lambda: run(validate=3), "setup: validate 3")
    _refused(lambda: ug.ultra_setup_from_ptau(r1cs[:-5], good, spec, device=-1), "setup: Section")
    _refused(lambda: ug.ultra_setup_from_ptau(r1cs, good, None, device=-1), "setup: an UltraGroth key needs")
    # a list rule fires before the .ptau is looked at, the .ptau's before any point: both wrong, the list is named
    _refused(lambda: run(dict(spec, rand_indx=9), ptau=PC.ptau(6, prepared=False)), "setup: rand_indx 9")
    # the Groth16 entry is what it was
    assert SC.zkey_header(ug.setup_from_ptau(r1cs, good, device=-1)[0])[2] == 32


def test_the_groth16_check_still_refuses_an_ultragroth_key():
    """ug_zkey_verify_run keeps its refusal of protocol 1337, for the committed key and for one made here (ug_ultra_zkey_verify_run is
    the call for them: tests/test_ultra_verify_host.py)"""
    ug = _ug()
    r1cs, spec, power, log_domain = UC.fixture()
    made = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta=(UC.FIXED_DELTA, UC.OTHER_DELTA), log_domain=log_domain, device=-1)[0]
    for zkey in (RC.golden("ultra.zkey"), made):
        _refused(lambda: ug.zkey_verify(r1cs, PC.ptau(power), zkey, device=-1), "zkey: protocol 1337 keys are not checked")


# ------------------------------------------------------------------------------------------- the tooling call
@pytest.mark.parametrize("which", range(len(UC.SEGMENT_COUNTS)), ids=["%d-%d-%d" % c for c in UC.SEGMENT_COUNTS])
def test_points_scale_segments_on_host_threads(which):
    ug = _ug()
    segments, pts = UC.segment_case(which)
    got = ug.points_scale_segments(segments, pts, device=-1)
    want = UC.segment_reference(which)
    assert [len(g) for g in got] == list(UC.SEGMENT_COUNTS[which])
    assert got == want
    for (scalar, index, count), g in zip(segments, got):
        if scalar == 0:
            assert g == [bytes(64)] * count
        if scalar == 1:
            assert g == [pts[j] for j in (index if index is not None else range(count))]
        if count >= 2 and index is not None:
            assert g[0] == bytes(64) and g[-1] == bytes(64)                  # infinity in, infinity out
    if UC.SEGMENT_COUNTS[which][2] >= 64 and segments[2][0]:
        assert got[2][0] == bytes(64) and got[2][63] == bytes(64)


def test_points_scale_segments_rules():
    ug = _ug()
    _, pts = PC.scale_points(65)
    one = ug.points_scale_segments([(7, None, 65)], pts, device=-1)
    assert one == [ug.points_scale(7, pts, device=-1)]
    assert ug.points_scale_segments([], pts, device=-1) == []
    assert ug.points_scale_segments([(5, None, 0), (5, [], 0)], pts, device=-1) == [[], []]
    assert ug.points_scale_segments([(3, [64, 64, 1], 3)], pts, device=-1) == [[ug.points_scale(3, pts, device=-1)[j] for j in (64, 64, 1)]]
    _refused(lambda: ug.points_scale_segments([(R, None, 1)], pts, device=-1), "setup: segment 0: scalar is not below the field modulus")
    _refused(lambda: ug.points_scale_segments([(1, None, 1), (2, [65], 1)], pts, device=-1), "setup: segment 1 index 0: point 65 out of range")
    _refused(lambda: ug.points_scale_segments([(2, None, 66)], pts, device=-1), "setup: segment 0: 66 records of 65")
    _refused(lambda: ug.points_scale_segments([(2, None, 1)] * 4, pts, device=-1), "setup: 4 segments: at most 3")


# ------------------------------------------------------------------------------------------- ABI
def test_the_new_symbols_are_declared_exported_and_mirrored():
    ug = _ug()
    from ultragroth_amd import _lib
    lib = ug.load()
    header = open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ug_ultra_setup_ptau_size", "ug_ultra_setup_ptau_run", "ug_points_scale_segments"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.INNER_SYMBOLS and hasattr(lib, name), name
    # struct sizes: the header's layout, restated (4 u32, 64 bytes, 2 u32, two pointer + count pairs | two pointers, a count)
    assert C.sizeof(ug._UltraSetupPtauOptions) == 16 + 64 + 8 + 32 == 120
    assert C.sizeof(ug._ScaleSegment) == 24
    r1cs, spec = UC.irregular()
    opt = ug._UltraSetupPtauOptions()
    opt.size = 119                                           # another size is refused, by the size the library was built with
    err = C.create_string_buffer(256)
    z = C.c_uint64()
    assert lib.ug_ultra_setup_ptau_size(C.byref(opt), r1cs, len(r1cs), PC.ptau(6), len(PC.ptau(6)), C.byref(z), None, err, 255) != 0
    assert err.value == b"setup: options struct of another size (119)"
    assert lib.ug_ultra_setup_ptau_size(None, r1cs, len(r1cs), PC.ptau(6), len(PC.ptau(6)), C.byref(z), None, err, 255) != 0
    assert err.value == b"setup: null options"


# ------------------------------------------------------------------------------------------- the tool
def test_cli_warns_and_writes_the_key(tmp_path):
    """zkey_new_ultra <r1cs> <ptau> <spec> <zkey> <vkey> on host threads: without --delta it says that both deltas are 1, with
    --delta draw that this is a single-party phase 2; --delta <file> (64 bytes) reproduces dev_setup's key; exit codes 0 and 1"""
    r1cs, spec = UC.irregular()
    (tmp_path / "c.r1cs").write_bytes(r1cs)
    (tmp_path / "p.ptau").write_bytes(PC.ptau(6))
    (tmp_path / "s.json").write_text(json.dumps(spec))
    (tmp_path / "d.bin").write_bytes(UC.FIXED_DELTA.to_bytes(32, "little") + UC.OTHER_DELTA.to_bytes(32, "little"))
    (tmp_path / "short.bin").write_bytes(UC.FIXED_DELTA.to_bytes(32, "little"))
    exe = os.path.join(CSRC, "zkey_new_ultra")
    base = [exe, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau")]

    def run(out, *more, spec_file="s.json"):
        return subprocess.run(base + [str(tmp_path / spec_file), str(tmp_path / (out + ".zkey")), str(tmp_path / (out + ".json")), "--device", "-1"]
                              + list(more), capture_output=True, text=True, timeout=120)

    r = run("a")
    assert r.returncode == 0 and "delta_round = delta_final = 1" in r.stderr and "forge" in r.stderr, r.stderr
    assert (tmp_path / "a.zkey").read_bytes() == UC.dev_key(r1cs, spec, 1, 1)[0]
    assert json.loads((tmp_path / "a.json").read_text()) == UC.dev_key(r1cs, spec, 1, 1)[1]
    r = run("b", "--delta", str(tmp_path / "d.bin"))
    assert r.returncode == 0 and "forges" in r.stderr, r.stderr
    assert (tmp_path / "b.zkey").read_bytes() == UC.dev_key(r1cs, spec, UC.FIXED_DELTA, UC.OTHER_DELTA)[0]
    r = run("c", "--delta", "draw", "--validate", "2")
    assert r.returncode == 0 and "single-party phase 2" in r.stderr and "no transcript" in r.stderr, r.stderr
    assert (tmp_path / "c.zkey").read_bytes() != (tmp_path / "a.zkey").read_bytes()
    r = run("d", "--delta", str(tmp_path / "short.bin"))
    assert r.returncode == 1 and "64 bytes" in r.stderr and not (tmp_path / "d.zkey").exists()
    (tmp_path / "bad.json").write_text(json.dumps(dict(spec, rand_indx=5)))
    r = run("e", spec_file="bad.json")
    assert r.returncode == 1 and "Error: setup: rand_indx 5 is not a public signal" in r.stderr and not (tmp_path / "e.zkey").exists()
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Usage: zkey_new_ultra" in r.stderr


# ------------------------------------------------------------------------------------------- native
@pytest.fixture(scope="module")
def fuzz_ultra(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz_ultra_keys"), "fuzz_ultra_keys",
                                 ["fuzz_ultra_keys.cpp", "zkey_verify_host.cpp", "setup_ptau.cpp", "point_check.cpp", "setup_host.cpp", "host_util.cpp"],
                                 flags=("-O2", "-pthread", "-Wno-unknown-pragmas"))


def test_mutated_inputs_never_crash_the_setup(fuzz_ultra, tmp_path):
    """tests/native/fuzz_ultra_keys.cpp: the host path alone (no HIP code linked) under AddressSanitizer + UBSan, a stand-alone
    child process: a two-constraint circuit, its .ptau, the signal lists and the deltas through the setup, and the key they give
    (or the spec it is checked against) through the check, one of them mutated per turn"""
    from ultragroth_amd import synth
    rows = [({1: 1}, {2: 1}, {3: 1}), ({3: 1, 0: R - 1}, {3: 1}, {4: 1, 1: 2})]
    r1cs = synth.r1cs_file(6, 1, 0, rows)
    (tmp_path / "c.r1cs").write_bytes(r1cs)
    (tmp_path / "p.ptau").write_bytes(PC.ptau(2))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_ultra, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau"), "1", "6", "3000", "1"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 crashed")
    words = r.stdout.replace(",", "").split()
    keys, refused, valid, invalid, check_refused = int(words[0]), int(words[2]), int(words[4]), int(words[6]), int(words[8])
    assert keys + refused + valid + invalid + check_refused == 3000
    assert refused > 800 and keys > 150 and check_refused > 150 and invalid > 20 and valid > 10
