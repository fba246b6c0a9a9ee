"""Naming the wrong records of a failing section on host threads (include/ultragroth_hip.h: ug_zkey_locate_run,
ug_ultra_zkey_locate_run, device = -1): zkey_locate_cases.py fixes every located report in advance; the verdict, failing sections,
first section and message must be zkey_verify's on the same files. test_gpu_zkey_locate.py holds the device to the same answers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
import sanitized_build
import setup_ptau_cases as PC
import ultra_keys_cases as UC
import zkey_locate_cases as LC
import zkey_verify_cases as ZC
import ultragroth_amd as ug
from ultragroth_amd import _lib

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")


# ------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize("case_id", ("fixture-delta-1", "fixture-fixed-delta", "dev-setup-own-gamma"))
def test_valid_keys_locate_nothing(case_id):
    timings = {}
    assert ug.zkey_locate(*ZC.valid_case(case_id), device=-1, timings=timings) is None
    assert timings["locate"] == 0


def test_valid_chain_keys():
    assert ug.zkey_locate(LC.chain()[3], PC.ptau(LC.CHAIN_POWER), LC.chain_key(), device=-1) is None
    assert ug.ultra_zkey_locate(LC.chain()[3], PC.ptau(LC.CHAIN_POWER), LC.ultra_chain_key(), ultra=LC.chain_spec(), device=-1) is None


@pytest.mark.parametrize("case_id", LC.PLANTED_IDS)
def test_planted_changes_are_named(case_id):
    LC.check_planted(case_id, -1)


def test_planted_cases_are_all_listed():
    assert set(LC.planted_cases()) == set(LC.PLANTED_IDS) and set(LC.GPU_PLANTED_IDS) <= set(LC.PLANTED_IDS)
    assert set(LC.ultra_cases()) == set(LC.ULTRA_IDS)


@pytest.mark.parametrize("case_id", ("swap-5", "swap-3", "swap-8", "other-delta-9", "ptau-of-tau-plus-1", "section-4-byte", "delta1-of-another-key",
                                     "gamma2-and-delta1-at-infinity", "section-4-byte-swap-3-other-delta-9"))
def test_small_circuit_answers_are_the_verify_entrys(case_id):
    """zkey_verify_cases' keys of the 12-constraint circuit: verdict, sections, first section and message as fixed there; an entry for
    every failing point section and for no other (section 3 under a gamma2 at infinity has none: there is no ratio to test)"""
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case_id]
    got = ug.zkey_locate(r1cs, ptau, zkey, device=-1)
    assert got[:3] == (first, failing, message)
    want = [s for s in failing if s in (3, 5, 6, 7, 8, 9)]
    if case_id == "gamma2-and-delta1-at-infinity":
        want = []
    assert sorted(got[3]) == want
    for sid, e in got[3].items():
        assert e["method"] == LC.METHOD[sid] and e["exact"] == 1 and 1 <= e["bad_records"] <= e["records"] and e["index"] == sorted(e["index"])
        assert all(i < e["records"] for i in e["index"])
    if case_id.startswith("swap-"):
        assert got[3][failing[0]]["bad_records"] == 2
    if case_id == "ptau-of-tau-plus-1":          # another tau: every record that is not infinity on both sides is wrong
        assert got[3][9]["bad_records"] == got[3][9]["records"] == 32


@pytest.mark.parametrize("case_id", LC.ULTRA_IDS)
def test_ultragroth_sections(case_id):
    got = LC.check_ultra(case_id, -1)
    if case_id == "c1-record-replaced":          # the index is the place in the key's list: the wire is round_signals[i]
        assert LC.chain_spec()["round_signals"][got[3][8]["index"][0]] == 591 - 2 * 257


@pytest.mark.parametrize("case_id", ZC.REFUSAL_IDS)
def test_refusals_are_the_verify_entrys(case_id):
    r1cs, ptau, zkey, text = ZC.refusals()[case_id]
    with pytest.raises(ug.SetupError) as e:
        ug.zkey_locate(r1cs, ptau, zkey, device=-1)
    assert text in str(e.value)
    with pytest.raises(ug.SetupError) as v:
        ug.zkey_verify(r1cs, ptau, zkey, device=-1)
    assert str(v.value) == str(e.value)


@pytest.mark.parametrize("case_id", ("groth16-key", "lists-do-not-partition", "rand-indx-not-public"))
def test_ultra_refusals_are_the_verify_entrys(case_id):
    r1cs, ptau, zkey, validate, text = UC.refusals()[case_id]
    with pytest.raises(ug.SetupError) as e:
        ug.ultra_zkey_locate(r1cs, ptau, zkey, device=-1, validate=validate)
    assert text in str(e.value)
    with pytest.raises(ug.SetupError) as v:
        ug.ultra_zkey_verify(r1cs, ptau, zkey, device=-1, validate=validate)
    assert str(v.value) == str(e.value)


# ------------------------------------------------------------------------------------------- ABI
def _header():
    return open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()


def test_symbols_are_declared_listed_and_exported():
    lib = ug.load()
    for name in ("ug_points_ratio_mask", "ug_zkey_locate_run", "ug_ultra_zkey_locate_run"):
        assert re.search(r"\b%s\s*\(" % name, _header()) and name in _lib.INNER_SYMBOLS and hasattr(lib, name)
    for name, value in (("UG_RATIO_LISTED", ug.UG_RATIO_LISTED), ("UG_ZKEY_LOCATE_SECTIONS", ug.UG_ZKEY_LOCATE_SECTIONS),
                        ("UG_ZKEY_LOCATE_LISTED", ug.UG_ZKEY_LOCATE_LISTED), ("UG_LOCATE_BYTES", ug.LOCATE_METHODS.index("bytes")),
                        ("UG_LOCATE_RATIO", ug.LOCATE_METHODS.index("ratio"))):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, _header())
        assert m and int(m.group(1)) == value


def test_structs_have_the_c_layout():
    assert C.sizeof(ug._ZkeyVerifyOptions) == 8 and C.sizeof(ug._UltraZkeyVerifyOptions) == 48          # the old ones, unchanged
    assert C.sizeof(ug._ZkeyLocateOptions) == 16 and ug._ZkeyLocateOptions.max_listed.offset == 8 and ug._ZkeyLocateOptions.max_blocks.offset == 12
    assert C.sizeof(ug._UltraZkeyLocateOptions) == 56 and ug._UltraZkeyLocateOptions.max_listed.offset == 48
    assert C.sizeof(ug._ZkeyLocateSection) == 72 + 8 * 1024 and ug._ZkeyLocateSection.index.offset == 72 and ug._ZkeyLocateSection.exact.offset == 48
    assert C.sizeof(ug._ZkeyLocateReport) == 16 + 7 * (72 + 8 * 1024) and ug._ZkeyLocateReport.section.offset == 16
    assert C.sizeof(ug._RatioReport) == 48 + 8 * 16 + 16 and ug._RatioReport.index.offset == 48


def _call(entry, opt, size, extra=()):
    opt.size = size
    opt.validate = 2
    rep, err = ug._ZkeyVerifyReport(), C.create_string_buffer(256)
    rc = entry(C.byref(opt), None, 0, None, 0, None, 0, -1, C.byref(rep), *extra, None, err, 255)
    return rc, err.value.decode()


def test_every_entry_refuses_a_struct_of_another_size():
    lib = ug.load()
    located = ug._ZkeyLocateReport()
    for entry, struct, extra in ((lib.ug_zkey_verify_run, ug._ZkeyVerifyOptions, ()), (lib.ug_ultra_zkey_verify_run, ug._UltraZkeyVerifyOptions, ()),
                                 (lib.ug_zkey_locate_run, ug._ZkeyLocateOptions, (C.byref(located),)),
                                 (lib.ug_ultra_zkey_locate_run, ug._UltraZkeyLocateOptions, (C.byref(located),))):
        for size in (0, 8, 16, 48, 56, 64):
            rc, msg = _call(entry, struct(), size, extra)
            assert rc == 1
            if size != C.sizeof(struct):
                assert msg == "zkey: options struct of another size (%d)" % size, (entry, size)
            else:                                # its own size passes the options' rules and reaches the files
                assert "options struct" not in msg and msg


def test_max_listed_above_the_cap_is_refused():
    with pytest.raises(ug.SetupError, match="zkey: max_listed 1025 exceeds 1024"):
        ug.zkey_locate(*ZC.valid_case("fixture-delta-1"), device=-1, max_listed=1025)


# ------------------------------------------------------------------------------------------- the tool
def _tool(name, *args):
    return subprocess.run([os.path.join(CSRC, name)] + list(args) + ["--device", "-1"], capture_output=True, text=True)


def test_tool_locate_lines(tmp_path):
    r1cs, ptau, zkey, _, _ = LC.planted_cases()["two-sections-5-and-8"]
    h_other = LC.planted_cases()["h-of-another-delta-max-blocks-2"][2]
    paths = {}
    for name, data in (("c.r1cs", r1cs), ("p.ptau", ptau), ("k.zkey", zkey), ("h.zkey", h_other), ("ok.zkey", LC.chain_key())):
        paths[name] = str(tmp_path / name)
        open(paths[name], "wb").write(data)
    plain = _tool("zkey_verify", paths["c.r1cs"], paths["p.ptau"], paths["k.zkey"])
    assert plain.returncode == 1 and plain.stdout.count("\n") == 1 and plain.stdout.startswith("invalid: sections 5, 8 (parse ")
    located = _tool("zkey_verify", paths["c.r1cs"], paths["p.ptau"], paths["k.zkey"], "--locate")
    lines = located.stdout.splitlines()
    assert located.returncode == 1 and located.stderr == plain.stderr and lines[0].startswith("invalid: sections 5, 8 (parse ")
    assert lines[1:] == ["section 5: 1 of 593 records wrong: 17", "section 8: 2 of 591 records wrong: 300, 590"]
    listed = _tool("zkey_verify", paths["c.r1cs"], paths["p.ptau"], paths["h.zkey"], "--locate", "--max-listed", "3")
    assert listed.returncode == 1 and listed.stdout.splitlines()[1:] == ["section 9: 1 024 of 1 024 records wrong: 0, 1, 2, ..."]
    ok = _tool("zkey_verify", paths["c.r1cs"], paths["p.ptau"], paths["ok.zkey"], "--locate")
    assert ok.returncode == 0 and ok.stdout.count("\n") == 1 and ok.stdout.startswith("valid (parse ")
    bad = _tool("zkey_verify", paths["c.r1cs"], paths["p.ptau"], paths["ok.zkey"], "--max-listed", "0")
    assert bad.returncode == 2 and bad.stderr.startswith("Error: --max-listed takes 1 to 1024\n")


# ------------------------------------------------------------------------------------------- native
@pytest.fixture(scope="module")
def fuzz_locate(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz_zkey_locate"), "fuzz_zkey_locate",
                                 ["fuzz_zkey_locate.cpp", "zkey_verify_host.cpp", "setup_ptau.cpp", "point_check.cpp", "setup_host.cpp", "host_util.cpp"],
                                 flags=("-O2", "-pthread", "-Wno-unknown-pragmas"))


def test_mutated_files_never_crash_locating(fuzz_locate, tmp_path):
    """tests/native/fuzz_zkey_locate.cpp: the host path alone (no HIP code linked) under AddressSanitizer + UBSan, a stand-alone child
    process: a two-constraint circuit's key, .ptau and .r1cs, one of them mutated per turn, three turns in sixteen inside what
    locating reads (such a turn costs a hundred refusals). Every listed index must lie below its section's record count and the verify part of the answer must equal
    ug_zkey_verify_run's on the same bytes (the program aborts otherwise)."""
    from ultragroth_amd import synth
    rows = [({1: 1}, {2: 1}, {3: 1}), ({3: 1, 0: ZC.R - 1}, {2: 1}, {4: 5, 0: 7})]
    r1cs = synth.r1cs_file(5, 1, 1, rows)
    ptau = PC.ptau(3)
    zkey = ug.setup_from_ptau(r1cs, ptau, delta=ZC.FIXED_DELTA, device=-1)[0]
    for name, data in (("c.r1cs", r1cs), ("p.ptau", ptau), ("k.zkey", zkey)):
        open(tmp_path / name, "wb").write(data)
    r = subprocess.run([fuzz_locate, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau"), str(tmp_path / "k.zkey"), "1000", "20261021"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    m = re.fullmatch(r"(\d+) valid, (\d+) invalid, (\d+) refused, (\d+) sections located, 0 crashed\n", r.stdout)
    assert m and sum(int(g) for g in m.groups()[:3]) == 1000 and int(m.group(2)) > 30 and int(m.group(4)) > 30
