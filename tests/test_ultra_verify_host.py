"""Checking an UltraGroth key against its circuit and powers of tau on host threads (device = -1): include/ultragroth_hip.h
ug_ultra_zkey_verify_run / ug_r1cs_fold_classes through ultragroth_amd.ultra_zkey_verify / r1cs_fold_classes and the
zkey_verify_ultra tool. The references: Python integers for the fold; for a verdict, how the key was made (ultra_keys_cases.py):
a key of ultra_setup_from_ptau or dev_setup's own is valid, every invalid key is ONE planted change whose failing sections and
message are known in advance."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ultra_keys_cases as UC
import zkey_verify_cases as ZC

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = SC.R


def _ug():
    import ultragroth_amd as ug
    return ug


# ------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("kind", UC.CLASS_MAPS)
@pytest.mark.parametrize("name", ZC.FOLD_CASES)
def test_fold_classes_against_python_integers(name, kind):
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case(name)
    rho, cls = ZC.fold_rho(n_wires), UC.class_map(n_wires, n_public, kind)
    log_n = ZC.log_domain_of(len(rows), n_public)
    got = ug.r1cs_fold_classes(r1cs, rho, cls, device=-1)
    assert got == tuple(list(v) for v in UC.fold_classes_reference(rows, n_public, rho, cls, log_n))
    if kind == "all-final":                                  # no wire in class 1: r1cs_fold's six vectors and their sums
        six = ug.r1cs_fold(r1cs, rho, device=-1)
        assert (got[0], got[1], got[2], got[6], got[7], got[8]) == six
        assert all(not any(got[v]) for v in (3, 4, 5))
        assert got[9] == [(x + y) % R for x, y in zip(six[0], six[3])] and got[10] == [(x + y) % R for x, y in zip(six[1], six[4])]


def test_fold_classes_rules():
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case("odd-1-2")
    rho = ZC.fold_rho(n_wires)
    with pytest.raises(ug.SetupError, match="r1cs: class 3 of wire 5 is not 0, 1 or 2"):
        ug.r1cs_fold_classes(r1cs, rho, [0] * 5 + [3] + [1] * (n_wires - 6), device=-1)
    with pytest.raises(ug.SetupError, match="r1cs: cls takes one class per wire"):
        ug.r1cs_fold_classes(r1cs, rho, [0] * (n_wires - 1), device=-1)
    wide = ug.r1cs_fold_classes(r1cs, rho, UC.class_map(n_wires, n_public, "random"), log_domain=7, device=-1)
    assert len(wide[0]) == 128 and not any(wide[9][len(rows) + n_public + 1:])


# ------------------------------------------------------------------------------------------- verdicts
@pytest.mark.parametrize("case_id", UC.VALID_IDS)
def test_valid_keys_are_accepted(case_id):
    ug = _ug()
    r1cs, ptau, zkey, spec = UC.valid_case(case_id)
    timings = {}
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, device=-1, timings=timings) is None
    assert timings["subgroup_checked"] is True and set(ug.ZKEY_VERIFY_PHASES) <= set(timings)
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1) is None


@pytest.mark.parametrize("case_id", UC.INVALID_IDS)
def test_invalid_keys_fail_exactly_the_named_sections(case_id):
    ug = _ug()
    r1cs, ptau, zkey, spec, failing, first, message = UC.invalid_cases()[case_id]
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1) == (first, failing, message)


@pytest.mark.parametrize("case_id", UC.COMPOUND_IDS)
def test_several_planted_changes_report_every_section_and_the_first_relation(case_id):
    ug = _ug()
    r1cs, ptau, zkey, spec, failing, first, message = UC.invalid_cases()[case_id]
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1) == (first, failing, message)


@pytest.mark.parametrize("case_id", UC.HEADER_ORDER_IDS)
def test_header_rules_are_tried_in_their_order(case_id):
    """two header rules broken at once: the message is the earlier rule's -- gamma2 at infinity comes before the deltas"""
    ug = _ug()
    r1cs, ptau, zkey, spec, failing, first, message = UC.invalid_cases()[case_id]
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1) == (first, failing, message)


@pytest.mark.parametrize("case_id", UC.REFUSAL_IDS)
def test_refusals(case_id):
    ug = _ug()
    r1cs, ptau, zkey, validate, text = UC.refusals()[case_id]
    with pytest.raises(ug.SetupError) as e:
        ug.ultra_zkey_verify(r1cs, ptau, zkey, device=-1, validate=validate)
    assert text in str(e.value), str(e.value)


def test_level_1_says_that_the_subgroup_was_not_checked():
    ug = _ug()
    r1cs, ptau, zkey, _ = UC.valid_case("alternating")
    timings = {}
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, device=-1, validate=1, timings=timings) is None
    assert timings["subgroup_checked"] is False
    for validate in (0, 3):
        with pytest.raises(ug.SetupError, match="zkey: validate %d is not 1 or 2" % validate):
            ug.ultra_zkey_verify(r1cs, ptau, zkey, device=-1, validate=validate)
    with pytest.raises(ug.SetupError, match="zkey: a signal of the spec is not below 2\\^32"):
        ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra={"rand_indx": 1 << 32, "round_signals": [], "final_signals": []}, device=-1)


def test_the_groth16_check_and_the_ultragroth_check_refuse_each_other_s_keys():
    ug = _ug()
    r1cs, ptau, zkey, _ = UC.valid_case("golden-own-gamma")
    with pytest.raises(ug.SetupError, match="zkey: protocol 1337 keys are not checked"):
        ug.zkey_verify(r1cs, ptau, zkey, device=-1)
    with pytest.raises(ug.SetupError, match="zkey: zkey file is not ultragroth"):
        ug.ultra_zkey_verify(r1cs, ptau, RC.golden("groth16.zkey"), device=-1)


# ------------------------------------------------------------------------------------------- ABI
def test_the_new_symbols_are_declared_exported_and_mirrored():
    ug = _ug()
    from ultragroth_amd import _lib
    lib = ug.load()
    header = open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ug_ultra_zkey_verify_run", "ug_r1cs_fold_classes", "ug_r1cs_fold_classes_dvec"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.INNER_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(ug._UltraZkeyVerifyOptions) == 16 + 32 == 48
    r1cs, ptau, zkey, _ = UC.valid_case("alternating")
    opt = ug._UltraZkeyVerifyOptions()
    opt.size = 47
    err = C.create_string_buffer(256)
    rep = ug._ZkeyVerifyReport()
    assert lib.ug_ultra_zkey_verify_run(C.byref(opt), r1cs, len(r1cs), ptau, len(ptau), zkey, len(zkey), -1, C.byref(rep), None, err, 255) == 1
    assert err.value == b"zkey: options struct of another size (47)"


# ------------------------------------------------------------------------------------------- the tool
def test_cli_exit_codes(tmp_path):
    """zkey_verify_ultra on host threads: 0 valid, 1 invalid with the sections on stdout and the message on stderr, 2 refused"""
    r1cs, ptau, zkey, spec = UC.valid_case("alternating")
    bad = UC.invalid_cases()["h-under-delta-round"][2]
    groth = UC.refusals()["groth16-key"][2]
    for name, data in (("c.r1cs", r1cs), ("p.ptau", ptau), ("k.zkey", zkey), ("bad.zkey", bad), ("g.zkey", groth)):
        (tmp_path / name).write_bytes(data)
    (tmp_path / "s.json").write_text(json.dumps(spec))
    (tmp_path / "other.json").write_text(json.dumps(UC.irregular("descending")[1]))
    exe = os.path.join(CSRC, "zkey_verify_ultra")
    run = lambda key, *more: subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau"), str(tmp_path / key), "--device", "-1"] + list(more),
                                            capture_output=True, text=True, timeout=120)
    r = run("k.zkey")
    assert r.returncode == 0 and r.stdout.startswith("valid ("), (r.stdout, r.stderr)
    r = run("k.zkey", "--spec", str(tmp_path / "s.json"))
    assert r.returncode == 0 and r.stdout.startswith("valid ("), (r.stdout, r.stderr)
    r = run("k.zkey", "--validate", "1")
    assert r.returncode == 0 and r.stdout.startswith("relations hold, subgroup not checked"), r.stdout
    r = run("bad.zkey")
    assert r.returncode == 1 and r.stdout.startswith("invalid: sections 12 (") and UC.section_message(12) in r.stderr, (r.stdout, r.stderr)
    r = run("k.zkey", "--spec", str(tmp_path / "other.json"))
    assert r.returncode == 1 and r.stdout.startswith("invalid: sections 10, 11 ("), r.stdout
    r = run("g.zkey")
    assert r.returncode == 2 and r.stdout == "refused\n" and "Error: zkey: zkey file is not ultragroth" in r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "Usage: zkey_verify_ultra" in r.stderr
