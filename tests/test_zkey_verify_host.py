"""The check of a Groth16 key against its circuit and a prepared powers-of-tau file on host threads (device = -1):
include/ultragroth_hip.h ug_zkey_verify_run and ug_r1cs_fold through ultragroth_amd.zkey_verify / r1cs_fold, and the tool. The
cases and what each of them must answer are tests/zkey_verify_cases.py's; test_gpu_zkey_verify.py asks the device the same."""
import os
import subprocess

import pytest

from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import zkey_verify_cases as ZC

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = ZC.R


def _ug():
    import ultragroth_amd as ug
    return ug


# ------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("name", ZC.FOLD_CASES)
def test_fold_equals_python_integers(name):
    """one lane, the last lane of a block, a block boundary and one row past it; no public wire and three; the public rows carry
    rho_s mod r, the rows above them nothing"""
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case(name)
    rho = ZC.fold_rho(n_wires)
    assert {0, 1, (1 << 128) - 1} <= set(rho) and any(x >= R for x in rho)
    log_n = ZC.log_domain_of(len(rows), n_public)
    got = ug.r1cs_fold(r1cs, rho, device=-1)
    want = ZC.fold_reference(rows, n_public, rho, log_n)
    assert len(got) == 6 and all(len(v) == 1 << log_n for v in got)
    for v, label in enumerate(("a_pub", "b_pub", "c_pub", "a_priv", "b_priv", "c_priv")):
        assert got[v] == want[v], label
    m = len(rows)
    assert got[0][m:m + n_public + 1] == [x % R for x in rho[:n_public + 1]]
    for v in range(6):
        assert not any(got[v][m + n_public + 1:]) and (v == 0 or not any(got[v][m:]))


def test_fold_in_a_larger_domain_and_its_refusals():
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case("odd-1-2")
    rho = ZC.fold_rho(n_wires)
    assert ug.r1cs_fold(r1cs, rho, log_domain=7, device=-1) == ZC.fold_reference(rows, n_public, rho, 7)
    for call, text in ((lambda: ug.r1cs_fold(r1cs, rho, log_domain=4, device=-1), "r1cs: log_domain 4 is too small"),
                       (lambda: ug.r1cs_fold(r1cs, rho[:-1], device=-1), "r1cs: rho takes one integer"),
                       (lambda: ug.r1cs_fold(r1cs[:-7], rho, device=-1), "r1cs: Section")):
        with pytest.raises(ug.SetupError) as e:
            call()
        assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------- verdicts
@pytest.mark.parametrize("case", [c[0] for c in ZC.VALID])
def test_valid_keys_are_accepted(case):
    ug = _ug()
    r1cs, ptau, zkey = ZC.valid_case(case)
    timings = {}
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1, timings=timings) is None
    assert timings["subgroup_checked"] is True and set(ug.ZKEY_VERIFY_PHASES) <= set(timings)


@pytest.mark.parametrize("case", ZC.INVALID_IDS)
def test_one_planted_change_fails_exactly_its_sections(case):
    ug = _ug()
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case]
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1) == (first, failing, message)


@pytest.mark.parametrize("case", ZC.COMPOUND_IDS)
def test_several_planted_changes_report_every_section_and_the_first_relation(case):
    ug = _ug()
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case]
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1) == (first, failing, message)


@pytest.mark.parametrize("case", ZC.HEADER_ORDER_IDS)
def test_header_rules_are_tried_in_their_order(case):
    """two header rules broken at once: the message is the earlier rule's -- delta1 / delta2 at infinity come before gamma2"""
    ug = _ug()
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case]
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1) == (first, failing, message)


def test_a_circuit_of_public_wires_only_has_an_empty_section_8():
    ug = _ug()
    r1cs, ptau, zkey = ZC.all_public_case()
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1) is None
    secs = dict(RC.sections(zkey))
    assert ug.zkey_verify(r1cs, ptau, PC.with_sections(zkey, {3: ZC.swapped(secs[3], 64)}), device=-1) == (3, [3], ZC.section_message(3))


@pytest.mark.parametrize("case", ZC.REFUSAL_IDS)
def test_refusals(case):
    ug = _ug()
    r1cs, ptau, zkey, text = ZC.refusals()[case]
    with pytest.raises(ug.SetupError) as e:
        ug.zkey_verify(r1cs, ptau, zkey, device=-1)
    assert text in str(e.value), str(e.value)


def test_level_1_says_that_the_subgroup_was_not_checked_and_lets_the_bad_point_through():
    """validate = 1 is for timing: the relations are evaluated, the report says that "valid" cannot be concluded"""
    ug = _ug()
    r1cs, ptau, zkey = ZC.valid_case("odd12-power-6")
    timings = {}
    assert ug.zkey_verify(r1cs, ptau, zkey, device=-1, validate=1, timings=timings) is None
    assert timings["subgroup_checked"] is False
    r1cs, ptau, bad, _ = ZC.refusals()["b2-off-subgroup"]
    assert ug.zkey_verify(r1cs, ptau, bad, device=-1, validate=1) == (7, [7], ZC.section_message(7))
    for level in (0, 3):
        with pytest.raises(ug.SetupError) as e:
            ug.zkey_verify(r1cs, ptau, zkey, device=-1, validate=level)
        assert "zkey: validate %d is not 1 or 2" % level in str(e.value)


def test_files_given_as_paths_and_two_planted_changes(tmp_path):
    """ptau and zkey as paths that the call maps; two sections changed at once are both reported, the message is the first's"""
    ug = _ug()
    r1cs, ptau, zkey = ZC.valid_case("odd12-power-6")
    (tmp_path / "p.ptau").write_bytes(ptau)
    (tmp_path / "k.zkey").write_bytes(zkey)
    assert ug.zkey_verify(r1cs, str(tmp_path / "p.ptau"), str(tmp_path / "k.zkey"), device=-1) is None
    secs = dict(RC.sections(zkey))
    both = PC.with_sections(zkey, {6: ZC.swapped(secs[6], 64), 9: ZC.swapped(secs[9], 64)})
    assert ug.zkey_verify(r1cs, memoryview(ptau), both, device=-1) == (6, [6, 9], ZC.section_message(6))


def test_cli_exit_codes(tmp_path):
    """zkey_verify <r1cs> <ptau> <zkey> on host threads: 0 valid, 1 invalid, 2 refused; one line on stdout, the message on stderr"""
    r1cs, ptau, zkey = ZC.valid_case("odd12-power-6")
    bad = ZC.invalid_cases()["swap-8"][2]
    odd = ZC.refusals()["truncated-section-8"][2]
    for name, data in (("c.r1cs", r1cs), ("p.ptau", ptau), ("k.zkey", zkey), ("bad.zkey", bad), ("odd.zkey", odd)):
        (tmp_path / name).write_bytes(data)
    exe = os.path.join(CSRC, "zkey_verify")
    run = lambda key, *more: subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau"), str(tmp_path / key), "--device", "-1"] + list(more),
                                            capture_output=True, text=True, timeout=120)
    r = run("k.zkey")
    assert r.returncode == 0 and r.stdout.startswith("valid (") and r.stdout.count("\n") == 1 and r.stderr == "", (r.stdout, r.stderr)
    r = run("k.zkey", "--validate", "1")
    assert r.returncode == 0 and r.stdout.startswith("relations hold, subgroup not checked ("), r.stdout
    r = run("bad.zkey")
    assert r.returncode == 1 and r.stdout.startswith("invalid: sections 8 (") and r.stderr.strip() == ZC.section_message(8), (r.stdout, r.stderr)
    r = run("odd.zkey")
    assert r.returncode == 2 and r.stdout == "refused\n" and "Error: zkey: Section 8 is shorter than the header implies" in r.stderr
    r = run("missing.zkey")
    assert r.returncode == 2 and r.stdout == "refused\n" and r.stderr.startswith("Error: ")


# ------------------------------------------------------------------------------------------- native
@pytest.fixture(scope="module")
def fuzz_verify(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz_zkey_verify"), "fuzz_zkey_verify",
                                 ["fuzz_zkey_verify.cpp", "zkey_verify_host.cpp", "setup_ptau.cpp", "point_check.cpp", "setup_host.cpp", "host_util.cpp"],
                                 flags=("-O2", "-pthread", "-Wno-unknown-pragmas"))


def test_mutated_files_never_crash_the_check(fuzz_verify, tmp_path):
    """tests/native/fuzz_zkey_verify.cpp: the host path alone (no HIP code linked) under AddressSanitizer + UBSan, a stand-alone
    child process: a two-constraint circuit's key, .ptau and .r1cs, one of them mutated per turn. (A turn that reaches the
    pairings takes half a second under the sanitizers, which is what this test's minutes are made of.)"""
    ug = _ug()
    from ultragroth_amd import synth
    rows = [({1: 1}, {2: 1}, {3: 1}), ({3: 1, 0: R - 1}, {3: 1}, {4: 1, 1: 2})]
    r1cs = synth.r1cs_file(5, 1, 0, rows)
    ptau = PC.ptau(2)
    zkey = ug.setup_from_ptau(r1cs, ptau, delta=ZC.FIXED_DELTA, device=-1)[0]
    assert SC.zkey_header(zkey) == (5, 1, 4)
    for name, data in (("c.r1cs", r1cs), ("p.ptau", ptau), ("k.zkey", zkey)):
        (tmp_path / name).write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_verify, str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau"), str(tmp_path / "k.zkey"), "2000", "1"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 crashed")
    valid, invalid, refused = (int(r.stdout.split()[i]) for i in (0, 2, 4))
    assert valid + invalid + refused == 2000 and refused > 1000 and invalid > 20 and valid > 20
