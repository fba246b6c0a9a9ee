"""The check of a Groth16 key against its circuit and a prepared powers-of-tau file on the device (zkey_verify.hip: the fold kernel,
the gather of H's sources, the MSMs of the existing engine), through ultragroth_amd.zkey_verify / r1cs_fold with device = 0. The
cases are tests/zkey_verify_cases.py's, the ones test_zkey_verify_host.py runs on host threads: what each of them must answer is
fixed there in advance, so the device and the host twin are held to the same verdict, failing sections and message; the fold is
also compared with the host's byte for byte."""
import pytest

import zkey_verify_cases as ZC

pytestmark = pytest.mark.gpu
R = ZC.R


def _ug():
    import ultragroth_amd as ug
    return ug


@pytest.mark.parametrize("name", ZC.FOLD_CASES)
def test_fold_equals_python_integers_and_the_host(name):
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case(name)
    rho = ZC.fold_rho(n_wires)
    log_n = ZC.log_domain_of(len(rows), n_public)
    timing = []
    got = ug.r1cs_fold(r1cs, rho, device=0, timing=timing)
    want = ZC.fold_reference(rows, n_public, rho, log_n)
    for v, label in enumerate(("a_pub", "b_pub", "c_pub", "a_priv", "b_priv", "c_priv")):
        assert got[v] == want[v], label
    assert got == ug.r1cs_fold(r1cs, rho, device=-1)
    assert len(timing) == 1 and timing[0] > 0
    m = len(rows)
    assert got[0][m:m + n_public + 1] == [x % R for x in rho[:n_public + 1]]
    for v in range(6):
        assert not any(got[v][m + n_public + 1:]) and (v == 0 or not any(got[v][m:]))


def test_fold_in_a_larger_domain():
    ug = _ug()
    n_wires, n_public, rows, r1cs = ZC.fold_case("odd-1-2")
    rho = ZC.fold_rho(n_wires)
    assert ug.r1cs_fold(r1cs, rho, log_domain=9, device=0) == ZC.fold_reference(rows, n_public, rho, 9)


@pytest.mark.parametrize("case", [c[0] for c in ZC.VALID])
def test_valid_keys_are_accepted(case):
    ug = _ug()
    r1cs, ptau, zkey = ZC.valid_case(case)
    timings = {}
    assert ug.zkey_verify(r1cs, ptau, zkey, device=0, timings=timings) is None
    assert timings["subgroup_checked"] is True and timings["peak_device_bytes"] > 0 and timings["fold_kernel"] > 0


@pytest.mark.parametrize("case", ZC.INVALID_IDS)
def test_one_planted_change_fails_exactly_its_sections(case):
    ug = _ug()
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case]
    got = ug.zkey_verify(r1cs, ptau, zkey, device=0)
    assert got == (first, failing, message)
    assert got == ug.zkey_verify(r1cs, ptau, zkey, device=-1)


@pytest.mark.parametrize("case", ZC.COMPOUND_IDS + ZC.HEADER_ORDER_IDS)
def test_several_planted_changes_and_the_header_rules_order(case):
    ug = _ug()
    r1cs, ptau, zkey, failing, first, message = ZC.invalid_cases()[case]
    got = ug.zkey_verify(r1cs, ptau, zkey, device=0)
    assert got == (first, failing, message)
    assert got == ug.zkey_verify(r1cs, ptau, zkey, device=-1)


@pytest.mark.parametrize("case", ZC.REFUSAL_IDS)
def test_refusals(case):
    ug = _ug()
    r1cs, ptau, zkey, text = ZC.refusals()[case]
    with pytest.raises(ug.SetupError) as e:
        ug.zkey_verify(r1cs, ptau, zkey, device=0)
    assert text in str(e.value), str(e.value)
    with pytest.raises(ug.SetupError) as host:
        ug.zkey_verify(r1cs, ptau, zkey, device=-1)
    assert str(host.value) == str(e.value)


def test_level_1_lets_the_off_subgroup_point_through_to_the_relations():
    ug = _ug()
    r1cs, ptau, bad, _ = ZC.refusals()["b2-off-subgroup"]
    timings = {}
    assert ug.zkey_verify(r1cs, ptau, bad, device=0, validate=1, timings=timings) == (7, [7], ZC.section_message(7))
    assert timings["subgroup_checked"] is False
