"""Checking an UltraGroth key on the device: the fold with a class per wire (r1cs_fold_classes_kernel) and the MSMs of the relations,
through ultragroth_amd.ultra_zkey_verify / r1cs_fold_classes with device = 0. The references are those of
tests/test_ultra_verify_host.py: Python integers for the fold, and for every verdict the host path's (device = -1), which that file
holds against how each key was made."""
import pytest

import ultra_keys_cases as UC
import zkey_verify_cases as ZC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", UC.CLASS_MAPS)
@pytest.mark.parametrize("name", ZC.FOLD_CASES)
def test_fold_classes_against_python_integers(device, name, kind):
    import ultragroth_amd as ug
    n_wires, n_public, rows, r1cs = ZC.fold_case(name)
    rho, cls = ZC.fold_rho(n_wires), UC.class_map(n_wires, n_public, kind)
    timing = []
    got = ug.r1cs_fold_classes(r1cs, rho, cls, device=0, timing=timing)
    assert got == tuple(list(v) for v in UC.fold_classes_reference(rows, n_public, rho, cls, ZC.log_domain_of(len(rows), n_public)))
    assert got == ug.r1cs_fold_classes(r1cs, rho, cls, device=-1) and timing[0] >= 0
    if kind == "all-final":
        six = ug.r1cs_fold(r1cs, rho, device=0)
        assert (got[0], got[1], got[2], got[6], got[7], got[8]) == six


def test_fold_classes_in_a_wider_domain(device):
    import ultragroth_amd as ug
    n_wires, n_public, rows, r1cs = ZC.fold_case("odd-1-2")
    rho, cls = ZC.fold_rho(n_wires), UC.class_map(n_wires, n_public, "random")
    assert ug.r1cs_fold_classes(r1cs, rho, cls, log_domain=9, device=0) == ug.r1cs_fold_classes(r1cs, rho, cls, log_domain=9, device=-1)


@pytest.mark.parametrize("case_id", UC.VALID_IDS)
def test_valid_keys_are_accepted(device, case_id):
    import ultragroth_amd as ug
    r1cs, ptau, zkey, spec = UC.valid_case(case_id)
    timings = {}
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=0, timings=timings) is None
    assert timings["subgroup_checked"] is True and timings["peak_device_bytes"] > 0 and timings["fold_kernel"] >= 0


@pytest.mark.parametrize("case_id", UC.INVALID_IDS)
def test_invalid_keys_get_the_host_path_s_verdict(device, case_id):
    import ultragroth_amd as ug
    r1cs, ptau, zkey, spec, failing, first, message = UC.invalid_cases()[case_id]
    got = ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=0)
    assert got == (first, failing, message)
    assert got == ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1)


@pytest.mark.parametrize("case_id", UC.COMPOUND_IDS + UC.HEADER_ORDER_IDS)
def test_several_planted_changes_and_the_header_rules_order(device, case_id):
    import ultragroth_amd as ug
    r1cs, ptau, zkey, spec, failing, first, message = UC.invalid_cases()[case_id]
    got = ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=0)
    assert got == (first, failing, message)
    assert got == ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=-1)


@pytest.mark.parametrize("case_id", UC.REFUSAL_IDS)
def test_refusals(device, case_id):
    import ultragroth_amd as ug
    r1cs, ptau, zkey, validate, text = UC.refusals()[case_id]
    with pytest.raises(ug.SetupError) as e:
        ug.ultra_zkey_verify(r1cs, ptau, zkey, device=0, validate=validate)
    assert text in str(e.value), str(e.value)


def test_long_column_key_and_level_1(device):
    import setup_ptau_cases as PC
    import ultragroth_amd as ug
    r1cs, spec = UC.long_column()
    ptau = PC.ptau(10, device=0)
    zkey = ug.ultra_setup_from_ptau(r1cs, ptau, spec, delta="draw", device=0)[0]
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, ultra=spec, device=0) is None
    timings = {}
    assert ug.ultra_zkey_verify(r1cs, ptau, zkey, device=0, validate=1, timings=timings) is None and timings["subgroup_checked"] is False
