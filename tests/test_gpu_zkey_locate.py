"""Naming the wrong records of a failing section on the device (ug_zkey_locate_run, ug_ultra_zkey_locate_run with device >= 0: the
expected records through the combination kernels, the ratio test through ratio_block_sums_kernel and ratio_judge_kernel). The
answers are those zkey_locate_cases.py fixes in advance, and the host twin's, field for field."""
import pytest

import setup_ptau_cases as PC
import zkey_locate_cases as LC
import zkey_verify_cases as ZC
import ultragroth_amd as ug

pytestmark = pytest.mark.gpu


def test_valid_keys_locate_nothing():
    timings = {}
    assert ug.zkey_locate(*ZC.valid_case("fixture-fixed-delta"), device=0, timings=timings) is None and timings["locate"] == 0
    assert ug.zkey_locate(*ZC.valid_case("dev-setup-own-gamma"), device=0) is None
    assert ug.zkey_locate(LC.chain()[3], PC.ptau(LC.CHAIN_POWER), LC.chain_key(), device=0) is None
    assert ug.ultra_zkey_locate(LC.chain()[3], PC.ptau(LC.CHAIN_POWER), LC.ultra_chain_key(), ultra=LC.chain_spec(), device=0) is None


@pytest.mark.parametrize("case_id", LC.GPU_PLANTED_IDS)
def test_planted_changes_are_named(case_id):
    LC.check_planted(case_id, 0)


@pytest.mark.parametrize("case_id", LC.ULTRA_IDS)
def test_ultragroth_sections(case_id):
    LC.check_ultra(case_id, 0)


@pytest.mark.parametrize("case_id", ("two-sections-5-and-8", "h-of-another-delta-max-blocks-2"))
def test_device_against_host(case_id):
    r1cs, ptau, zkey, _, kw = LC.planted_cases()[case_id]
    strip = lambda got: got[:3] + ({s: {k: v for k, v in e.items() if k != "kernel_ms"} for s, e in got[3].items()},)
    dev = ug.zkey_locate(r1cs, ptau, zkey, device=0, **kw)
    assert strip(dev) == strip(ug.zkey_locate(r1cs, ptau, zkey, device=-1, **kw))
    assert all(e["kernel_ms"][0] > 0 and e["kernel_ms"][1] > 0 for e in dev[3].values() if e["method"] == "ratio")


def test_refusals_are_the_verify_entrys():
    for case_id in ("b2-off-subgroup", "truncated-section-8"):
        r1cs, ptau, zkey, text = ZC.refusals()[case_id]
        with pytest.raises(ug.SetupError) as e:
            ug.zkey_locate(r1cs, ptau, zkey, device=0)
        assert text in str(e.value)
