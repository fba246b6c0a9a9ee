"""The EVM and COMPRESSED record layouts on the device: records_ingest_kernel<EVM>, records_decompress_kernel and fq2_sqrt_kernel
(pairing.hip) against the host's code limb for limb (the arithmetic is pairing.hpp's, compiled twice), and
ug_*_verify_batch_records_fmt against the single verifier and the PLAIN device call on the converted records. Proofs are
prove_batch's; the layouts are verify_formats_cases' Python, independent of the library."""
import json

import pytest

import verify_batch_cases as VB
import verify_records_cases as VR
import verify_formats_cases as VF
from verify_batch_cases import VALID, INVALID
from verify_formats_cases import PLAIN, EVM, COMPRESSED

pytestmark = pytest.mark.gpu
NAMES = {EVM: "evm", COMPRESSED: "compressed"}


def _prove(cls, zkey, wtns, count):
    out = []
    with cls(zkey) as p:
        while len(out) < count:
            out += p.prove_batch([wtns] * min(16, count - len(out)))
    return [a for a, _ in out], [b for _, b in out]


@pytest.fixture(scope="module")
def g16(device):
    import ultragroth_amd as ug
    vk = json.loads(VB.load("groth16_vkey.json", "r"))
    proofs, pubs = _prove(ug.Groth16Prover, VB.load("groth16.zkey"), VB.load("groth16.wtns"), 65)
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert len(set(recs)) == 65 and VR.expected(False, recs, blocks, vk) == [VALID] * 65
    return proofs, pubs, recs, blocks, vk


@pytest.fixture(scope="module")
def ultra(device):
    import ultragroth_amd as ug
    vk = json.loads(VB.load("ultra_vkey.json", "r"))
    proofs, pubs = _prove(ug.UltraGrothProver, VB.load("ultra.zkey"), VB.load("ultra.uwtns"), 65)
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert VR.expected(True, recs, blocks, vk) == [VALID] * 65
    return proofs, pubs, recs, blocks, vk


@pytest.fixture(scope="module")
def ingest_batches(g16, ultra):
    """130 records per protocol and layout, made once; the host's reading of them is the reference of every count"""
    out = {}
    for is_ultra in (False, True):
        recs = (ultra if is_ultra else g16)[2]
        for fmt in (EVM, COMPRESSED):
            batch = VF.ingest_batch(fmt, recs, is_ultra, 130)
            out[is_ultra, fmt] = (batch,) + VF.ingest(-1, fmt, is_ultra, batch)
    return out


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("is_ultra", [False, True])
@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
def test_ingest_equals_the_host(ingest_batches, fmt, is_ultra, count):
    batch, host_plain, host_status = ingest_batches[is_ultra, fmt]
    plain, status = VF.ingest(0, fmt, is_ultra, batch[:count])
    assert status == host_status[:count]
    assert plain == host_plain[:count]
    if count == 130:                                                              # the batch holds what it is meant to hold
        assert {VF.OK, VF.OFF_CURVE, VF.OFF_SUBGROUP} == set(host_status)
        k = 4 if is_ultra else 3
        for i in range(130):
            kind = i % 16
            assert host_status[i] == (VF.OFF_CURVE if 6 <= kind < 6 + k else VF.OFF_SUBGROUP if kind == 5 else VF.OK), i
            stands = VF.to_plain(fmt, batch[i], b"", is_ultra)[0]
            if host_status[i] != VF.OFF_CURVE:                                    # ... and the host reads it as the layout's description does
                assert host_plain[i] == stands, i
            elif fmt == COMPRESSED:
                assert stands is None
        assert any(p[:64] == bytes(64) for p in host_plain) and any(p[64:192] == bytes(128) for p in host_plain)


def test_fq2_sqrt_equals_the_host(device):
    values = VF.sqrt_inputs()
    host = VF.fq2_sqrt(-1, values)
    dev = VF.fq2_sqrt(0, values)
    assert dev == host
    VF.check_sqrt(values, *dev)


@pytest.mark.parametrize("is_ultra", [False, True])
@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
def test_valid_batch_in_place(g16, ultra, fmt, is_ultra):
    proofs, pubs, recs, blocks, vk = ultra if is_ultra else g16
    pairs = [VF.to_format(fmt, r, b) for r, b in zip(recs, blocks)]
    rc, msg, verdicts, stats = VF.batch_fmt(is_ultra, fmt, [r for r, _ in pairs], [b for _, b in pairs], vk, device=0)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * 65)
    assert stats["batch_checks"] == 1 and stats["single_checks"] == 0 and stats["device_ms"] > 0
    assert VR.passes() == (1, 0)                                                  # nothing dropped: the arrays in place


@pytest.mark.parametrize("is_ultra", [False, True])
@pytest.mark.parametrize("judge", [0, 1])
@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
def test_mixed_batch(g16, ultra, fmt, judge, is_ultra):
    proofs, pubs, recs, blocks, vk = ultra if is_ultra else g16
    out_r, out_b, stands, expect = VF.mixed(fmt, recs, blocks, proofs, pubs, vk, is_ultra)
    assert [i for i, v in enumerate(expect) if v != VALID] == [0, 15, 16, 31, 32] and expect.count(INVALID) == 5
    opt = VR.options(judge, judge_min=1)
    rc, msg, verdicts, stats = VF.batch_fmt(is_ultra, fmt, out_r, out_b, vk, device=0, opt=opt)
    assert VR.passes() == (0, 1)                                                  # records 15 and 31 left the batch: gathered
    rc_p, msg_p, verdicts_p, stats_p = VF.plain_call_on(is_ultra, stands, vk, device=0, opt=opt)
    assert (rc, msg, verdicts) == (rc_p, msg_p, verdicts_p) == (INVALID, "proof 0: invalid proof", expect)
    assert stats["off_subgroup"] == stats_p["off_subgroup"] == 1
    assert (stats["judged"] > 0) == (stats_p["judged"] > 0) == bool(judge)
    if judge:
        assert stats["judge_launches"] >= 1


def test_plain_through_the_fmt_symbol(g16):
    proofs, pubs, recs, blocks, vk = g16
    old = VR.batch_records(False, recs, blocks, vk, device=0)
    old_passes = VR.passes()
    new = VF.batch_fmt(False, PLAIN, recs, blocks, vk, device=0)
    assert VR.passes() == old_passes == (1, 0)
    assert old[:3] == new[:3] == (VALID, "", [VALID] * 65)
    bad_r, bad_b = VR.mixed_batch(recs, blocks, proofs, pubs)
    old = VR.batch_records(False, bad_r, bad_b, vk, device=0, opt=VR.options(0))
    old_passes = VR.passes()
    new = VF.batch_fmt(False, PLAIN, bad_r, bad_b, vk, device=0, opt=VR.options(0))
    assert VR.passes() == old_passes == (0, 1) and old[:3] == new[:3]
    for name in ("batch_checks", "single_checks", "off_subgroup", "judged", "judge_launches"):
        assert old[3][name] == new[3][name], name


def test_python_entry_points(g16, device):
    import ultragroth_amd as ug
    proofs, pubs, recs, blocks, vk = g16
    n_pub = len(blocks[0]) // 32
    comp = [ug.proof_record_convert(r, ug.RECORDS_PLAIN, ug.RECORDS_COMPRESSED) for r in recs[:5]]
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(comp), b"".join(blocks[:5]), n_pub, vk, format=ug.RECORDS_COMPRESSED)
    assert verdicts == [VALID] * 5 and stats["device_ms"] > 0
    comp[2] = VF.without_root(comp[2], 0)
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(comp), b"".join(blocks[:5]), n_pub, vk, format=ug.RECORDS_COMPRESSED)
    assert verdicts == [VALID, VALID, INVALID, VALID, VALID] and stats["single_checks"] == 0
