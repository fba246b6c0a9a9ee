"""ug_groth16_verify_batch_records / ug_ultra_groth_verify_batch_records on the device: records_ingest_kernel, the subgroup ladder in
its mask form, the gather kernel and the resident form of the Miller pass (pairing.hip, check.hip). Proofs are prove_batch's, packed
by ug_proof_pack; every expected verdict is the single verifier's on the text the record stands for."""
import json

import pytest

from oracle import pairing as PR
import verify_batch_cases as VB
import verify_records_cases as VR
from verify_batch_cases import VALID, INVALID

pytestmark = pytest.mark.gpu


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
    proofs, pubs = _prove(ug.Groth16Prover, VB.load("groth16.zkey"), VB.load("groth16.wtns"), 130)
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert len(set(recs)) == 130 and VR.expected(False, recs, blocks, vk) == [VALID] * 130
    return proofs, pubs, recs, blocks, vk


@pytest.fixture(scope="module")
def ultra(device):
    import ultragroth_amd as ug
    vk = json.loads(VB.load("ultra_vkey.json", "r"))
    proofs, pubs = _prove(ug.UltraGrothProver, VB.load("ultra.zkey"), VB.load("ultra.uwtns"), 65)
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert VR.expected(True, recs, blocks, vk) == [VALID] * 65
    return proofs, pubs, recs, blocks, vk


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_valid_and_one_bad(g16, count):
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = list(recs[:count]), list(blocks[:count])
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk, device=0)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * count)
    assert stats["batch_checks"] == 1 and stats["single_checks"] == 0 and stats["device_ms"] > 0
    assert VR.passes() == (1, 0)                                                  # nothing dropped: the arrays in place
    at = count - 1
    recs[at], blocks[at] = VR.bad_record("signal+1", proofs[at], pubs[at])
    expect = [VALID] * count
    expect[at] = VR.single(False, recs[at], blocks[at], vk)
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk, device=0)
    assert expect[at] == INVALID and rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at
    VB.check_bound(count, 1, stats)


@pytest.mark.parametrize("kind", VR.KINDS + VR.BINARY_KINDS)
def test_kinds_of_bad_record(g16, kind):
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = list(recs[:65]), list(blocks[:65])
    if kind in VR.KINDS:
        recs[64], blocks[64] = VR.bad_record(kind, proofs[64], pubs[64])
    else:
        recs[64], blocks[64] = VR.binary_record(kind, recs[64], blocks[64])
    expect = [VALID] * 64 + [VR.single(False, recs[64], blocks[64], vk)]
    if kind in VR.KINDS:
        assert expect[64] == INVALID
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk, device=0)
    assert verdicts == expect and rc == expect[64]
    dropped = kind in ("B off subgroup", "C off curve")                           # left the batch before the Miller pass: the gather ran
    if kind in VR.KINDS:
        assert VR.passes() == ((0, 1) if dropped else (1, 0))
    if kind == "B off subgroup":
        assert stats["off_subgroup"] == 1 and stats["single_checks"] == 1 and stats["batch_checks"] == 1
    if kind == "C off curve":
        assert stats["off_subgroup"] == 0 and stats["single_checks"] == 0 and stats["batch_checks"] == 1


def test_cancelling_pair(g16):
    proofs, pubs, recs, blocks, vk = g16
    recs = list(recs[:65])
    a, b = VB.cancelling_pair(proofs[0], proofs[64])
    recs[0], recs[64] = VR.pack(a), VR.pack(b)
    expect = VR.expected(False, [recs[0], recs[64]], [blocks[0], blocks[64]], vk)
    assert expect == [INVALID, INVALID]
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks[:65], vk, device=0)
    assert rc == INVALID and verdicts == [INVALID] + [VALID] * 63 + [INVALID]
    VB.check_bound(65, 2, stats)


def test_many_off_subgroup_records(g16):
    """65 records whose every pi_b is off the subgroup: one ladder launch names them all"""
    proofs, pubs, recs, blocks, vk = g16
    pairs = [VR.bad_record("B off subgroup", proofs[i], pubs[i]) for i in range(65)]
    recs, blocks = [r for r, _ in pairs], [b for _, b in pairs]
    expect = VR.expected(False, recs, blocks, vk)
    assert expect == [INVALID] * 65
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk, device=0, opt=VR.options(0))
    assert rc == INVALID and verdicts == expect and stats["off_subgroup"] == 65 and stats["single_checks"] == 65 and stats["judged"] == 0
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk, device=0, opt=VR.options(1, judge_min=1))
    assert rc == INVALID and verdicts == expect and stats["off_subgroup"] == 65 and stats["judged"] == 65 and stats["single_checks"] == 0
    rc, msg, verdicts, stats = VR.batch_json_opt(False, [VR.unpack(r) for r in recs], [VR.unpack_inputs(b) for b in blocks], vk, device=0,
                                                 opt=VR.options(0))          # the JSON path: step 2 is one call of the mask form too
    assert verdicts == expect and stats["off_subgroup"] == 65


def test_f_equals_the_host_miller_loop(g16):
    """every f_i of a 65-record pass: miller(B_i, r_i A_i) of the host on the REDUCED points, limb for limb; two records carry a
    coordinate + q, so the ingest kernel's reduction is on the compared path"""
    proofs, pubs, recs, blocks, vk = g16
    recs = list(recs[:65])
    recs[3] = VR.binary_record("pi_a.x + q", recs[3], blocks[3])[0]
    recs[40] = VR.binary_record("pi_b.y.c1 + q", recs[40], blocks[40])[0]
    assert VR._get(recs[3], 0) >= VR.Q and VR._get(recs[40], 160) >= VR.Q
    expect = VR.expected(False, recs, blocks[:65], vk)
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks[:65], vk, device=0)
    assert verdicts == expect == [VALID] * 65
    scalars = set()
    for i in range(65):
        r, f = VB.trace(i)
        scalars.add(r)
        p = json.loads(proofs[i])
        ra = PR.g1_mul((int(p["pi_a"][0]), int(p["pi_a"][1])), r)
        assert f == VB.product_miller(VB.g1_rec(ra), VB.g2_rec(p["pi_b"])), i
    assert len(scalars) == 65


def test_device_host_and_json_agree(g16):
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = list(recs), list(blocks)
    for at, kind in ((0, "A.y negated"), (63, "C off curve"), (64, "C = generator"), (100, "B off subgroup"), (129, "A = infinity")):
        recs[at], blocks[at] = VR.bad_record(kind, proofs[at], pubs[at])
    expect = VR.expected(False, recs, blocks, vk)
    assert [i for i, v in enumerate(expect) if v != VALID] == [0, 63, 64, 100, 129]
    dev = VR.batch_records(False, recs, blocks, vk, device=0)
    assert VR.passes() == (0, 1)                                                  # records 63 and 100 left the batch: gathered
    host = VR.batch_records(False, recs, blocks, vk, device=-1)
    text = VR.batch_json_opt(False, [VR.unpack(r) for r in recs], [VR.unpack_inputs(b) for b in blocks], vk, device=0)
    assert dev[:3] == host[:3] == text[:3] == (INVALID, "proof 0: invalid proof", expect)
    assert dev[3]["off_subgroup"] == host[3]["off_subgroup"] == text[3]["off_subgroup"] == 1


def test_across_a_pass(g16):
    """2^16 + 1 records: the second pass is the one bad record"""
    proofs, pubs, recs, blocks, vk = g16
    n = (1 << 16) + 1
    many_r, many_b = (recs * (n // 130 + 1))[:n], (blocks * (n // 130 + 1))[:n]
    many_r[n - 1], many_b[n - 1] = VR.bad_record("signal+1", proofs[(n - 1) % 130], pubs[(n - 1) % 130])
    assert VR.single(False, many_r[n - 1], many_b[n - 1], vk) == INVALID
    rc, msg, verdicts, stats = VR.batch_records(False, many_r, many_b, vk, device=0)
    assert rc == INVALID and msg == "proof %d: invalid proof" % (n - 1)
    assert verdicts == [VALID] * (n - 1) + [INVALID]
    assert stats["batch_checks"] == 2 and stats["single_checks"] == 1            # one root check per pass; check_bound(1, 1) for the second
    assert VR.passes() == (2, 0)


@pytest.mark.parametrize("count", [1, 65])
def test_ultragroth(ultra, count):
    proofs, pubs, recs, blocks, vk = ultra
    recs, blocks = list(recs[:count]), list(blocks[:count])
    rc, msg, verdicts, stats = VR.batch_records(True, recs, blocks, vk, device=0)
    assert (rc, verdicts, stats["batch_checks"], stats["single_checks"]) == (VALID, [VALID] * count, 1, 0)
    last = count - 1
    recs[last] = recs[last][:256] + ultra[2][(last + 1) % 65][256:]               # another proof's round commitment
    if count > 1:
        a, b = VB.cancelling_pair(proofs[0], proofs[33], ultra=True)
        recs[0], recs[33] = VR.pack(a, True), VR.pack(b, True)
    bad = {last} | ({0, 33} if count > 1 else set())
    expect = [VR.single(True, recs[i], blocks[i], vk) if i in bad else VALID for i in range(count)]
    assert all(expect[i] == INVALID for i in bad)
    rc, msg, verdicts, stats = VR.batch_records(True, recs, blocks, vk, device=0)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(count, len(bad), stats)
    if count > 1:
        i = 7                                                                     # the device's f of an UltraGroth record as well
        r, f = VB.trace(i)
        p = json.loads(proofs[i])
        assert f == VB.product_miller(VB.g1_rec(PR.g1_mul((int(p["pi_a"][0]), int(p["pi_a"][1])), r)), VB.g2_rec(p["pi_b"]))


def test_python_entry_points(g16, device):
    import ultragroth_amd as ug
    proofs, pubs, recs, blocks, vk = g16
    n_pub = len(blocks[0]) // 32
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(recs[:5]), b"".join(blocks[:5]), n_pub, vk)
    assert verdicts == [VALID] * 5 and stats["device_ms"] > 0 and stats["judged"] == 0
    bad = VR.bad_record("C = generator", proofs[2], pubs[2])
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(recs[:2]) + bad[0], b"".join(blocks[:2]) + bad[1], n_pub, vk, judge=True, judge_min=1)
    assert verdicts == [VALID, VALID, INVALID] and stats["judged"] >= 1
