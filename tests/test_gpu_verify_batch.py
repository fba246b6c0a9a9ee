"""ug_groth16_verify_batch / ug_ultra_groth_verify_batch on the device (pairing.hip): the verdicts of the single-proof verifier
for batches that cross the lane, wave and workgroup boundaries and have odd trees, the kernels' f_i against the host's Miller loop
limb for limb, and agreement with the host-thread form of the protocol. Proofs are prove_batch's, with fresh blinding."""
import json

import pytest

from oracle import pairing as PR
import verify_batch_cases as VB
from verify_batch_cases import VALID, INVALID, ERROR

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
    assert len(set(proofs)) == 130
    assert all(VB.single(False, p, s, vk) == VALID for p, s in zip(proofs, pubs))
    return proofs, pubs, vk


@pytest.fixture(scope="module")
def ultra(device):
    import ultragroth_amd as ug
    vk = json.loads(VB.load("ultra_vkey.json", "r"))
    proofs, pubs = _prove(ug.UltraGrothProver, VB.load("ultra.zkey"), VB.load("ultra.uwtns"), 65)
    assert all(VB.single(True, p, s, vk) == VALID for p, s in zip(proofs, pubs))
    return proofs, pubs, vk


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_valid_and_one_bad(g16, count):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:count]), list(pubs[:count])
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk, device=0)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * count)
    assert stats["batch_checks"] == 1 and stats["single_checks"] == 0 and stats["device_ms"] > 0
    at = count - 1
    proofs[at], pubs[at] = VB.bad_proof("signal+1", proofs[at], pubs[at])
    expect = [VALID] * count
    expect[at] = VB.single(False, proofs[at], pubs[at], vk)
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk, device=0)
    assert expect[at] == INVALID and rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at
    VB.check_bound(count, 1, stats)


@pytest.mark.parametrize("kind", VB.KINDS)
def test_kinds_of_bad_proof(g16, kind):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:65]), list(pubs[:65])
    proofs[64], pubs[64] = VB.bad_proof(kind, proofs[64], pubs[64])
    expect = [VALID] * 64 + [VB.single(False, proofs[64], pubs[64], vk)]
    assert expect[64] == (ERROR if kind in ("json syntax", "signal count") else INVALID)
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk, device=0)
    assert rc == INVALID and verdicts == expect
    if kind == "B off subgroup":                                                  # found by the device's subgroup ladder
        assert stats["off_subgroup"] == 1 and stats["single_checks"] == 1 and stats["batch_checks"] == 1


def test_cancelling_pair(g16):
    proofs, pubs, vk = g16
    proofs = list(proofs[:65])
    proofs[0], proofs[64] = VB.cancelling_pair(proofs[0], proofs[64])
    expect = [VB.single(False, proofs[i], pubs[i], vk) if i in (0, 64) else VALID for i in range(65)]
    assert expect[0] == INVALID and expect[64] == INVALID
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs[:65], vk, device=0)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(65, 2, stats)


def test_f_equals_the_host_miller_loop(g16):
    """every f_i of a 65-proof device pass, with the scalars the pass drew: miller(B_i, r_i A_i) of the host, limb for limb"""
    proofs, pubs, vk = g16
    assert VB.batch(False, proofs[:65], pubs[:65], vk, device=0)[0] == VALID
    scalars = set()
    for i in range(65):
        r, f = VB.trace(i)
        scalars.add(r)
        p = json.loads(proofs[i])
        ra = PR.g1_mul((int(p["pi_a"][0]), int(p["pi_a"][1])), r)
        assert f == VB.product_miller(VB.g1_rec(ra), VB.g2_rec(p["pi_b"])), i
    assert len(scalars) == 65


@pytest.mark.parametrize("count", [1, 65])
def test_ultragroth(ultra, count):
    proofs, pubs, vk = ultra
    proofs, pubs = list(proofs[:count]), list(pubs[:count])
    rc, msg, verdicts, stats = VB.batch(True, proofs, pubs, vk, device=0)
    assert (rc, verdicts, stats["batch_checks"], stats["single_checks"]) == (VALID, [VALID] * count, 1, 0)
    last = count - 1
    mixed = json.loads(proofs[last])
    mixed["pi_r"] = json.loads(ultra[0][(last + 1) % 65])["pi_r"]                 # another proof's round commitment
    proofs[last] = json.dumps(mixed)
    if count > 1:
        proofs[0], proofs[33] = VB.cancelling_pair(proofs[0], proofs[33], ultra=True)
    bad = {last} | ({0, 33} if count > 1 else set())
    expect = [VB.single(True, proofs[i], pubs[i], vk) if i in bad else VALID for i in range(count)]
    assert all(expect[i] == INVALID for i in bad)
    rc, msg, verdicts, stats = VB.batch(True, proofs, pubs, vk, device=0)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(count, len(bad), stats)
    if count > 1:
        i = 7                                                                     # the device's f of an UltraGroth proof as well
        r, f = VB.trace(i)
        p = json.loads(proofs[i])
        assert f == VB.product_miller(VB.g1_rec(PR.g1_mul((int(p["pi_a"][0]), int(p["pi_a"][1])), r)), VB.g2_rec(p["pi_b"]))


def test_device_and_host_agree(g16):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    for at, kind in ((0, "A.y negated"), (63, "json syntax"), (64, "C = generator"), (100, "B off subgroup"), (129, "A = infinity")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    dev = VB.batch(False, proofs, pubs, vk, device=0)
    host = VB.batch(False, proofs, pubs, vk, device=-1)
    assert dev[:3] == host[:3] and dev[0] == INVALID
    assert [i for i, v in enumerate(dev[2]) if v != VALID] == [0, 63, 64, 100, 129] and dev[2][63] == ERROR
    assert dev[3]["off_subgroup"] == host[3]["off_subgroup"] == 1
    for s in (dev[3], host[3]):
        s = dict(s)
        s["single_checks"] -= 1                                                   # the off-subgroup proof never met the batch
        VB.check_bound(128, 3, s)


def test_python_entry_point(g16):
    import ultragroth_amd as ug
    proofs, pubs, vk = g16
    verdicts, stats = ug.groth16_verify_batch(proofs[:5], pubs[:5], vk)
    assert verdicts == [VALID] * 5 and stats["device_ms"] > 0
