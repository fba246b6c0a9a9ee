"""The judge of batch verification on the device (pairing.hip: vkx_mul_kernel, vkx_sum_kernel, judge_kernel): suspects decided by
their own equations, one lane each. Every expected verdict is the single-proof verifier's on the same strings; the device's final
exponentiation is compared with the host's limb for limb. Proofs are prove_batch's, as in test_gpu_verify_batch.py."""
import ctypes as C
import json

import pytest

from oracle import pairing as PR
import verify_batch_cases as VB
import verify_judge_cases as VJ
from verify_batch_cases import VALID, INVALID, ERROR

pytestmark = pytest.mark.gpu

WHOLE = dict(judge=1, search_width=0, judge_min=1)                  # no host search: a rejected pass is judged as a whole


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
    return proofs, pubs, vk


@pytest.fixture(scope="module")
def g16_bad(g16):
    """every proof with signal+1 and the single verifier's verdict on it, computed once"""
    proofs, pubs, vk = g16
    bad = [VB.bad_proof("signal+1", p, s) for p, s in zip(proofs, pubs)]
    verdicts = VJ.singles(False, [p for p, _ in bad], [s for _, s in bad], vk)
    assert verdicts == [INVALID] * 130
    return bad


@pytest.fixture(scope="module")
def ultra(device):
    import ultragroth_amd as ug
    vk = json.loads(VB.load("ultra_vkey.json", "r"))
    proofs, pubs = _prove(ug.UltraGrothProver, VB.load("ultra.zkey"), VB.load("ultra.uwtns"), 65)
    return proofs, pubs, vk


@pytest.mark.parametrize("count", [1, 17, 64, 65, 130])
def test_whole_pass_judged(g16, g16_bad, count):
    """one bad proof at the end, no host search: every proof of the pass is judged, the valid ones valid, on the device"""
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:count]), list(pubs[:count])
    at = count - 1
    proofs[at], pubs[at] = g16_bad[at]
    expect = [VALID] * at + [INVALID]
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=0, **WHOLE)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at
    assert stats["batch_checks"] == 1 and stats["single_checks"] == 0
    assert stats["judged"] == count and stats["judge_launches"] == 1 and 0 < stats["judge_ms"] <= stats["device_ms"]


@pytest.mark.parametrize("kind", VB.KINDS)
def test_kinds_of_bad_proof(g16, kind):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:65]), list(pubs[:65])
    proofs[64], pubs[64] = VB.bad_proof(kind, proofs[64], pubs[64])
    expect = [VALID] * 64 + [VB.single(False, proofs[64], pubs[64], vk)]
    assert expect[64] == (ERROR if kind in ("json syntax", "signal count") else INVALID)
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=0, **WHOLE)
    assert rc == INVALID and verdicts == expect and msg.startswith("proof 64: ") and stats["single_checks"] == 0
    if kind == "B off subgroup":                                                  # set aside by the subgroup ladder, judged alone
        assert stats["off_subgroup"] == 1 and stats["judged"] == 1 and stats["batch_checks"] == 1
    elif kind in ("json syntax", "signal count", "C off curve"):                  # answered without a pairing: the other 64 hold
        assert stats["judged"] == 0 and stats["judge_launches"] == 0
    else:                                                                         # "A = infinity": the skipped-pair rule in a lane
        assert stats["judged"] == 65


def test_unreduced_public_signal(g16, g16_bad):
    """a signal written as value + r: the same residue; the verdict is the single verifier's, whatever it is"""
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:65]), list(pubs[:65])
    s = json.loads(pubs[3])
    s[0] = str(int(s[0]) + PR.R)
    pubs[3] = json.dumps(s)
    proofs[40], pubs[40] = g16_bad[40]                                            # so that the pass is rejected and proof 3 judged
    expect = [VALID] * 65
    expect[3], expect[40] = VB.single(False, proofs[3], pubs[3], vk), INVALID
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=0, **WHOLE)
    assert verdicts == expect and stats["judged"] == 65 and stats["single_checks"] == 0


@pytest.mark.parametrize("every", [1, 2])
def test_many_bad_proofs(g16, g16_bad, every):
    """all 130 bad, and every second one; the search gives up at more than 4 failing nodes, 130 suspects >= 64"""
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    for i in range(0, 130, every):
        proofs[i], pubs[i] = g16_bad[i]
    expect = [INVALID if i % every == 0 else VALID for i in range(130)]
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=0, judge=1, search_width=4, judge_min=64)
    assert rc == INVALID and verdicts == expect and msg == "proof 0: invalid proof"
    assert stats["judged"] == 130 and stats["single_checks"] == 0 and stats["judge_launches"] == 1
    assert stats["batch_checks"] <= 1 + 2 * 4 * 4                                # ceil(log2(130 / 16)) = 4 levels, at most 4 open nodes each


def test_cancelling_pair(g16):
    proofs, pubs, vk = g16
    proofs = list(proofs[:65])
    proofs[0], proofs[64] = VB.cancelling_pair(proofs[0], proofs[64])
    expect = [VB.single(False, proofs[i], pubs[i], vk) if i in (0, 64) else VALID for i in range(65)]
    assert expect[0] == INVALID and expect[64] == INVALID
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs[:65], vk, device=0, **WHOLE)
    assert rc == INVALID and verdicts == expect and stats["judged"] == 65


def test_ultragroth(ultra):
    """t_rand, the IC_rand column and the two delta pairs: another proof's pi_r at the end, a cancelling pair at 0 and 33"""
    proofs, pubs, vk = ultra
    proofs, pubs = list(proofs), list(pubs)
    mixed = json.loads(proofs[64])
    mixed["pi_r"] = json.loads(proofs[0])["pi_r"]
    proofs[64] = json.dumps(mixed)
    proofs[0], proofs[33] = VB.cancelling_pair(proofs[0], proofs[33], ultra=True)
    bad = (0, 33, 64)
    expect = [VB.single(True, proofs[i], pubs[i], vk) if i in bad else VALID for i in range(65)]
    assert all(expect[i] == INVALID for i in bad)
    rc, msg, verdicts, stats = VJ.batch_opt(True, proofs, pubs, vk, device=0, **WHOLE)
    assert rc == INVALID and verdicts == expect and msg == "proof 0: invalid proof"
    assert stats["judged"] == 65 and stats["single_checks"] == 0 and stats["batch_checks"] == 1


def test_device_and_host_agree(g16):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    for at, kind in ((0, "A.y negated"), (63, "json syntax"), (64, "C = generator"), (100, "B off subgroup"), (129, "A = infinity")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    dev = VJ.batch_opt(False, proofs, pubs, vk, device=0, **WHOLE)
    host = VJ.batch_opt(False, proofs, pubs, vk, device=-1, **WHOLE)
    assert dev[:3] == host[:3] and dev[0] == INVALID
    assert [i for i, v in enumerate(dev[2]) if v != VALID] == [0, 63, 64, 100, 129] and dev[2][63] == ERROR
    for f in ("batch_checks", "single_checks", "off_subgroup", "judged"):
        assert dev[3][f] == host[3][f], f
    assert dev[3]["judged"] == 129 and dev[3]["judge_launches"] == 1 and host[3]["judge_launches"] == 0
    assert dev[2] == VB.batch(False, proofs, pubs, vk, device=0)[2]              # and the judge-off path says the same


def test_final_exp_device_equals_host(g16):
    proofs, pubs, vk = g16
    L = VB.lib()
    for name, f, one in VJ.final_exp_values(proofs[0], pubs[0], vk):
        fin = (C.c_uint32 * 108)(*VJ.f12_limbs(f))
        out = []
        for dev in (-1, 0):
            g, flag = (C.c_uint32 * 108)(), C.c_int(-1)
            assert L.ug_test_final_exp(dev, fin, g, C.byref(flag)) == 0, name
            out.append((list(g), flag.value))
        assert out[0] == out[1] and out[0][1] == int(one), name


def test_two_passes(g16, g16_bad):
    """2^16 + 3 proofs, the 130 distinct ones repeated: the first pass is accepted by one root check, the two bad proofs of the short
    second pass are the only rejected one's, and the judge sees that pass alone"""
    proofs, pubs, vk = g16
    n = (1 << 16) + 3
    ps, ss = [proofs[i % 130] for i in range(n)], [pubs[i % 130] for i in range(n)]
    for i in (n - 3, n - 1):
        ps[i], ss[i] = g16_bad[i % 130]
    rc, msg, verdicts, stats = VJ.batch_opt(False, ps, ss, vk, device=0, **WHOLE)
    assert rc == INVALID and msg == "proof %d: invalid proof" % (n - 3)
    assert [i for i, v in enumerate(verdicts) if v != VALID] == [n - 3, n - 1] and verdicts[n - 1] == INVALID
    assert stats["batch_checks"] == 2 and stats["judged"] == 3 and stats["judge_launches"] == 1 and stats["single_checks"] == 0
