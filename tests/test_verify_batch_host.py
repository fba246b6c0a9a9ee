"""ug_groth16_verify_batch / ug_ultra_groth_verify_batch with device = -1: the whole protocol (random scalars, trees of partial
products, prefix sums, the search of a rejected batch) on host threads, no GPU. Proofs are the oracle's, of the trapdoor fixtures;
every expected verdict is the single-proof verifier's on the same strings."""
import ctypes as C
import json
import os
import subprocess

import pytest

import oracle as O
from oracle import pairing as PR
import verify_batch_cases as VB
from verify_batch_cases import VALID, INVALID, ERROR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultragroth_amd", "csrc")


@pytest.fixture(scope="module")
def g16():
    zkey, wtns, vk = VB.load("groth16.zkey"), VB.load("groth16.wtns"), json.loads(VB.load("groth16_vkey.json", "r"))
    pairs = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(33)]
    assert len({p for p, _ in pairs}) == 33
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    assert all(VB.single(False, p, s, vk) == VALID for p, s in pairs)
    return proofs, pubs, vk


@pytest.fixture(scope="module")
def ultra():
    zkey, uwtns, vk = VB.load("ultra.zkey"), VB.load("ultra.uwtns"), json.loads(VB.load("ultra_vkey.json", "r"))
    pairs = [O.ultra_groth_prove(zkey, uwtns, 10 + i, 200 + i, 3000 + i)[:2] for i in range(17)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    assert all(VB.single(True, p, s, vk) == VALID for p, s in pairs)
    return proofs, pubs, vk


@pytest.mark.parametrize("count", [0, 1, 2, 3, 17, 33])
def test_valid_batches(g16, count):
    proofs, pubs, vk = g16
    rc, msg, verdicts, stats = VB.batch(False, proofs[:count], pubs[:count], vk)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * count)
    assert stats["batch_checks"] == (1 if count else 0) and stats["single_checks"] == 0 and stats["off_subgroup"] == 0


@pytest.mark.parametrize("at", [0, 16, 32])
def test_one_bad_proof_is_found(g16, at):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    proofs[at], pubs[at] = VB.bad_proof("signal+1", proofs[at], pubs[at])
    expect = [VALID] * 33
    expect[at] = VB.single(False, proofs[at], pubs[at], vk)
    assert expect[at] == INVALID
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at
    VB.check_bound(33, 1, stats)
    assert stats["single_checks"] >= 1 and stats["batch_checks"] >= 2


@pytest.mark.parametrize("kind", VB.KINDS)
def test_kinds_of_bad_proof(g16, kind):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs[:19]), list(pubs[:19])
    proofs[17], pubs[17] = VB.bad_proof(kind, proofs[17], pubs[17])
    expect = [VB.single(False, p, s, vk) if i == 17 else VALID for i, (p, s) in enumerate(zip(proofs, pubs))]
    assert expect[17] == (ERROR if kind in ("json syntax", "signal count") else INVALID)
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk)
    assert rc == INVALID and verdicts == expect and msg.startswith("proof 17: ")
    if kind == "json syntax":
        assert msg == "proof 17: invalid proof data"
    if kind == "B off subgroup":
        assert stats["off_subgroup"] == 1 and stats["single_checks"] == 1 and stats["batch_checks"] == 1
    if kind in ("json syntax", "signal count", "C off curve"):              # answered without a pairing: the other 18 hold
        assert stats["single_checks"] == 0 and stats["batch_checks"] == 1


def test_cancelling_pair(g16):
    """equal scalars would accept C_1 + D, C_2 - D: the product of the two equations holds"""
    proofs, pubs, vk = g16
    proofs = list(proofs[:20])
    proofs[3], proofs[18] = VB.cancelling_pair(proofs[3], proofs[18])
    expect = [VB.single(False, p, s, vk) for p, s in zip(proofs, pubs[:20])]
    assert [i for i, v in enumerate(expect) if v == INVALID] == [3, 18]
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs[:20], vk)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(20, 2, stats)


def test_several_bad_proofs(g16):
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    for at, kind in ((0, "A.y negated"), (15, "json syntax"), (16, "C = generator"), (31, "B off subgroup"), (32, "A = infinity")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = [VB.single(False, p, s, vk) for p, s in zip(proofs, pubs)]
    rc, msg, verdicts, stats = VB.batch(False, proofs, pubs, vk)
    assert rc == INVALID and verdicts == expect and expect.count(VALID) == 28
    assert msg == "proof 0: invalid proof"
    assert stats["off_subgroup"] == 1
    stats["single_checks"] -= 1                                                   # the off-subgroup proof never met the batch
    VB.check_bound(31, 3, stats)


def test_argument_errors(g16):
    proofs, pubs, vk = g16
    L = VB.lib()
    key = json.dumps(vk).encode()
    pa = (C.c_char_p * 2)(proofs[0].encode(), proofs[1].encode())
    ia = (C.c_char_p * 2)(pubs[0].encode(), pubs[1].encode())
    for args, text in (((2, None, ia, key), "null argument"), ((2, pa, None, key), "null argument"), ((2, pa, ia, None), "null argument"),
                       ((-1, pa, ia, key), "null argument"), ((2, pa, ia, key[:len(key) // 2]), "invalid verification key data")):
        verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
        err = C.create_string_buffer(256)
        count, p, i, k = args
        assert L.ug_groth16_verify_batch(-1, count, p, i, k, verdicts, None, err, 255) == ERROR
        assert err.value.decode() == text and list(verdicts) == [VB.SENTINEL] * 2
    assert L.ug_groth16_verify_batch(-1, 2, pa, ia, key, None, None, None, 0) == ERROR
    assert L.ug_groth16_verify_batch(-1, 0, None, None, key, None, None, None, 0) == VALID
    verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
    assert L.ug_groth16_verify_batch(-1, 2, pa, ia, key, verdicts, None, None, 0) == VALID and list(verdicts) == [VALID] * 2
    assert L.ug_ultra_groth_verify_batch(-1, 2, pa, ia, key, verdicts, None, None, 0) == ERROR          # a Groth16 key


def test_python_entry_points(g16):
    import ultragroth_amd as ug
    proofs, pubs, vk = g16
    verdicts, stats = ug.groth16_verify_batch(proofs[:3], pubs[:3], vk, device=-1)
    assert verdicts == [VALID] * 3 and stats["batch_checks"] == 1 and stats["host_ms"] > 0 and stats["device_ms"] == 0
    with pytest.raises(ug.VerifierError, match="invalid verification key data"):
        ug.groth16_verify_batch(proofs[:3], pubs[:3], "{", device=-1)
    assert ug.groth16_verify_batch([], [], vk, device=-1)[0] == []


@pytest.mark.parametrize("count", [3, 17])
def test_ultragroth(ultra, count):
    proofs, pubs, vk = ultra
    rc, msg, verdicts, stats = VB.batch(True, proofs[:count], pubs[:count], vk)
    assert (rc, verdicts, stats["batch_checks"], stats["single_checks"]) == (VALID, [VALID] * count, 1, 0)
    proofs, pubs = list(proofs[:count]), list(pubs[:count])
    last = count - 1
    mixed = json.loads(proofs[last])
    mixed["pi_r"] = json.loads(proofs[0])["pi_r"]                                 # another proof's round commitment: the challenge moves
    proofs[last] = json.dumps(mixed)
    proofs[1], pubs[1] = VB.bad_proof("C = generator", proofs[1], pubs[1], ultra=True)
    expect = [VB.single(True, p, s, vk) for p, s in zip(proofs, pubs)]
    assert expect[1] == INVALID and expect[last] == INVALID and expect.count(VALID) == count - 2
    rc, msg, verdicts, stats = VB.batch(True, proofs, pubs, vk)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(count, 2, stats)


def test_ultragroth_cancelling_round_commitments_and_key_off_subgroup(ultra):
    proofs, pubs, vk = ultra
    proofs = list(proofs[:4])
    proofs[0], proofs[2] = VB.cancelling_pair(proofs[0], proofs[2], ultra=True)
    expect = [VB.single(True, p, s, vk) for p, s in zip(proofs, pubs[:4])]
    assert expect == [INVALID, VALID, INVALID, VALID]
    assert VB.batch(True, proofs, pubs[:4], vk)[2] == expect
    key = dict(vk)
    key["vk_gamma_2"] = VB.off_subgroup_b()                                       # no batching under such a key: the single verdicts
    expect = [VB.single(True, p, s, key) for p, s in zip(proofs, pubs[:4])]
    rc, msg, verdicts, stats = VB.batch(True, proofs, pubs[:4], key)
    assert verdicts == expect and stats["single_checks"] == 4 and stats["batch_checks"] == 0


def test_miller_with_range_assertions_equals_the_product_build(g16):
    """libug_hostmath_test.so is pairing.hpp under -DUG_CHECK_BOUNDS: every lazy column sum of the Fq12 products checks its headroom
    and every subtraction its multiple of q, and the value is the product build's limb for limb"""
    proofs, pubs, vk = g16
    subprocess.check_call(["make", "-s", "-C", CSRC, os.path.join(CSRC, "libug_hostmath_test.so")])
    T = C.CDLL(os.path.join(CSRC, "libug_hostmath_test.so"))
    p = json.loads(proofs[0])
    a, b = VB.g1_rec(p["pi_a"]), VB.g2_rec(p["pi_b"])
    out = (C.c_uint32 * 108)()
    assert T.ugt_miller(out, a, b) == 0
    assert list(out) == VB.product_miller(a, b)
    assert any(out) and all(w < (1 << 29) for w in out)
    assert T.ugt_miller(out, bytes(64), b) == 1


def test_trace_is_the_miller_loop_of_the_scaled_point(g16):
    """the f_i of a host batch: miller(B_i, r_i A_i) with the call's own scalars, which differ from call to call"""
    proofs, pubs, vk = g16
    seen = set()
    for _ in range(2):
        assert VB.batch(False, proofs[:3], pubs[:3], vk)[0] == VALID
        for i in range(3):
            r, f = VB.trace(i)
            assert 0 < r < 1 << 128
            seen.add(r)
            p = json.loads(proofs[i])
            ra = PR.g1_mul((int(p["pi_a"][0]), int(p["pi_a"][1])), r)
            assert f == VB.product_miller(VB.g1_rec(ra), VB.g2_rec(p["pi_b"]))
    assert len(seen) == 6
