"""Batch verification under several keys on the device: the forest kernels (f12_forest_kernel, g1_forest_kernel), the keyed judge and
the resident path with records regrouped by key (pairing.hip). The forests are compared byte for byte with the host's; every
expected verdict is the single verifier's on the same strings under the proof's own key."""
import math
import random
import time

import pytest

import verify_batch_cases as VB
import verify_formats_cases as VF
import verify_keys_cases as VK
import verify_records_cases as VR
from verify_batch_cases import VALID, INVALID

pytestmark = pytest.mark.gpu
COUNTS = [20, 17, 20]
# an odd node at several levels, a segment that ends while its neighbours go on, the 64-lane block edge; many segments, so that the
# table lookup crosses several blocks (segments of one leaf alone launch nothing: the mixed lists do)
SEGMENT_LISTS = [[1], [2], [3], [1, 1, 1], [64, 65, 1, 3], [5, 127, 128, 129], [1] * 300, [2, 3, 1] * 100]


@pytest.fixture(scope="module")
def sets(device):
    return VK.g16_keys()


@pytest.fixture(scope="module")
def mixed(sets):
    proofs, pubs, key_of = VK.interleave(sets, COUNTS)
    return proofs, pubs, key_of, [s[0] for s in sets]


def positions(key_of, q):
    return [i for i, k in enumerate(key_of) if k == q]


def launches_bound(largest, passes=1):
    return 2 * passes * math.ceil(math.log2(largest)) if largest > 1 else 0


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sizes", SEGMENT_LISTS, ids=lambda s: "%dx%d" % (len(s), max(s)) if len(s) > 4 else str(s))
def test_device_forest_equals_the_host_forest(device, k, sizes):
    leaves_f, leaves_g = VK.forest_leaves(sum(sizes), k, 7)
    assert VK.forest(0, k, sizes, leaves_f, leaves_g) == VK.forest(-1, k, sizes, leaves_f, leaves_g)


def test_valid_and_bad_proofs(mixed):
    proofs, pubs, key_of, vks = mixed
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of, device=0)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * len(proofs))
    assert stats["batch_checks"] == 1 and stats["key_checks"] == 1 and stats["single_checks"] == 0 and stats["segments"] == 3
    assert 0 < stats["tree_launches"] <= launches_bound(20) and stats["device_ms"] > 0
    proofs, pubs = list(proofs), list(pubs)
    spots = [positions(key_of, 0)[0], positions(key_of, 2)[-1]]
    for at, kind in zip(spots, ("signal+1", "C = generator")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert sorted(i for i, v in enumerate(expect) if v == INVALID) == sorted(spots)
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of, device=0)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % min(spots)
    VK.check_bound(COUNTS, [1, 0, 1], stats)


def test_refused_key(mixed):
    proofs, pubs, key_of, vks = mixed
    vks = [dict(v) for v in vks]
    vks[1]["vk_gamma_2"] = VB.off_subgroup_b()
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of, device=0)
    assert verdicts == expect and stats["single_checks"] == COUNTS[1] and stats["segments"] == 2 and stats["batch_checks"] == 1
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    rc, msg, verdicts, stats = VK.keys_records(False, recs, blocks, vks, key_of, device=0)
    assert verdicts == expect and stats["single_checks"] == COUNTS[1] and stats["segments"] == 2


@pytest.mark.parametrize("fmt", [VF.PLAIN, VF.EVM, VF.COMPRESSED])
def test_records_with_a_compaction_pass(mixed, fmt):
    """one record off its curve and one pi_b off the subgroup in different segments: the arrays are compacted by the gather
    kernel, and what is kept is still in key order"""
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    spots = [positions(key_of, 0)[4], positions(key_of, 1)[9], positions(key_of, 2)[2]]
    for at, kind in zip(spots, ("C off curve", "B off subgroup", "signal+1")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert sorted(i for i, v in enumerate(expect) if v == INVALID) == sorted(spots)
    ug = VK._ug()
    if fmt == VF.COMPRESSED:
        # a point off its curve has no compressed form; its kin there is an x without a y, INVALID by the layout's contract
        valid = ug.proof_record_convert(VR.pack(mixed[0][spots[0]]), VF.PLAIN, fmt)
        recs = [VF.without_root(valid, 2) if i == spots[0] else ug.proof_record_convert(VR.pack(p), VF.PLAIN, fmt) for i, p in enumerate(proofs)]
    else:
        recs = [ug.proof_record_convert(VR.pack(p), VF.PLAIN, fmt) for p in proofs]
    blocks = [ug.inputs_convert(VR.pack_inputs(s), VF.PLAIN, fmt) for s in pubs]
    rc, msg, verdicts, stats = VK.keys_records(False, recs, blocks, vks, key_of, device=0, fmt=fmt)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % min(spots)
    assert stats["off_subgroup"] == 1 and stats["segments"] == 3 and VR.passes() == (0, 1)
    assert stats["tree_launches"] <= launches_bound(20)
    got, st = ug.groth16_verify_batch_records_keys(b"".join(recs), b"".join(blocks), vks, key_of, device=0, format=fmt)
    assert got == expect


def test_ultragroth_two_keys(device):
    u = VK.ultra_keys()
    vks = [s[0] for s in u]
    proofs, pubs, key_of = VK.interleave(u, [12, 11])
    at = positions(key_of, 1)[4]
    proofs[at], pubs[at] = VB.bad_proof("C = generator", proofs[at], pubs[at], ultra=True)
    expect = VK.expected(True, proofs, pubs, vks, key_of)
    assert expect[at] == INVALID and expect.count(VALID) == 22
    rc, msg, verdicts, stats = VK.keys_batch(True, proofs, pubs, vks, key_of, device=0)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at and stats["segments"] == 2
    VK.check_bound([12, 11], [0, 1], stats)
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    for fmt in (VF.PLAIN, VF.COMPRESSED):                                       # compressed: the challenge from the device's pi_r
        ug = VK._ug()
        conv = [ug.proof_record_convert(r, VF.PLAIN, fmt, ultra=True) for r in recs]
        assert VK.keys_records(True, conv, blocks, vks, key_of, device=0, fmt=fmt)[:3] == (rc, msg, verdicts)


def test_keyed_judge_one_launch(mixed):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    spots = [positions(key_of, 0)[1], positions(key_of, 1)[16], positions(key_of, 2)[0]]
    for at, kind in zip(spots, ("signal+1", "B off subgroup", "A.y negated")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert sorted(i for i, v in enumerate(expect) if v == INVALID) == sorted(spots)
    off = VK.keys_batch(False, proofs, pubs, vks, key_of, device=0, opt=VR.options(0))
    on = VK.keys_batch(False, proofs, pubs, vks, key_of, device=0, opt=VR.options(1, -1, 1))
    assert off[:3] == on[:3] and on[2] == expect
    assert on[3]["judge_launches"] == 1 and on[3]["judged"] >= 3 and on[3]["single_checks"] == 0
    suspects_of = set()                                                         # the launch did hold suspects of three keys
    for at in spots:
        suspects_of.add(key_of[at])
    assert len(suspects_of) == 3
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    rec_on = VK.keys_records(False, recs, blocks, vks, key_of, device=0, opt=VR.options(1, 0, 1))      # width 0: the whole pass is judged
    assert rec_on[2] == expect and rec_on[3]["judge_launches"] == 1 and rec_on[3]["judged"] == len(proofs)


def test_pass_boundary(sets):
    """65 536 + 40 records, repeats of valid records of three keys, interleaved by the caller; the middle key's group crosses the
    pass boundary, with one bad record on each side of it"""
    vks = [s[0] for s in sets]
    packed = [([VR.pack(p) for p in s[1]], [VR.pack_inputs(x) for x in s[2]]) for s in sets]
    counts = [10000, 55556, 20]
    key_of = [q for q, c in enumerate(counts) for _ in range(c)]
    random.Random(3).shuffle(key_of)
    seen, recs, blocks = [0, 0, 0], [], []
    for q in key_of:
        recs.append(packed[q][0][seen[q] % VK.PER_KEY])
        blocks.append(packed[q][1][seen[q] % VK.PER_KEY])
        seen[q] += 1
    middle = positions(key_of, 1)
    spots = [middle[100], middle[-1]]                                           # in key order: position 10 100 and 65 555
    for at in spots:
        proof, pub = VB.bad_proof("signal+1", sets[1][1][0], sets[1][2][0])
        recs[at], blocks[at] = VR.pack(proof), VR.pack_inputs(pub)
        assert VR.single(False, recs[at], blocks[at], vks[1]) == INVALID
    t0 = time.time()
    rc, msg, verdicts, stats = VK.keys_records(False, recs, blocks, vks, key_of, device=0)
    print("pass boundary: %.2f s, stats %s" % (time.time() - t0, stats))
    assert rc == INVALID and msg == "proof %d: invalid proof" % min(spots)
    assert [i for i, v in enumerate(verdicts) if v != VALID] == sorted(spots) and all(verdicts[i] == INVALID for i in spots)
    assert stats["batch_checks"] >= 2 and stats["segments"] == 4                # keys 0 and 1 in the first pass, 1 and 2 in the second
    assert stats["tree_launches"] <= launches_bound(55536) + launches_bound(20)
