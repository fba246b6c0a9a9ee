"""Batch verification under several keys (include/verifier.h: ug_*_verify_batch_keys, ug_*_verify_batch_records_keys) with
device = -1: no GPU. Keys with 1, 2 and 3 public inputs (verify_keys_cases); every expected verdict is the single-proof verifier's on
the same strings under the proof's own key, and every intended-bad proof is first shown to be INVALID there."""
import ctypes as C
import json
import os
import re

import pytest

import verify_batch_cases as VB
import verify_formats_cases as VF
import verify_keys_cases as VK
import verify_records_cases as VR
from oracle import pairing as PR
from verify_batch_cases import VALID, INVALID, ERROR, SENTINEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [20, 17, 20]


@pytest.fixture(scope="module")
def sets():
    return VK.g16_keys()


@pytest.fixture(scope="module")
def mixed(sets):
    """57 valid proofs under three keys, interleaved: (proofs, pubs, key_of, vks)"""
    proofs, pubs, key_of = VK.interleave(sets, COUNTS)
    return proofs, pubs, key_of, [s[0] for s in sets]


def positions(key_of, q):
    """the caller's indices of the proofs of key q, in the order of their segment"""
    return [i for i, k in enumerate(key_of) if k == q]


@pytest.mark.parametrize("n_keys", [1, 2, 3])
def test_valid_interleaved_batches(sets, n_keys):
    proofs, pubs, key_of = VK.interleave(sets[:n_keys], COUNTS[:n_keys])
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, [s[0] for s in sets[:n_keys]], key_of)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * len(proofs))
    assert stats["batch_checks"] == 1 and stats["key_checks"] == 1 and stats["single_checks"] == 0 and stats["segments"] == n_keys
    assert stats["tree_launches"] == 0                                          # host threads launch nothing


@pytest.mark.parametrize("bad", [None, 13])
@pytest.mark.parametrize("judge", [False, True])
def test_one_key_equals_the_one_key_call(sets, bad, judge):
    vk, proofs, pubs = sets[1][0], list(sets[1][1]), list(sets[1][2])
    if bad is not None:
        proofs[bad], pubs[bad] = VB.bad_proof("A.y negated", proofs[bad], pubs[bad])
    from ultragroth_amd._lib import VerifyBatchStatsEx
    opt = VR.options(1 if judge else 0, -1, 1)
    n = len(proofs)
    pa = (C.c_char_p * n)(*[p.encode() for p in proofs])
    ia = (C.c_char_p * n)(*[p.encode() for p in pubs])
    verdicts, st, err = (C.c_int * n)(*([SENTINEL] * n)), VerifyBatchStatsEx(), C.create_string_buffer(512)
    rc1 = VB.lib().ug_groth16_verify_batch_opt(-1, n, pa, ia, json.dumps(vk).encode(), verdicts, C.byref(opt), C.byref(st), err, 511)
    one = VR._stats(st)
    rc, msg, got, stats = VK.keys_batch(False, proofs, pubs, [vk], [0] * n, opt=opt)
    assert (rc, msg, got) == (rc1, err.value.decode(), list(verdicts))
    assert rc == (INVALID if bad is not None else VALID)
    for f in ("batch_checks", "single_checks", "off_subgroup", "judged", "judge_launches"):
        assert stats[f] == one[f], f
    assert stats["segments"] == 1 and stats["key_checks"] == 1


@pytest.mark.parametrize("kind", VB.KINDS)
def test_kinds_of_bad_proof_in_one_key(mixed, kind):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    at = positions(key_of, 1)[5]
    proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert expect[at] != VALID and [v for i, v in enumerate(expect) if i != at] == [VALID] * 56
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert rc == INVALID and verdicts == expect and msg.startswith("proof %d: " % at)
    if kind not in ("json syntax", "signal count", "C off curve", "B off subgroup"):
        VK.check_bound(COUNTS, [0, 1, 0], stats)


@pytest.mark.parametrize("q,where", [(0, 0), (0, -1), (2, 0), (2, -1)])
def test_bad_proof_at_the_ends_of_the_first_and_last_segment(mixed, q, where):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    at = positions(key_of, q)[where]
    proofs[at], pubs[at] = VB.bad_proof("signal+1", proofs[at], pubs[at])
    assert VB.single(False, proofs[at], pubs[at], vks[q]) == INVALID
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert rc == INVALID and msg == "proof %d: invalid proof" % at                # the caller's index
    assert verdicts == [INVALID if i == at else VALID for i in range(len(proofs))]
    VK.check_bound(COUNTS, [1 if s == q else 0 for s in range(3)], stats)


def test_two_bad_proofs_under_two_keys(mixed):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    spots = [positions(key_of, 0)[3], positions(key_of, 2)[11]]
    for at, kind in zip(spots, ("C = generator", "A.y negated")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert sorted(i for i, v in enumerate(expect) if v == INVALID) == sorted(spots)
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % min(spots)
    VK.check_bound(COUNTS, [1, 0, 1], stats)


def test_cancelling_pair_across_two_segments(sets):
    """C_1 + D under key 1 and C_2 - D under a copy of key 1 given as another key: two segments with the same delta, whose errors
    cancel in any combination with equal weights"""
    vk, proofs, pubs = sets[1]
    a, b = VB.cancelling_pair(proofs[2], proofs[9])
    ps, ss, key_of = list(proofs[:12]), list(pubs[:12]), [0] * 6 + [1] * 6
    ps[2], ps[9] = a, b
    expect = VK.expected(False, ps, ss, [vk, vk], key_of)
    assert [i for i, v in enumerate(expect) if v == INVALID] == [2, 9]
    rc, msg, verdicts, stats = VK.keys_batch(False, ps, ss, [vk, vk], key_of)
    assert rc == INVALID and verdicts == expect and stats["segments"] == 2


def test_proof_labelled_with_another_key(sets):
    """valid under key 1, labelled key 2 (another input count: ERROR, as the single call says) and under a same-shape other key"""
    vks = [s[0] for s in sets]
    proofs, pubs, key_of = VK.interleave(sets, [6, 6, 6])
    at = positions(key_of, 1)[2]
    key_of[at] = 2
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert expect[at] == ERROR
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: len(inputs)+1 != len(vk.IC)" % at
    u = VK.ultra_keys()                                                        # same circuit, another trapdoor: INVALID
    proofs, pubs, key_of = VK.interleave(u, [5, 5])
    at = positions(key_of, 0)[1]
    key_of[at] = 1
    expect = VK.expected(True, proofs, pubs, [s[0] for s in u], key_of)
    assert expect[at] == INVALID and expect.count(VALID) == 9
    rc, msg, verdicts, stats = VK.keys_batch(True, proofs, pubs, [s[0] for s in u], key_of)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at


def test_refused_key_sends_only_its_own_proofs_to_the_single_verifier(mixed):
    proofs, pubs, key_of, vks = mixed
    vks = [dict(v) for v in vks]
    vks[1]["vk_gamma_2"] = VB.off_subgroup_b()                                  # on the twist, outside the subgroup
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert all(v == VALID for v, q in zip(expect, key_of) if q != 1)
    rc, msg, verdicts, stats = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert verdicts == expect and stats["single_checks"] == COUNTS[1] and stats["segments"] == 2 and stats["batch_checks"] == 1
    only = [i for i, q in enumerate(key_of) if q != 1]                          # without that key's proofs: no single check at all
    rc, msg, verdicts, stats = VK.keys_batch(False, [proofs[i] for i in only], [pubs[i] for i in only], vks, [key_of[i] for i in only])
    assert (rc, verdicts) == (VALID, [VALID] * len(only)) and stats["single_checks"] == 0


def test_argument_errors(mixed):
    proofs, pubs, key_of, vks = mixed
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    untouched = [SENTINEL] * len(proofs)
    for wrong in (3, -1):
        ko = list(key_of)
        ko[4] = wrong
        rc, msg, verdicts, _ = VK.keys_batch(False, proofs, pubs, vks, ko)
        assert (rc, msg, verdicts) == (ERROR, "proof 4: key index %d out of range" % wrong, untouched)
        rc, msg, verdicts, _ = VK.keys_records(False, recs, blocks, vks, ko)
        assert (rc, msg, verdicts) == (ERROR, "proof 4: key index %d out of range" % wrong, untouched)
    rc, msg, verdicts, _ = VK.keys_batch(False, proofs, pubs, [vks[0], "{", vks[2]], key_of)
    assert (rc, msg, verdicts) == (ERROR, "key 1: invalid verification key data", untouched)
    rc, msg, verdicts, _ = VK.keys_records(False, recs, blocks, vks, key_of, n_pub=[1, 2, 4])
    assert (rc, msg, verdicts) == (ERROR, "key 2: len(inputs)+1 != len(vk.IC)", untouched)
    rc, msg, verdicts, _ = VK.keys_records(False, recs, blocks, vks, key_of, n_pub=[1, 0, 3])
    assert (rc, msg, verdicts) == (ERROR, "key 1: invalid inputs data", untouched)
    rc, msg, verdicts, _ = VK.keys_records(False, recs, blocks, vks, key_of, fmt=3)
    assert rc == ERROR and msg.startswith("format: not one of UG_RECORDS_PLAIN") and verdicts == untouched
    rc, msg, verdicts, _ = VK.keys_batch(False, proofs, pubs, vks, key_of, n_keys=0)
    assert rc == ERROR and msg.startswith("n_keys") and verdicts == untouched
    rc, msg, verdicts, _ = VK.keys_batch(False, proofs, pubs, vks, None)
    assert (rc, msg, verdicts) == (ERROR, "null argument", untouched)
    # count == 0: valid, with keys or without; a key that no proof names is parsed as well
    rc, msg, verdicts, stats = VK.keys_batch(False, [], [], vks, [])
    assert (rc, msg) == (VALID, "") and stats["batch_checks"] == 0 and stats["segments"] == 0
    assert VK.keys_batch(False, [], [], [], [])[0] == VALID and VK.keys_records(False, [], [], [], [], n_pub=[])[0] == VALID
    two = [i for i, q in enumerate(key_of) if q != 2]
    sub = ([proofs[i] for i in two], [pubs[i] for i in two])
    rc, msg, verdicts, stats = VK.keys_batch(False, sub[0], sub[1], vks, [key_of[i] for i in two])
    assert (rc, verdicts) == (VALID, [VALID] * len(two)) and stats["segments"] == 2
    rc, msg, verdicts, _ = VK.keys_batch(False, sub[0], sub[1], vks[:2] + ["[]"], [key_of[i] for i in two])
    assert (rc, msg) == (ERROR, "key 2: invalid verification key data")


@pytest.mark.parametrize("fmt", [VF.PLAIN, VF.EVM, VF.COMPRESSED])
def test_records_with_ragged_inputs_equal_the_text_call(mixed, fmt):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    at = positions(key_of, 2)[7]
    proofs[at], pubs[at] = VB.bad_proof("signal+1", proofs[at], pubs[at])
    rc0, msg0, verdicts0, stats0 = VK.keys_batch(False, proofs, pubs, vks, key_of)
    assert verdicts0 == VK.expected(False, proofs, pubs, vks, key_of) and rc0 == INVALID
    ug = VK._ug()
    recs = [ug.proof_record_convert(VR.pack(p), VF.PLAIN, fmt) for p in proofs]
    blocks = [ug.inputs_convert(VR.pack_inputs(s), VF.PLAIN, fmt) for s in pubs]
    assert len({len(b) for b in blocks}) == 3                                   # ragged indeed
    rc, msg, verdicts, stats = VK.keys_records(False, recs, blocks, vks, key_of, fmt=fmt)
    assert (rc, msg, verdicts) == (rc0, msg0, verdicts0)
    assert stats["batch_checks"] == stats0["batch_checks"] and stats["segments"] == 3
    got, st = ug.groth16_verify_batch_records_keys(b"".join(recs), ug.inputs_pack_ragged(pubs, fmt), vks, key_of, device=-1, format=fmt)
    assert got == verdicts0 and st["segments"] == 3
    assert ug.groth16_verify_batch_keys(proofs, pubs, vks, key_of, device=-1)[0] == verdicts0


def test_ultragroth_twins_over_two_keys():
    u = VK.ultra_keys()
    vks = [s[0] for s in u]
    proofs, pubs, key_of = VK.interleave(u, [12, 11])
    at = positions(key_of, 1)[4]
    proofs[at], pubs[at] = VB.bad_proof("C = generator", proofs[at], pubs[at], ultra=True)
    expect = VK.expected(True, proofs, pubs, vks, key_of)
    assert expect[at] == INVALID and expect.count(VALID) == 22
    rc, msg, verdicts, stats = VK.keys_batch(True, proofs, pubs, vks, key_of)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at and stats["segments"] == 2
    VK.check_bound([12, 11], [0, 1], stats)
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert VK.keys_records(True, recs, blocks, vks, key_of)[:3] == (rc, msg, verdicts)
    ug = VK._ug()
    assert ug.ultra_groth_verify_batch_keys(proofs, pubs, vks, key_of, device=-1)[0] == expect
    assert ug.ultra_groth_verify_batch_records_keys(b"".join(recs), b"".join(blocks), vks, key_of, device=-1)[0] == expect


@pytest.mark.parametrize("width", [0, 1, 2])
def test_judge_gives_the_same_verdicts(mixed, width):
    proofs, pubs, key_of, vks = mixed
    proofs, pubs = list(proofs), list(pubs)
    spots = [positions(key_of, 0)[1], positions(key_of, 1)[16], positions(key_of, 2)[0]]
    for at, kind in zip(spots, ("signal+1", "B off subgroup", "A.y negated")):
        proofs[at], pubs[at] = VB.bad_proof(kind, proofs[at], pubs[at])
    expect = VK.expected(False, proofs, pubs, vks, key_of)
    assert sorted(i for i, v in enumerate(expect) if v == INVALID) == sorted(spots)
    off = VK.keys_batch(False, proofs, pubs, vks, key_of, opt=VR.options(0))
    on = VK.keys_batch(False, proofs, pubs, vks, key_of, opt=VR.options(1, width, 1))
    assert off[:3] == on[:3] and on[2] == expect
    assert on[3]["judged"] >= 3 and on[3]["single_checks"] == 0 and off[3]["judged"] == 0
    if width == 0:                                                              # the whole pass is suspect after its one equation
        assert on[3]["batch_checks"] == 1 and on[3]["judged"] == len(proofs)


SEGMENT_LISTS = [[1], [2], [3], [1, 1, 1], [5, 1, 2], [17, 4, 33, 16]]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sizes", SEGMENT_LISTS, ids=str)
def test_host_forest_equals_the_segments_own_trees(k, sizes):
    leaves_f, leaves_g = VK.forest_leaves(sum(sizes), k, 40 + k)
    f_tree, g_tree = VK.forest(-1, k, sizes, leaves_f, leaves_g)
    assert len(f_tree) == VK.forest_nodes(sizes) * 432
    assert f_tree[:len(bytes(leaves_f))] == bytes(leaves_f) and g_tree[:len(bytes(leaves_g))] == bytes(leaves_g)
    assert (f_tree, g_tree) == VK.forest_from_single_trees(k, sizes, leaves_f, leaves_g)


def test_one_segment_tree_against_the_oracles_group_law():
    """the G1 root of a one-segment forest is the sum of its leaves, by oracle/pairing.py's own addition"""
    n = 7
    leaves_f, leaves_g = VK.forest_leaves(n, 1, 9)
    _, g_tree = VK.forest(-1, 1, [n], leaves_f, leaves_g)
    words = (C.c_uint32 * (len(g_tree) // 4)).from_buffer_copy(g_tree)
    rinv = pow(1 << 261, -1, VK.Q)
    coord = lambda at: sum(int(words[at + i]) << (29 * i) for i in range(9)) * rinv % VK.Q

    def affine(node):
        x, y, zz, zzz = (coord(node * 36 + 9 * c) for c in range(4))
        return (x * pow(zz, -1, VK.Q) % VK.Q, y * pow(zzz, -1, VK.Q) % VK.Q)
    total = None
    for i in range(n):
        total = PR.g1_add(total, affine(i))
    assert affine(VK.forest_nodes([n]) - 1) == total


def test_exports_and_header():
    from ultragroth_amd import _lib
    lib = VB.lib()
    header = open(os.path.join(ROOT, "include", "verifier.h")).read()
    for name in ("ug_groth16_verify_batch_keys", "ug_ultra_groth_verify_batch_keys", "ug_groth16_verify_batch_records_keys",
                 "ug_ultra_groth_verify_batch_records_keys", "ug_test_tree_forest"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.VERIFIER_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_lib.VerifyBatchStatsKeys) == 88 and _lib.VerifyBatchStatsKeys.segments.offset == 64
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"f12_forest_kernel" in blob and b"g1_forest_kernel" in blob and blob.count(b"judge_kernel") >= 2
    assert b"f12_tree_kernel" in blob                                           # the one-key calls keep their tree kernels
