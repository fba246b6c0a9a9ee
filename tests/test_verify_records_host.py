"""ug_groth16_verify_batch_records / ug_ultra_groth_verify_batch_records with device = -1, and the pack / unpack calls: no GPU.
Proofs are the oracle's, of the trapdoor fixtures; every expected verdict is the single-proof verifier's on the text the record
stands for, and every intended-bad record is first shown to be INVALID there."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import oracle as O
import verify_batch_cases as VB
import verify_records_cases as VR
from verify_batch_cases import VALID, INVALID, ERROR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g16():
    zkey, wtns, vk = VB.load("groth16.zkey"), VB.load("groth16.wtns"), json.loads(VB.load("groth16_vkey.json", "r"))
    pairs = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(33)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert len(set(recs)) == 33 and all(len(r) == 256 for r in recs)
    assert VR.expected(False, recs, blocks, vk) == [VALID] * 33
    return proofs, pubs, recs, blocks, vk


@pytest.fixture(scope="module")
def ultra():
    zkey, uwtns, vk = VB.load("ultra.zkey"), VB.load("ultra.uwtns"), json.loads(VB.load("ultra_vkey.json", "r"))
    pairs = [O.ultra_groth_prove(zkey, uwtns, 10 + i, 200 + i, 3000 + i)[:2] for i in range(17)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert all(len(r) == 320 for r in recs) and VR.expected(True, recs, blocks, vk) == [VALID] * 17
    return proofs, pubs, recs, blocks, vk


def test_round_trip(g16):
    proofs, pubs, recs, blocks, vk = g16
    cases = [(proofs[0], pubs[0])] + [VB.bad_proof(kind, proofs[1], pubs[1]) for kind in VR.KINDS]
    for proof, pub in cases:
        rec, block = VR.pack(proof), VR.pack_inputs(pub)
        text, ins = VR.unpack(rec), VR.unpack_inputs(block)
        assert VB.single(False, text, ins, vk) == VB.single(False, proof, pub, vk)
        assert VR.pack(text) == rec and VR.pack_inputs(ins) == block
        assert json.loads(text)["pi_a"][:2] == json.loads(proof)["pi_a"][:2] and json.loads(ins) == json.loads(pub)
    assert [VB.single(False, p, s, vk) for p, s in cases] == [VALID] + [INVALID] * len(VR.KINDS)
    for kind in VR.BINARY_KINDS:                                                   # records no text of a prover gives still round-trip
        rec, block = VR.binary_record(kind, recs[2], blocks[2])
        assert VR.pack(VR.unpack(rec)) == rec and VR.pack_inputs(VR.unpack_inputs(block)) == block


def test_pack_refuses_what_a_record_cannot_hold(g16):
    proofs, pubs, recs, blocks, vk = g16
    L = VB.lib()
    rec = C.create_string_buffer(b"\x55" * 256, 256)
    big = json.loads(proofs[0])
    big["pi_c"][0] = str(1 << 256)
    edge = json.loads(proofs[0])
    edge["pi_c"][0] = str((1 << 256) - 1)
    for text in (proofs[0][:-1], "", "[]", json.dumps(big), proofs[0].replace("groth16", "ultragroth")):
        assert L.ug_proof_pack(0, text.encode(), rec) == 1 and rec.raw == b"\x55" * 256
    assert L.ug_proof_pack(0, json.dumps(edge).encode(), rec) == 0 and rec.raw[192:224] == b"\xff" * 32
    assert L.ug_proof_pack(1, proofs[0].encode(), rec) == 1 and L.ug_proof_pack(0, None, rec) == 1
    out = C.create_string_buffer(96)
    assert L.ug_inputs_pack(pubs[0].encode(), out, len(json.loads(pubs[0])) + 1) == 1
    assert L.ug_inputs_pack(b"[", out, 1) == 1 and L.ug_inputs_pack(json.dumps([str(1 << 256)]).encode(), out, 1) == 1
    small = C.create_string_buffer(64)
    assert L.ug_proof_unpack(0, recs[0], small, 64) == 1 and L.ug_inputs_unpack(blocks[0], len(blocks[0]) // 32, small, 4) == 1


@pytest.mark.parametrize("count", [0, 1, 2, 17, 33])
def test_valid_batches(g16, count):
    proofs, pubs, recs, blocks, vk = g16
    rc, msg, verdicts, stats = VR.batch_records(False, recs[:count], blocks[:count], vk)
    assert (rc, msg, verdicts) == (VALID, "", [VALID] * count)
    assert stats["batch_checks"] == (1 if count else 0) and stats["single_checks"] == 0 and stats["off_subgroup"] == 0


@pytest.mark.parametrize("at", [0, 16, 32])
@pytest.mark.parametrize("kind", VR.KINDS)
def test_kinds_of_bad_record(g16, kind, at):
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = list(recs), list(blocks)
    recs[at], blocks[at] = VR.bad_record(kind, proofs[at], pubs[at])
    expect = VR.expected(False, recs, blocks, vk)
    assert expect[at] == INVALID and expect.count(VALID) == 32
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk)
    assert rc == INVALID and verdicts == expect and msg == "proof %d: invalid proof" % at
    if kind == "B off subgroup":
        assert stats["off_subgroup"] == 1 and stats["single_checks"] == 1 and stats["batch_checks"] == 1
    elif kind == "C off curve":                                                   # answered without a pairing: the other 32 hold
        assert stats["single_checks"] == 0 and stats["batch_checks"] == 1
    else:
        VB.check_bound(33, 1, stats)


def test_cancelling_pair(g16):
    proofs, pubs, recs, blocks, vk = g16
    recs = list(recs[:20])
    a, b = VB.cancelling_pair(proofs[3], proofs[18])
    recs[3], recs[18] = VR.pack(a), VR.pack(b)
    expect = VR.expected(False, recs, blocks[:20], vk)
    assert [i for i, v in enumerate(expect) if v == INVALID] == [3, 18]
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks[:20], vk)
    assert rc == INVALID and verdicts == expect
    VB.check_bound(20, 2, stats)


@pytest.mark.parametrize("kind", VR.BINARY_KINDS)
def test_binary_only_kinds(g16, kind):
    """whatever the single verifier says of the unpacked text is the expectation (a value + modulus reduces to the valid proof)"""
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = list(recs[:19]), list(blocks[:19])
    recs[17], blocks[17] = VR.binary_record(kind, recs[17], blocks[17])
    expect = VR.expected(False, recs, blocks, vk)
    assert expect[:17] + expect[18:] == [VALID] * 18 and expect[17] in (VALID, INVALID)
    rc, msg, verdicts, stats = VR.batch_records(False, recs, blocks, vk)
    assert verdicts == expect and rc == (VALID if expect[17] == VALID else INVALID)
    assert msg == ("" if rc == VALID else "proof 17: invalid proof")


def test_argument_errors(g16):
    proofs, pubs, recs, blocks, vk = g16
    L = VB.lib()
    key = json.dumps(vk).encode()
    n_pub = len(blocks[0]) // 32
    rb, ib = recs[0] + recs[1], blocks[0] + blocks[1]
    for args, text in (((2, None, ib, n_pub, key), "null argument"), ((2, rb, None, n_pub, key), "null argument"),
                       ((2, rb, ib, n_pub, None), "null argument"), ((-1, rb, ib, n_pub, key), "null argument"),
                       ((2, rb, ib, 0, key), "invalid inputs data"), ((2, rb, ib, -3, key), "invalid inputs data"),
                       ((2, rb, ib, n_pub + 1, key), "len(inputs)+1 != len(vk.IC)"), ((2, rb, ib, n_pub - 1 or 7, key), "len(inputs)+1 != len(vk.IC)"),
                       ((2, rb, ib, n_pub, key[:len(key) // 2]), "invalid verification key data")):
        verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
        err = C.create_string_buffer(256)
        count, r, i, np_, k = args
        assert L.ug_groth16_verify_batch_records(-1, count, r, i, np_, k, verdicts, None, None, err, 255) == ERROR
        assert err.value.decode() == text and list(verdicts) == [VB.SENTINEL] * 2
    assert L.ug_groth16_verify_batch_records(-1, 2, rb, ib, n_pub, key, None, None, None, None, 0) == ERROR
    assert L.ug_groth16_verify_batch_records(-1, 0, None, None, n_pub, key, None, None, None, None, 0) == VALID
    verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
    assert L.ug_groth16_verify_batch_records(-1, 2, rb, ib, n_pub, key, verdicts, None, None, None, 0) == VALID and list(verdicts) == [VALID] * 2
    assert L.ug_ultra_groth_verify_batch_records(-1, 2, rb, ib, n_pub, key, verdicts, None, None, None, 0) == ERROR       # a Groth16 key
    bad = VR.options(2)
    assert L.ug_groth16_verify_batch_records(-1, 2, rb, ib, n_pub, key, verdicts, C.byref(bad), None, None, 0) == ERROR


@pytest.mark.parametrize("count", [3, 17])
def test_ultragroth(ultra, count):
    proofs, pubs, recs, blocks, vk = ultra
    rc, msg, verdicts, stats = VR.batch_records(True, recs[:count], blocks[:count], vk)
    assert (rc, verdicts, stats["batch_checks"], stats["single_checks"]) == (VALID, [VALID] * count, 1, 0)
    recs, blocks = list(recs[:count]), list(blocks[:count])
    last = count - 1
    recs[last] = recs[last][:256] + recs[0][256:]                                 # another proof's round commitment: the challenge moves
    recs[1], blocks[1] = VR.bad_record("C = generator", proofs[1], pubs[1], ultra=True)
    expect = VR.expected(True, recs, blocks, vk)
    assert expect[1] == INVALID and expect[last] == INVALID and expect.count(VALID) == count - 2
    rc, msg, verdicts, stats = VR.batch_records(True, recs, blocks, vk)
    assert rc == INVALID and verdicts == expect and msg == "proof 1: invalid proof"
    VB.check_bound(count, 2, stats)


def test_ultragroth_cancelling_pair_of_pi_f(ultra):
    proofs, pubs, recs, blocks, vk = ultra
    recs = list(recs[:4])
    a, b = VB.cancelling_pair(proofs[0], proofs[2], ultra=True)
    recs[0], recs[2] = VR.pack(a, True), VR.pack(b, True)
    expect = VR.expected(True, recs, blocks[:4], vk)
    assert expect == [INVALID, VALID, INVALID, VALID]
    assert VR.batch_records(True, recs, blocks[:4], vk)[2] == expect


@pytest.mark.parametrize("judge", [0, 1])
def test_agreement_with_the_json_path(g16, judge):
    proofs, pubs, recs, blocks, vk = g16
    recs, blocks = VR.mixed_batch(recs, blocks, proofs, pubs)
    expect = VR.expected(False, recs, blocks, vk)
    assert [i for i, v in enumerate(expect) if v != VALID] == [0, 15, 16, 31, 32] and expect.count(INVALID) == 5
    opt = VR.options(judge, judge_min=1)
    texts, ins = [VR.unpack(r) for r in recs], [VR.unpack_inputs(b) for b in blocks]
    rc_j, msg_j, verdicts_j, stats_j = VR.batch_json_opt(False, texts, ins, vk, opt=opt)
    rc_r, msg_r, verdicts_r, stats_r = VR.batch_records(False, recs, blocks, vk, opt=opt)
    assert (rc_r, msg_r, verdicts_r) == (rc_j, msg_j, verdicts_j) == (INVALID, "proof 0: invalid proof", expect)
    assert stats_r["off_subgroup"] == stats_j["off_subgroup"] == 1
    assert (stats_r["judged"] > 0) == (stats_j["judged"] > 0) == bool(judge)


def test_key_the_batch_refuses_keeps_its_path(g16):
    proofs, pubs, recs, blocks, vk = g16
    key = dict(vk)
    key["vk_gamma_2"] = VB.off_subgroup_b()
    expect = VR.expected(False, recs[:4], blocks[:4], key)
    rc, msg, verdicts, stats = VR.batch_records(False, recs[:4], blocks[:4], key)
    assert verdicts == expect and stats["single_checks"] == 4 and stats["batch_checks"] == 0


def test_python_entry_points(g16):
    import ultragroth_amd as ug
    proofs, pubs, recs, blocks, vk = g16
    assert ug.proof_pack(proofs[0]) == recs[0] and ug.proof_pack(json.loads(proofs[0])) == recs[0]
    assert ug.inputs_pack(pubs[0]) == blocks[0] and ug.inputs_unpack(blocks[0]) == VR.unpack_inputs(blocks[0])
    assert ug.proof_unpack(recs[0]) == VR.unpack(recs[0])
    with pytest.raises(ValueError):
        ug.proof_pack(proofs[0][:-1])
    n_pub = len(blocks[0]) // 32
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(recs[:3]), b"".join(blocks[:3]), n_pub, vk, device=-1)
    assert verdicts == [VALID] * 3 and stats["batch_checks"] == 1 and stats["host_ms"] > 0 and stats["device_ms"] == 0
    with pytest.raises(ug.VerifierError, match="invalid verification key data"):
        ug.groth16_verify_batch_records(b"".join(recs[:3]), b"".join(blocks[:3]), n_pub, "{", device=-1)
    assert ug.groth16_verify_batch_records(b"", b"", n_pub, vk, device=-1)[0] == []
    assert callable(ug.ultra_groth_verify_batch_records) and callable(ug.Device.points_check_mask)


NEW_VERIFIER = ["ug_groth16_verify_batch_records", "ug_ultra_groth_verify_batch_records", "ug_proof_pack", "ug_inputs_pack",
                "ug_proof_unpack", "ug_inputs_unpack"]


def test_symbols_are_declared_listed_and_exported():
    import ultragroth_amd as ug
    from ultragroth_amd import _lib
    lib = ug.load()
    inner = open(os.path.join(ROOT, "include", "ultragroth_hip.h")).read()
    outer = open(os.path.join(ROOT, "include", "verifier.h")).read()
    assert re.search(r"\bug_points_check_mask\s*\(", inner) and "ug_points_check_mask" in _lib.INNER_SYMBOLS and hasattr(lib, "ug_points_check_mask")
    for name in NEW_VERIFIER:
        assert re.search(r"\b%s\s*\(" % name, outer) and name in _lib.VERIFIER_SYMBOLS and hasattr(lib, name), name
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"records_ingest_kernel" in blob and b"gather_rows_kernel" in blob and b"StatusBytes" in blob


def test_headers_compile_as_plain_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    inc = os.path.join(ROOT, "include")
    for h in ("verifier.h", "ultragroth_hip.h"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c", "-"],
                           input='#include "%s"\n' % h, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
