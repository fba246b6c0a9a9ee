"""Shared by tests/test_verify_records_host.py and tests/test_gpu_verify_records.py: raw calls of the packed-record entry points, the
kinds of bad record, and the single verifier's verdict on the text a record stands for. Every expectation is that verdict
(groth16_verify / ultra_groth_verify on the UNPACKED text of the same record), never the batch code's."""
import ctypes as C
import json

import verify_batch_cases as VB
from verify_batch_cases import VALID, INVALID, ERROR, SENTINEL
from oracle import pairing as PR

Q = PR.P
R = PR.R

# the kinds of verify_batch_cases that a record can hold (a record cannot fail to parse or carry another signal count)
KINDS = ["signal+1", "A.y negated", "C = generator", "A = infinity", "B off subgroup", "C off curve"]
BINARY_KINDS = ["pi_a.x + q", "input + r", "coordinate 2^256 - 1", "B = infinity", "all-zero record"]


def rec_size(ultra):
    return 320 if ultra else 256


def pack(proof, ultra=False):
    rec = C.create_string_buffer(rec_size(ultra))
    assert VB.lib().ug_proof_pack(1 if ultra else 0, VB._enc(proof), rec) == 0
    return rec.raw


def pack_inputs(pub):
    n_pub = len(json.loads(pub) if isinstance(pub, (str, bytes)) else pub)
    out = C.create_string_buffer(32 * n_pub)
    assert VB.lib().ug_inputs_pack(VB._enc(pub), out, n_pub) == 0
    return out.raw


def unpack(rec, ultra=False):
    out = C.create_string_buffer(1400)
    assert VB.lib().ug_proof_unpack(1 if ultra else 0, rec, out, 1400) == 0
    return out.value.decode()


def unpack_inputs(block):
    n_pub = len(block) // 32
    out = C.create_string_buffer(81 * n_pub + 3)
    assert VB.lib().ug_inputs_unpack(block, n_pub, out, 81 * n_pub + 3) == 0
    return out.value.decode()


def single(ultra, rec, block, vk):
    """the single verifier's verdict on the texts that (record, input block) stand for"""
    return VB.single(ultra, unpack(rec, ultra), unpack_inputs(block), vk)


def expected(ultra, recs, blocks, vk):
    return [single(ultra, r, b, vk) for r, b in zip(recs, blocks)]


def options(judge, search_width=-1, judge_min=-1):
    from ultragroth_amd._lib import VerifyBatchOptions
    return VerifyBatchOptions(C.sizeof(VerifyBatchOptions), int(judge), search_width, judge_min)


def _stats(stats):
    from ultragroth_amd._lib import VerifyBatchStats
    out = {f: getattr(stats.base, f) for f, _ in VerifyBatchStats._fields_}
    out.update({f: getattr(stats, f) for f in ("judged", "judge_launches", "judge_ms")})
    return out


def batch_records(ultra, recs, blocks, vk, device=-1, opt=None, n_pub=None):
    """raw call: (rc, message, verdicts, stats dict); opt: None (the environment) or options(...)"""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_records if ultra else L.ug_groth16_verify_batch_records
    n = len(recs)
    if n_pub is None:
        n_pub = len(blocks[0]) // 32 if blocks else len(vk["IC"]) - 1
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStatsEx(), C.create_string_buffer(512)
    rc = fn(device, n, b"".join(recs) or b"\0", b"".join(blocks) or b"\0", n_pub, VB._enc(vk), verdicts,
            C.byref(opt) if opt is not None else None, C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), _stats(stats)


def batch_json_opt(ultra, proofs, pubs, vk, device=-1, opt=None):
    """ug_*_verify_batch_opt on texts: (rc, message, verdicts, stats dict)"""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_opt if ultra else L.ug_groth16_verify_batch_opt
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in pubs])
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStatsEx(), C.create_string_buffer(512)
    rc = fn(device, n, pa, ia, VB._enc(vk), verdicts, C.byref(opt) if opt is not None else None, C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), _stats(stats)


def bad_record(kind, proof, pub, ultra=False):
    """one valid (proof, pub) pair of texts -> the tampered (record, input block)"""
    p, s = VB.bad_proof(kind, proof, pub, ultra=ultra)
    return pack(p, ultra), pack_inputs(s)


def _put(rec, at, value):
    return rec[:at] + value.to_bytes(32, "little") + rec[at + 32:]


def _get(rec, at):
    return int.from_bytes(rec[at:at + 32], "little")


def binary_record(kind, rec, block):
    """records that no decimal text written by a prover would give: values at or above the moduli, infinity, all zero"""
    if kind == "pi_a.x + q":
        return _put(rec, 0, _get(rec, 0) + Q), block
    if kind == "pi_b.y.c1 + q":
        return _put(rec, 160, _get(rec, 160) + Q), block
    if kind == "input + r":
        return rec, _put(block, 0, _get(block, 0) + R)
    if kind == "coordinate 2^256 - 1":
        return _put(rec, 32, (1 << 256) - 1), block
    if kind == "B = infinity":
        return rec[:64] + bytes(128) + rec[192:], block
    if kind == "all-zero record":
        return bytes(len(rec)), block
    raise KeyError(kind)


def mixed_batch(recs, blocks, proofs, pubs, ultra=False):
    """five kinds of bad record among the valid ones, as test_several_bad_proofs places them; needs at least 33 records"""
    recs, blocks = list(recs), list(blocks)
    for at, kind in ((0, "A.y negated"), (15, "C off curve"), (16, "C = generator"), (31, "B off subgroup"), (32, "A = infinity")):
        recs[at], blocks[at] = bad_record(kind, proofs[at], pubs[at], ultra)
    return recs, blocks


def passes():
    """(in place, gathered): how the passes of the last records call on a device used their resident arrays (test hook)"""
    out = (C.c_ulonglong * 2)()
    assert VB.lib().ug_test_verify_records_passes(out) == 0
    return out[0], out[1]
