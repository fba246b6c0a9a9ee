"""Shared by tests/test_verify_batch_host.py and tests/test_gpu_verify_batch.py: raw calls of the batch and single verifiers, the
kinds of bad proof, and the bound on the work of a rejected batch. Every expectation is the SINGLE verifier's verdict on the same
strings (groth16_verify / ultra_groth_verify), never the batch code's."""
import ctypes as C
import json
import math
import os

from conftest import GOLDEN
from oracle import pairing as PR

VALID, INVALID, ERROR = 0, 1, 2
TD = os.path.join(GOLDEN, "trapdoor")
Q = PR.P
SENTINEL = -7


def load(name, mode="rb"):
    with open(os.path.join(TD, name), mode) as f:
        return f.read()


def lib():
    import ultragroth_amd as ug
    return ug.load()


def _enc(v):
    return v if isinstance(v, bytes) else (v if isinstance(v, str) else json.dumps(v)).encode()


def single(ultra, proof, pub, vk):
    """the verdict of the single-proof call"""
    L = lib()
    fn = L.ultra_groth_verify if ultra else L.groth16_verify
    return fn(_enc(proof), _enc(pub), _enc(vk), None, 0)


def batch(ultra, proofs, pubs, vk, device=-1):
    """raw call: (rc, message, verdicts, stats dict)"""
    from ultragroth_amd._lib import VerifyBatchStats
    L = lib()
    fn = L.ug_ultra_groth_verify_batch if ultra else L.ug_groth16_verify_batch
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[_enc(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[_enc(p) for p in pubs])
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStats(), C.create_string_buffer(512)
    rc = fn(device, n, pa, ia, _enc(vk), verdicts, C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), {f: getattr(stats, f) for f, _ in VerifyBatchStats._fields_}


def check_bound(count, bad, stats):
    """A rejected pass of `count` proofs with `bad` bad ones: the root check, then two checks per bad proof and level while the
    failing node still covers more than 16 proofs -- the tree has ceil(log2(count / 16)) such levels -- and the single verifier for
    the at most 16 proofs of each failing node at the bottom."""
    levels = max(0, math.ceil(math.log2(count / 16))) if count else 0
    assert stats["batch_checks"] <= 1 + 2 * bad * levels, stats
    assert stats["single_checks"] <= 16 * bad, stats


# ---- bad proofs -----------------------------------------------------------------------------------------------------------
def _g1(j):
    return None if (int(j[0]), int(j[1])) == (0, 0) else (int(j[0]), int(j[1]))


def _j1(p):
    return ["0", "0", "1"] if p is None else [str(p[0]), str(p[1]), "1"]


def f2_sqrt(a):
    """square root in Fq2 = Fq[u]/(u^2+1), q = 3 mod 4 (complex method); None when a is no square"""
    a1 = PR.f2_pow(a, (Q - 3) // 4)
    x0 = PR.f2_mul(a1, a)
    alpha = PR.f2_mul(a1, x0)
    if alpha == (Q - 1, 0):
        x = PR.f2_mul((0, 1), x0)
    else:
        x = PR.f2_mul(PR.f2_pow(PR.f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    return x if PR.f2_mul(x, x) == a else None


def off_subgroup_b():
    """a point of the twist outside the subgroup of order r, built as tests/test_gpu_validate.py builds its P"""
    b2 = PR.f2_muls(PR.f2_inv(PR.XI), 3)
    x = (1, 0)
    y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), b2))
    assert y is not None and PR.g2_on_curve((x, y))
    return [[str(x[0]), str(x[1])], [str(y[0]), str(y[1])], ["1", "0"]]


def c_name(ultra):
    return "pi_f" if ultra else "pi_c"


def bad_proof(kind, proof, pub, ultra=False):
    """one valid (proof, pub) pair of strings -> the tampered pair"""
    p, s = json.loads(proof), json.loads(pub)
    if kind == "signal+1":
        s[0] = str(int(s[0]) + 1)
    elif kind == "A.y negated":
        p["pi_a"][1] = str(Q - int(p["pi_a"][1]))
    elif kind == "C = generator":
        p[c_name(ultra)] = ["1", "2", "1"]
    elif kind == "json syntax":
        return proof[:-1], pub
    elif kind == "A = infinity":
        p["pi_a"] = ["0", "0", "1"]
    elif kind == "B off subgroup":
        p["pi_b"] = off_subgroup_b()
    elif kind == "C off curve":
        p[c_name(ultra)][1] = str(int(p[c_name(ultra)][1]) ^ 1)
    elif kind == "signal count":
        s = s[:-1] + ["1", "1"]
    else:
        raise KeyError(kind)
    return json.dumps(p), json.dumps(s)


KINDS = ["signal+1", "A.y negated", "C = generator", "json syntax", "A = infinity", "B off subgroup", "C off curve", "signal count"]


def cancelling_pair(proof1, proof2, ultra=False):
    """C_1 + D and C_2 - D with D = (1, 2): the two errors cancel in any combination with equal weights"""
    a, b = json.loads(proof1), json.loads(proof2)
    d = (1, 2)
    a[c_name(ultra)] = _j1(PR.g1_add(_g1(a[c_name(ultra)]), d))
    b[c_name(ultra)] = _j1(PR.g1_add(_g1(b[c_name(ultra)]), PR.g1_neg(d)))
    return json.dumps(a), json.dumps(b)


# ---- records for the Miller exports ------------------------------------------------------------------------------------------
def mont(x):
    return (x * (1 << 256) % Q).to_bytes(32, "little")


def g1_rec(j):
    return mont(int(j[0])) + mont(int(j[1]))


def g2_rec(j):
    return mont(int(j[0][0])) + mont(int(j[0][1])) + mont(int(j[1][0])) + mont(int(j[1][1]))


def product_miller(g1, g2):
    """the product library's host Miller loop (test hook) of zkey records: 108 limbs"""
    out = (C.c_uint32 * 108)()
    assert lib().ug_test_miller(g1, g2, out) == 0
    return list(out)


def trace(index):
    """(r, f) of proof `index` of the last batch call: the 128-bit scalar and the 108 limbs of miller(B, r A)"""
    r, f = (C.c_uint32 * 4)(), (C.c_uint32 * 108)()
    assert lib().ug_test_verify_batch_trace(index, r, f) == 0
    return sum(int(w) << (32 * k) for k, w in enumerate(r)), list(f)
