"""The judge of batch verification without a GPU: the final exponentiation of pairing.hpp against the oracle's, and
ug_groth16_verify_batch_opt with judge = 1 and device = -1 -- the breadth-first search of a rejected pass and the suspects decided by
their own equations, the shared code on host threads. Every expected verdict is the single-proof verifier's on the same strings."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest

import oracle as O
import verify_batch_cases as VB
import verify_judge_cases as VJ
from verify_batch_cases import VALID, INVALID, ERROR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
NO_PAIRING = ("json syntax", "signal count", "C off curve")          # answered by the parser / the curve check


@pytest.fixture(scope="module")
def g16():
    zkey, wtns, vk = VB.load("groth16.zkey"), VB.load("groth16.wtns"), json.loads(VB.load("groth16_vkey.json", "r"))
    pairs = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(33)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    return proofs, pubs, vk


@pytest.fixture(scope="module")
def tampered(g16):
    """kind -> (proofs, pubs, the single verifier's verdicts): 33 proofs, a bad one of that kind at 0, 16 and 32"""
    proofs, pubs, vk = g16
    out = {}
    for kind in VB.KINDS:
        p, s = list(proofs), list(pubs)
        for at in (0, 16, 32):
            p[at], s[at] = VB.bad_proof(kind, p[at], s[at])
        expect = [VB.single(False, p[i], s[i], vk) if i in (0, 16, 32) else VALID for i in range(33)]
        assert all(expect[i] == (ERROR if kind in ("json syntax", "signal count") else INVALID) for i in (0, 16, 32))
        out[kind] = (p, s, expect)
    return out


def test_final_exp_against_the_oracle(g16):
    """ugt_final_exp is pairing.hpp's final exponentiation under the range assertions: its verdict is oracle.pairing.final_exp's for a
    valid proof's Miller product (one), the product with a tampered pair (not one), 1 (one) and 0 (not one)"""
    proofs, pubs, vk = g16
    subprocess.check_call(["make", "-s", "-C", CSRC, os.path.join(CSRC, "libug_hostmath_test.so")])
    T = C.CDLL(os.path.join(CSRC, "libug_hostmath_test.so"))
    values = VJ.final_exp_values(proofs[0], pubs[0], vk)
    assert [one for _, _, one in values] == [True, False, True, False]
    for name, f, one in values:
        fin, g = (C.c_uint32 * 108)(*VJ.f12_limbs(f)), (C.c_uint32 * 108)()
        assert T.ugt_final_exp(g, fin) == int(one), name
        assert all(w < (1 << 29) for w in g), name
        assert any(g) == (name != "zero"), name
        if one:                                                     # the value after the hard part lies in Fq6: no odd coefficient
            assert not any(g[9 * k + i] for k in range(1, 12, 2) for i in range(9)), name


@pytest.mark.parametrize("kind", VB.KINDS)
def test_whole_pass_judged(g16, tampered, kind):
    """search_width = 0: no host search, a rejected pass is suspect as a whole; judge_min = 1: the judge decides every suspect"""
    vk = g16[2]
    proofs, pubs, expect = tampered[kind]
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=-1, judge=1, search_width=0, judge_min=1)
    assert rc == INVALID and verdicts == expect and msg.startswith("proof 0: ")
    assert stats["batch_checks"] == 1 and stats["single_checks"] == 0
    # proofs that reach a pairing in the judge: none when the three bad ones were answered before (the other 30 pass the root check),
    # the three off-subgroup ones alone when they were set aside (the other 30 pass), else the whole rejected pass
    judged = 0 if kind in NO_PAIRING else 3 if kind == "B off subgroup" else 33
    assert stats["judged"] == judged and stats["off_subgroup"] == (3 if kind == "B off subgroup" else 0)
    assert stats["judge_launches"] == 0 and stats["judge_ms"] == 0 and stats["device_ms"] == 0       # host threads


@pytest.mark.parametrize("kind", VB.KINDS)
def test_search_width_4(g16, tampered, kind):
    vk = g16[2]
    proofs, pubs, expect = tampered[kind]
    rc, msg, verdicts, stats = VJ.batch_opt(False, proofs, pubs, vk, device=-1, judge=1, search_width=4, judge_min=1)
    assert rc == INVALID and verdicts == expect
    levels = math.ceil(math.log2(33 / 16))
    assert 1 <= stats["batch_checks"] <= 1 + 2 * 4 * levels and stats["single_checks"] == 0
    # the same inputs with the judge off: verdicts, result and message are the same
    assert VB.batch(False, proofs, pubs, vk)[:3] == (rc, msg, verdicts)


def test_few_suspects_go_to_the_single_verifier(g16, tampered):
    """below judge_min the suspects of the search are verified one by one, as with the judge off: one bad proof does the same work"""
    proofs, pubs, vk = g16
    proofs, pubs = list(proofs), list(pubs)
    proofs[16], pubs[16] = VB.bad_proof("signal+1", proofs[16], pubs[16])
    on = VJ.batch_opt(False, proofs, pubs, vk, device=-1, judge=1)
    off = VJ.batch_opt(False, proofs, pubs, vk, device=-1, judge=0)
    plain = VB.batch(False, proofs, pubs, vk)
    assert on[:3] == off[:3] == plain[:3] and on[2][16] == INVALID
    for f in ("batch_checks", "single_checks", "off_subgroup"):
        assert on[3][f] == off[3][f] == plain[3][f], f
    assert on[3]["judged"] == 0 and off[3]["judged"] == 0 and 1 <= on[3]["single_checks"] <= 16


def test_option_errors(g16):
    from ultragroth_amd._lib import VerifyBatchOptions, VerifyBatchStatsEx
    proofs, pubs, vk = g16
    L = VB.lib()
    pa, ia = (C.c_char_p * 1)(proofs[0].encode()), (C.c_char_p * 1)(pubs[0].encode())
    for opt, text in ((VerifyBatchOptions(8, 1, -1, -1), "size"), (VerifyBatchOptions(16, 2, -1, -1), "judge")):
        verdicts, err = (C.c_int * 1)(VB.SENTINEL), C.create_string_buffer(256)
        assert L.ug_groth16_verify_batch_opt(-1, 1, pa, ia, json.dumps(vk).encode(), verdicts, C.byref(opt), None, err, 255) == ERROR
        assert text in err.value.decode() and verdicts[0] == VB.SENTINEL
    verdicts = (C.c_int * 1)(VB.SENTINEL)
    assert L.ug_groth16_verify_batch_opt(-1, 1, pa, ia, json.dumps(vk).encode(), verdicts, None, None, None, 0) == VALID and verdicts[0] == VALID


def test_python_entry_point(g16, tampered):
    import ultragroth_amd as ug
    vk = g16[2]
    proofs, pubs, expect = tampered["A.y negated"]
    verdicts, stats = ug.groth16_verify_batch(proofs, pubs, vk, device=-1, judge=True, search_width=0, judge_min=1)
    assert verdicts == expect and stats["judged"] == 33 and stats["single_checks"] == 0 and stats["judge_launches"] == 0
    verdicts, stats = ug.groth16_verify_batch(proofs, pubs, vk, device=-1)
    assert verdicts == expect and "judged" not in stats


_CHILD = """
import ctypes as C, json, sys
sys.path.insert(0, %r)
import conftest
import verify_batch_cases as VB
from ultragroth_amd._lib import VerifyBatchStats
proofs, pubs, vk = json.load(sys.stdin)
L = VB.lib()
n = len(proofs)
pa, ia = (C.c_char_p * n)(*[p.encode() for p in proofs]), (C.c_char_p * n)(*[p.encode() for p in pubs])
verdicts, err = (C.c_int * n)(*([VB.SENTINEL] * n)), C.create_string_buffer(512)
raw = (C.c_ubyte * 64)(*([0xAB] * 64))
rc = L.ug_groth16_verify_batch(-1, n, pa, ia, json.dumps(vk).encode(), verdicts, raw, err, 511)
stats = VerifyBatchStats.from_buffer_copy(bytes(raw)[:40])
print(json.dumps({"rc": rc, "msg": err.value.decode(), "verdicts": list(verdicts), "tail": list(raw)[40:],
                  "batch_checks": stats.batch_checks, "single_checks": stats.single_checks}))
"""


def _child(setting, proofs, pubs, vk):
    env = dict(os.environ)
    env.pop("ULTRAGROTH_VERIFY_JUDGE", None)
    if setting is not None:
        env["ULTRAGROTH_VERIFY_JUDGE"] = setting
    out = subprocess.run([sys.executable, "-c", _CHILD % os.path.join(ROOT, "tests")], input=json.dumps([proofs, pubs, vk]), env=env, cwd=ROOT,
                         capture_output=True, text=True, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_environment_switch(g16):
    """ULTRAGROTH_VERIFY_JUDGE=1 through the old entry point, library defaults: 260 bad proofs are more than judge_min suspects, so the
    judge decides them and the 40-byte stats show no single verification; with 0, as unset, the single verifier decides all of them"""
    proofs, pubs, vk = g16
    bad = [VB.bad_proof("signal+1", p, s) for p, s in zip(proofs, pubs)]
    assert [VB.single(False, p, s, vk) for p, s in bad] == [INVALID] * 33
    n = 260
    ps, ss = [bad[i % 33][0] for i in range(n)], [bad[i % 33][1] for i in range(n)]
    ps[7], ss[7] = proofs[7], pubs[7]                                            # one valid proof among them
    expect = [INVALID] * n
    expect[7] = VALID
    on = _child("1", ps, ss, vk)
    assert on["rc"] == INVALID and on["verdicts"] == expect and on["msg"] == "proof 0: invalid proof"
    assert on["single_checks"] == 0 and on["tail"] == [0xAB] * 24
    off = _child("0", ps, ss, vk)
    assert (off["rc"], off["verdicts"], off["msg"]) == (on["rc"], on["verdicts"], on["msg"])
    assert off["single_checks"] == n and off["tail"] == [0xAB] * 24
    unset = VB.batch(False, ps, ss, vk)                                           # this process: the variable is not set
    assert "ULTRAGROTH_VERIFY_JUDGE" not in os.environ and unset[:3] == (off["rc"], off["msg"], off["verdicts"])
    assert unset[3]["single_checks"] == n and unset[3]["batch_checks"] == off["batch_checks"]
    for setting in ("yes", "2", "11"):
        wrong = _child(setting, ps[:2], ss[:2], vk)
        assert wrong["rc"] == ERROR and "ULTRAGROTH_VERIFY_JUDGE" in wrong["msg"] and wrong["verdicts"] == [VB.SENTINEL] * 2


def test_abi():
    """the new symbols are exported; the structures have the sizes of include/verifier.h; the old entry points keep the 40-byte stats"""
    from ultragroth_amd import _lib
    L = VB.lib()
    for name in ("ug_groth16_verify_batch_opt", "ug_ultra_groth_verify_batch_opt", "ug_test_final_exp"):
        assert hasattr(L, name) and name in _lib.VERIFIER_SYMBOLS
    assert C.sizeof(_lib.VerifyBatchStats) == 40 and C.sizeof(_lib.VerifyBatchOptions) == 16 and C.sizeof(_lib.VerifyBatchStatsEx) == 64
    assert _lib.VerifyBatchStatsEx.base.offset == 0 and _lib.VerifyBatchStatsEx.judged.offset == 40
