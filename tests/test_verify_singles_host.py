"""The proofs a batch call decides one by one (device = -1): every proof under a key the batch refuses, the proofs whose pi_b is outside
the subgroup and the suspects of a rejected pass. They are decided from what the call has already parsed, so every verdict and the
call's message are compared with groth16_verify / ultra_groth_verify on the same proof as text -- for JSON texts and for packed
records in all three layouts. No GPU. Proofs are the oracle's, of the trapdoor fixtures; the tampering is verify_batch_cases'."""
import ctypes as C
import json

import pytest

import oracle as O
import verify_batch_cases as VB
import verify_records_cases as VR
import verify_formats_cases as VF
from verify_batch_cases import VALID, INVALID, ERROR
from verify_formats_cases import PLAIN, EVM, COMPRESSED

N = 6
LAYOUTS = ["json", PLAIN, EVM, COMPRESSED]
IDS = {"json": "json", PLAIN: "plain", EVM: "evm", COMPRESSED: "compressed"}


@pytest.fixture(scope="module")
def cases():
    """per protocol: N valid (proof, public) texts and the key"""
    zkey, wtns, vk = VB.load("groth16.zkey"), VB.load("groth16.wtns"), json.loads(VB.load("groth16_vkey.json", "r"))
    g16 = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(N)]
    zkey, uwtns, uvk = VB.load("ultra.zkey"), VB.load("ultra.uwtns"), json.loads(VB.load("ultra_vkey.json", "r"))
    ultra = [O.ultra_groth_prove(zkey, uwtns, 10 + i, 200 + i, 3000 + i)[:2] for i in range(N)]
    for is_ultra, pairs, key in ((False, g16, vk), (True, ultra, uvk)):
        assert all(VB.single(is_ultra, p, s, key) == VALID for p, s in pairs)
    return {False: (g16, vk), True: (ultra, uvk)}


def single(is_ultra, proof, pub, vk):
    """(verdict, message) of the single-proof call; proof / pub None: a null pointer"""
    L = VB.lib()
    fn = L.ultra_groth_verify if is_ultra else L.groth16_verify
    err = C.create_string_buffer(256)
    rc = fn(None if proof is None else VB._enc(proof), None if pub is None else VB._enc(pub), VB._enc(vk), err, 255)
    return rc, err.value.decode()


def call_says(singles):
    """what the batch call returns for proofs with these single answers: (rc, message, verdicts)"""
    verdicts = [rc for rc, _ in singles]
    bad = [i for i, rc in enumerate(verdicts) if rc != VALID]
    if not bad:
        return VALID, "", verdicts
    rc, msg = singles[bad[0]]
    return INVALID, "proof %d: %s" % (bad[0], msg if rc == ERROR else "invalid proof"), verdicts


def batch_json(is_ultra, proofs, pubs, vk):
    """ug_*_verify_batch_opt, judge off, on texts that may be null pointers: (rc, message, verdicts, stats)"""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_opt if is_ultra else L.ug_groth16_verify_batch_opt
    n = len(proofs)
    enc = lambda v: None if v is None else VB._enc(v)
    pa, ia = (C.c_char_p * n)(*[enc(p) for p in proofs]), (C.c_char_p * n)(*[enc(p) for p in pubs])
    verdicts = (C.c_int * n)(*([VB.SENTINEL] * n))
    stats, err, opt = VerifyBatchStatsEx(), C.create_string_buffer(512), VR.options(0)
    rc = fn(-1, n, pa, ia, VB._enc(vk), verdicts, C.byref(opt), C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts), VR._stats(stats)


def run(is_ultra, layout, pairs, kinds, vk):
    """The batch call, judge off, on `pairs` with pairs[i] tampered as kinds[i] (None: left valid), as texts or as records of a layout,
    beside the single verifier's answers on the texts the same proofs stand for: ((rc, message, verdicts), stats, expected)"""
    if layout == "json":
        texts = [VB.bad_proof(kind, p, s, ultra=is_ultra) if kind else (p, s) for (p, s), kind in zip(pairs, kinds)]
        rc, msg, verdicts, stats = batch_json(is_ultra, [p for p, _ in texts], [s for _, s in texts], vk)
        return (rc, msg, verdicts), stats, call_says([single(is_ultra, p, s, vk) for p, s in texts])
    recs, blocks, singles = [], [], []
    for (p, s), kind in zip(pairs, kinds):
        rec, block = VR.pack(p, is_ultra), VR.pack_inputs(s)
        if kind:
            r, b, stands = VF.expressed(layout, kind, rec, block, p, s, is_ultra)
        else:
            (r, b), stands = VF.to_format(layout, rec, block), (rec, block, None)
        recs.append(r)
        blocks.append(b)
        singles.append((VF.expected_one(is_ultra, stands, vk), ""))                   # a record always parses: VALID or INVALID
    if layout == PLAIN:
        rc, msg, verdicts, stats = VR.batch_records(is_ultra, recs, blocks, vk, opt=VR.options(0))
    else:
        rc, msg, verdicts, stats = VF.batch_fmt(is_ultra, layout, recs, blocks, vk, opt=VR.options(0))
    return (rc, msg, verdicts), stats, call_says(singles)


def off_curve_key(vk):
    key = json.loads(json.dumps(vk))
    key["IC"][1][1] = str(int(key["IC"][1][1]) ^ 1)
    return key


def off_subgroup_key(vk):
    key = dict(vk)
    key["vk_gamma_2"] = VB.off_subgroup_b()
    return key


@pytest.mark.parametrize("is_ultra", [False, True], ids=["groth16", "ultragroth"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: IDS[v])
@pytest.mark.parametrize("refused", [off_curve_key, off_subgroup_key], ids=["key off its curve", "gamma off the subgroup"])
def test_key_the_batch_refuses(cases, refused, layout, is_ultra):
    """(a), (b): no pass is made and every proof is the single verifier's, a point off its curve and infinity among them"""
    pairs, vk = cases[is_ultra]
    key = refused(vk)
    kinds = [None, "C off curve", None, "A = infinity", "signal+1", None]
    got, stats, want = run(is_ultra, layout, pairs, kinds, key)
    assert got == want
    assert stats["single_checks"] == N and stats["batch_checks"] == 0 and stats["off_subgroup"] == 0 and stats["judged"] == 0
    if refused is off_curve_key:                                                  # no pairing is defined under such a key
        assert want == (INVALID, "proof 0: invalid proof", [INVALID] * N)
    else:
        assert want[2][1] == want[2][4] == INVALID


@pytest.mark.parametrize("is_ultra", [False, True], ids=["groth16", "ultragroth"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: IDS[v])
def test_set_aside_and_suspects(cases, layout, is_ultra):
    """(c): a pi_b off the subgroup never meets the batch; the pass of the other five is rejected at its root and, being no larger
    than a leaf node, sends all five to the single verifier"""
    pairs, vk = cases[is_ultra]
    kinds = [None, "B off subgroup", None, None, "A.y negated", None]
    got, stats, want = run(is_ultra, layout, pairs, kinds, vk)
    assert got == want and want == (INVALID, "proof 1: invalid proof", [VALID, INVALID, VALID, VALID, INVALID, VALID])
    assert stats["off_subgroup"] == 1 and stats["batch_checks"] == 1 and stats["single_checks"] == N and stats["judged"] == 0


DEFECTS = {"malformed proof": ("json syntax", "invalid proof data"), "inputs of another length": ("signal count", None), "null entry": (None, "null argument")}


@pytest.mark.parametrize("is_ultra", [False, True], ids=["groth16", "ultragroth"])
@pytest.mark.parametrize("refused", [None, off_curve_key], ids=["good key", "key off its curve"])
def test_texts_that_do_not_parse(cases, refused, is_ultra):
    """(d): the message of a proof that fails before any pairing is the single call's own, under a key the batch refuses as well"""
    pairs, vk = cases[is_ultra]
    key = refused(vk) if refused else vk
    length = "len(inputs) != len(vk.IC)" if is_ultra else "len(inputs)+1 != len(vk.IC)"

    def texts(places):
        out = list(pairs)
        for at, name in places.items():
            kind = DEFECTS[name][0]
            out[at] = VB.bad_proof(kind, *pairs[at], ultra=is_ultra) if kind else (None, pairs[at][1])
        return [p for p, _ in out], [s for _, s in out]

    for at, name in ((4, "malformed proof"), (2, "inputs of another length"), (0, "null entry"), (5, "null entry")):
        proofs, pubs = texts({at: name})
        if name == "null entry" and at == 5:                                      # ... and a null inputs text
            proofs[5], pubs[5] = pairs[5][0], None
        singles = [single(is_ultra, p, s, key) for p, s in zip(proofs, pubs)]
        assert singles[at] == (ERROR, DEFECTS[name][1] or length)
        rc, msg, verdicts, stats = batch_json(is_ultra, proofs, pubs, key)
        assert (rc, msg, verdicts) == call_says(singles) and verdicts[at] == ERROR
        if not refused:
            assert msg == "proof %d: %s" % (at, singles[at][1]) and verdicts.count(VALID) == N - 1
            assert stats["single_checks"] == 0 and stats["batch_checks"] == 1     # answered without a pairing: the other five hold
        else:
            assert stats["single_checks"] == N and stats["batch_checks"] == 0
    proofs, pubs = texts({1: "malformed proof", 3: "inputs of another length", 5: "null entry"})
    singles = [single(is_ultra, p, s, key) for p, s in zip(proofs, pubs)]
    rc, msg, verdicts, stats = batch_json(is_ultra, proofs, pubs, key)
    assert (rc, msg, verdicts) == call_says(singles) and [verdicts[i] for i in (1, 3, 5)] == [ERROR] * 3
    if not refused:
        assert msg == "proof 1: invalid proof data" and verdicts == [VALID, ERROR, VALID, ERROR, VALID, ERROR]
