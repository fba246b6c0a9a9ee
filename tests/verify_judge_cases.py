"""Shared by tests/test_verify_judge_host.py and tests/test_gpu_verify_judge.py: the raw call of the batch verifier with options
(ug_*_verify_batch_opt), Fq12 values as the library's limbs, and the four values the final exponentiation is tested on. As in
verify_batch_cases.py every expected verdict is the SINGLE verifier's on the same strings; oracle/pairing.py is the second yardstick
for the final exponentiation."""
import ctypes as C
import json

from oracle import pairing as PR
import verify_batch_cases as VB

Q = PR.P
LIMBS, LIMB_BITS = 9, 29
STAT_FIELDS = ("batch_checks", "single_checks", "off_subgroup", "device_ms", "host_ms")
JUDGE_FIELDS = ("judged", "judge_launches", "judge_ms")


def batch_opt(ultra, proofs, pubs, vk, device=-1, judge=1, search_width=-1, judge_min=-1):
    """raw call: (rc, message, verdicts, stats dict with the judge's fields)"""
    from ultragroth_amd._lib import VerifyBatchOptions, VerifyBatchStatsEx
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_opt if ultra else L.ug_groth16_verify_batch_opt
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in pubs])
    verdicts = (C.c_int * max(n, 1))(*([VB.SENTINEL] * max(n, 1)))
    opt = VerifyBatchOptions(C.sizeof(VerifyBatchOptions), judge, search_width, judge_min)
    stats, err = VerifyBatchStatsEx(), C.create_string_buffer(512)
    rc = fn(device, n, pa, ia, VB._enc(vk), verdicts, C.byref(opt), C.byref(stats), err, 511)
    out = {f: getattr(stats.base, f) for f in STAT_FIELDS}
    out.update({f: getattr(stats, f) for f in JUDGE_FIELDS})
    return rc, err.value.decode(), list(verdicts[:n]), out


def singles(ultra, proofs, pubs, vk):
    return [VB.single(ultra, p, s, vk) for p, s in zip(proofs, pubs)]


# ---- Fq12 values: 12 coefficients in w, each 9 limbs of 29 bits of x * 2^261 mod q (canonical device Montgomery form) ------------
def f12_limbs(coeffs):
    out = []
    for x in coeffs:
        v = x % Q * (1 << (LIMBS * LIMB_BITS)) % Q
        out += [(v >> (LIMB_BITS * i)) & ((1 << LIMB_BITS) - 1) for i in range(LIMBS)]
    return out


def _g1(j):
    return int(j[0]), int(j[1])


def _g2(j):
    return (int(j[0][0]), int(j[0][1])), (int(j[1][0]), int(j[1][1]))


def final_exp_values(proof, pub, vk):
    """[(name, Fq12 coefficients, is f^((p^12-1)/r) one by oracle.pairing.final_exp)] for: the Miller product of a valid Groth16
    proof's four pairs, the same with the public signal of the vkX pair moved by one, f = 1 and f = 0"""
    proof, pub = json.loads(proof), json.loads(pub)
    ic = [_g1(x) for x in vk["IC"]]

    def product(signals):
        vkx = ic[0]
        for v, pt in zip(signals, ic[1:]):
            vkx = PR.g1_add(vkx, PR.g1_mul(pt, int(v) % PR.R))
        f = PR.miller(_g2(proof["pi_b"]), _g1(proof["pi_a"]))
        f = PR.f12_mul(f, PR.miller(_g2(vk["vk_beta_2"]), PR.g1_neg(_g1(vk["vk_alpha_1"]))))
        f = PR.f12_mul(f, PR.miller(_g2(vk["vk_gamma_2"]), PR.g1_neg(vkx)))
        return PR.f12_mul(f, PR.miller(_g2(vk["vk_delta_2"]), PR.g1_neg(_g1(proof["pi_c"]))))

    values = [("valid proof", product(pub)), ("tampered pair", product([str(int(pub[0]) + 1)] + pub[1:])),
              ("one", list(PR.F12_ONE)), ("zero", [0] * 12)]
    return [(name, f, PR.final_exp(f) == PR.F12_ONE) for name, f in values]
