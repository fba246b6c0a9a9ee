"""Shared case builders of the key-check tests (test_zkey_verify_host.py on host threads, test_gpu_zkey_verify.py on the device):
include/ultragroth_hip.h ug_zkey_verify_run / ug_r1cs_fold through ultragroth_amd.zkey_verify / r1cs_fold.

The references: for the fold, Python integers over the case builders' rows; for a verdict, how the key was made -- a key of
setup_from_ptau (pinned byte for byte against dev_setup by test_setup_ptau_host.py) or dev_setup's own is valid, and every
invalid key is ONE planted change to such a key whose effect on each relation is known in advance, so the exact set of failing
sections and the message are asserted (COMPOUND_IDS and HEADER_ORDER_IDS plant several such changes in one key: the sections add
up, the first relation in the check's order gives the message). Every builder is deterministic (but for the drawn delta, which nobody reads) and cached:
the two files share one copy, which nobody changes. Every key and every .ptau is made on host threads."""
import functools
import random
import struct

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
from oracle import pairing as PR
from ultragroth_amd import synth

R = SC.R
Q = PR.P
MONT = 1 << 256
FIXED_DELTA = PC.FIXED_DELTA
OTHER_DELTA = 0x1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f809 % R
SECTION_TEXT = "zkey: section %d: does not match the circuit and the powers of tau"


def section_message(sid):
    return SECTION_TEXT % sid + (" under the key's delta" if sid in (8, 9) else "")


# ------------------------------------------------------------------------------------------- the fold
@functools.lru_cache(maxsize=None)
def fold_case(name):
    """(n_wires, n_public, rows, .r1cs bytes) of a fold case: irregular-<m> has no public wire but wire 0; odd-<out>-<in> is
    setup_cases.odd_circuit(12, out, in)"""
    kind, *args = name.split("-")
    if kind == "irregular":
        n_wires, rows, _, _, _ = RC.irregular(int(args[0]))
        return n_wires, 0, tuple(rows), synth.r1cs_file(n_wires, 0, 0, rows)
    n_wires, rows, r1cs = SC.odd_circuit(12, int(args[0]), int(args[1]))
    return n_wires, int(args[0]) + int(args[1]), rows, r1cs


FOLD_CASES = ("irregular-1", "irregular-255", "irregular-256", "irregular-257", "odd-0-0", "odd-1-2")


@functools.lru_cache(maxsize=None)
def fold_rho(n_wires):
    """one rho for every case of that many wires: weights below 2^128 with 0, 1, 2^128 - 1 and values >= r among them -- on the
    constant wire (so that a public row has to reduce it), on wires of both sides and on the last wire"""
    rng = random.Random(0xF01D + n_wires)
    rho = [rng.randrange(1 << 128) for _ in range(n_wires)]
    rho[0] = R + 7
    for wire, value in ((1, 0), (2, 1), (3, (1 << 128) - 1), (4, R + 5), (5, (1 << 256) - 1), (n_wires - 1, 2 * R + 1)):
        if wire < n_wires:
            rho[wire] = value
    return tuple(rho)


def log_domain_of(n_constraints, n_public):
    return max(1, (n_constraints + n_public).bit_length())       # the smallest 2^n >= n_constraints + n_public + 1


def fold_reference(rows, n_public, rho, log_n):
    """(a_pub, b_pub, c_pub, a_priv, b_priv, c_priv) by Python integers"""
    n = 1 << log_n
    out = [[0] * n for _ in range(6)]
    for k, row in enumerate(rows):
        for t in range(3):
            for s, co in RC.terms_of(row[t]):
                v = t if s <= n_public else 3 + t
                out[v][k] = (out[v][k] + co * rho[s]) % R
    for s in range(n_public + 1):
        out[0][len(rows) + s] = rho[s] % R
    return tuple(out)


# ------------------------------------------------------------------------------------------- circuits, files, keys
@functools.lru_cache(maxsize=None)
def circuit(name):
    """.r1cs bytes and the log_domain its keys are made with (0: the smallest)"""
    if name == "fixture":
        return RC.trapdoor()[2], 10
    if name == "odd300":
        return SC.odd_circuit(300, 2, 0)[2], 0
    if name == "odd12":
        return SC.odd_circuit(12, 1, 2)[2], 0
    if name == "long257":
        return SC.long_column_circuit(257)[2], 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ptau_shifted(power):
    """the .ptau of (tau + 1, alpha, beta)"""
    t = SC.trapdoor_dict()
    return synth.ptau_file(power, (int(t["tau"]) + 1) % R, int(t["alpha"]), int(t["beta"]), device=-1)


@functools.lru_cache(maxsize=None)
def ptau_key(name, power, delta):
    """setup_from_ptau's key of the circuit; delta: None (delta = 1), an integer or "draw" """
    import ultragroth_amd as ug
    r1cs, log_domain = circuit(name)
    return ug.setup_from_ptau(r1cs, PC.ptau(power), delta=delta, log_domain=log_domain, device=-1)[0]


# (id, circuit, power of the .ptau, the key)
VALID = (
    ("fixture-delta-1", "fixture", 11, lambda: ptau_key("fixture", 11, None)),
    ("fixture-fixed-delta", "fixture", 11, lambda: ptau_key("fixture", 11, FIXED_DELTA)),
    ("fixture-drawn-delta", "fixture", 11, lambda: ptau_key("fixture", 11, "draw")),
    ("odd300", "odd300", 10, lambda: ptau_key("odd300", 10, FIXED_DELTA)),
    ("odd12-power-6", "odd12", 6, lambda: ptau_key("odd12", 6, FIXED_DELTA)),
    ("odd12-power-5-padded-level", "odd12", 5, lambda: ptau_key("odd12", 5, FIXED_DELTA)),
    ("long-column-257", "long257", 10, lambda: ptau_key("long257", 10, FIXED_DELTA)),
    # dev_setup's key of the fixture trapdoor, with its own gamma != 1, against the .ptau synthesized for the same tau, alpha, beta
    ("dev-setup-own-gamma", "fixture", 11, lambda: RC.golden("groth16.zkey")),
)


def valid_case(case_id):
    """(r1cs, ptau, zkey)"""
    for cid, name, power, key in VALID:
        if cid == case_id:
            return circuit(name)[0], PC.ptau(power), key()
    raise KeyError(case_id)


# ------------------------------------------------------------------------------------------- planted changes
HEADER_POINTS = 4 + 32 + 4 + 32 + 12             # section 2: n8q, q, n8r, r, nVars, nPublic, domain; then the points
ALPHA1, BETA1, DELTA1 = HEADER_POINTS, HEADER_POINTS + 64, HEADER_POINTS + 64 + 64 + 128 + 128
GAMMA2 = HEADER_POINTS + 64 + 64 + 128
SECTION_RECORD = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}


def records(sec, size):
    return [sec[i:i + size] for i in range(0, len(sec), size)]


def swapped(sec, size):
    """the section with its first two unequal records, neither of them infinity, swapped"""
    recs = records(sec, size)
    live = [i for i, r in enumerate(recs) if any(r)]
    i = live[0]
    j = next(j for j in live[1:] if recs[j] != recs[i])
    recs[i], recs[j] = recs[j], recs[i]
    return b"".join(recs)


def c_coefficient_changed(r1cs, constraint, term):
    """the .r1cs with coefficient `term` of constraint `constraint`'s C combination increased by one, patched in section 2"""
    secs = RC.sections(r1cs)
    body = bytearray(dict(secs)[2])
    pos = 0
    for k in range(constraint + 1):
        for t in range(3):
            n = struct.unpack_from("<I", body, pos)[0]
            if k == constraint and t == 2:
                at = pos + 4 + 36 * term + 4
                assert term < n
                value = (int.from_bytes(body[at:at + 32], "little") + 1) % R
                body[at:at + 32] = value.to_bytes(32, "little")
            pos += 4 + 36 * n
    return RC.binfile(b"r1cs", 1, [(i, bytes(body) if i == 2 else p) for i, p in secs])


def f2_sqrt(a):
    """square root in Fq2 = Fq[u]/(u^2 + 1), q = 3 mod 4 (complex method)"""
    a1 = PR.f2_pow(a, (Q - 3) // 4)
    x0 = PR.f2_mul(a1, a)
    alpha = PR.f2_mul(a1, x0)
    x = PR.f2_mul((0, 1), x0) if alpha == (Q - 1, 0) else PR.f2_mul(PR.f2_pow(PR.f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    assert PR.f2_mul(x, x) == a
    return x


@functools.lru_cache(maxsize=None)
def off_subgroup_record():
    """a G2 record on the twist and outside the subgroup of order r: x = 1, as test_gpu_validate.py makes one"""
    x = (1, 0)
    y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), PR.f2_muls(PR.f2_inv(PR.XI), 3)))
    assert PR.g2_on_curve((x, y))
    return b"".join((c * MONT % Q).to_bytes(32, "little") for c in (x[0], x[1], y[0], y[1]))


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """{id: (r1cs, ptau, zkey, failing sections in ascending order, first failing section, message)}; all on odd_circuit(12, 1, 2)
    (four public wires, domain 2^5) with PC.ptau(6) unless the case says otherwise"""
    import ultragroth_amd as ug
    r1cs = circuit("odd12")[0]
    ptau = PC.ptau(6)
    key = ptau_key("odd12", 6, FIXED_DELTA)
    other = ptau_key("odd12", 6, OTHER_DELTA)
    secs, other_secs = dict(RC.sections(key)), dict(RC.sections(other))
    out = {}

    def add(name, failing, first, message, zkey=key, r1cs=r1cs, ptau=ptau):
        out[name] = (r1cs, ptau, zkey, list(failing), first, message)

    for sid in (5, 6, 7, 3, 8, 9):               # section 6 with section 7 left alone and the reverse are among these
        add("swap-%d" % sid, [sid], sid, section_message(sid), PC.with_sections(key, {sid: swapped(secs[sid], SECTION_RECORD[sid])}))
    # A_s + D and A_s' - D: the plain sum of the section is unchanged, so equal or absent weights would not see it
    recs = records(secs[5], 64)
    s, s2 = [i for i, r in enumerate(recs) if any(r)][1:3]
    d = ug.generator_mul([0xD15C0], device=-1)[0]
    recs[s], recs[s2] = ug.points_combine([0, 2, 4], [0, 2, 1, 2], [1, 1, 1, R - 1], [recs[s], recs[s2], d], device=-1)
    assert b"".join(recs) != secs[5]
    add("plus-minus-5", [5], 5, section_message(5), PC.with_sections(key, {5: b"".join(recs)}))
    for sid in (8, 9):
        add("other-delta-%d" % sid, [sid], sid, section_message(sid), PC.with_sections(key, {sid: other_secs[sid]}))
    header = secs[2][:DELTA1] + other_secs[2][DELTA1:DELTA1 + 64] + secs[2][DELTA1 + 64:]
    add("delta1-of-another-key", [2], 2, "zkey: header: delta1 and delta2 are not the same delta", PC.with_sections(key, {2: header}))
    header = secs[2][:ALPHA1] + secs[2][BETA1:BETA1 + 64] + secs[2][ALPHA1 + 64:]
    add("alpha1-is-beta1", [2], 2, "zkey: header: alpha1 is not the powers of tau's", PC.with_sections(key, {2: header}))
    record = 17
    coefs = bytearray(secs[4])
    coefs[4 + 44 * record + 12 + 5] ^= 0x10
    add("section-4-byte", [4], 4, "zkey: section 4 record %d: does not match the circuit" % record, PC.with_sections(key, {4: bytes(coefs)}))
    # dev_setup's H is L_k(tau / g) ...: not the padded level's, which is all a .ptau of the domain's own power has
    add("dev-setup-against-power-5", [9], 9, section_message(9), PC.dev_setup_key(r1cs, FIXED_DELTA, 0)[0], ptau=PC.ptau(5))
    add("ptau-of-tau-plus-1", [3, 5, 6, 7, 8, 9], 5, section_message(5), ptau=ptau_shifted(6))
    # C is in no section of the key: only the K sums see it. Constraint 3's C names a private wire; the last constraint's C is
    # [(0, 5), (0, r - 5)] on the constant wire, which is public
    n_rows = len(SC.odd_circuit(12, 1, 2)[1])
    add("r1cs-c-coefficient-private", [8], 8, section_message(8), r1cs=c_coefficient_changed(r1cs, 3, 0))
    add("r1cs-c-coefficient-public", [3], 3, section_message(3), r1cs=c_coefficient_changed(r1cs, n_rows - 1, 0))
    # ---- several planted changes in one key (COMPOUND_IDS): every failing section is reported, the first relation in the check's
    # order -- header, section 4, then 5, 6, 7, 3, 8, 9 -- gives `first` and the message
    swap3, swap5 = swapped(secs[3], 64), swapped(secs[5], 64)
    add("section-4-byte-swap-3-other-delta-9", [3, 4, 9], 4, "zkey: section 4 record %d: does not match the circuit" % record,
        PC.with_sections(key, {4: bytes(coefs), 3: swap3, 9: other_secs[9]}))
    add("swap-3-and-5", [3, 5], 5, section_message(5), PC.with_sections(key, {3: swap3, 5: swap5}))
    # ---- the header's rules in their order (HEADER_ORDER_IDS). The point check lets an all-zero record (infinity) through. gamma2 at
    # infinity also fails section 3, whose relation stands under gamma2; delta1 is in no relation but the header's own
    zero = lambda sec, at, size: sec[:at] + bytes(size) + sec[at + size:]
    add("gamma2-and-delta1-at-infinity", [2, 3], 2, "zkey: header: delta1 is the point at infinity",
        PC.with_sections(key, {2: zero(zero(secs[2], GAMMA2, 128), DELTA1, 64)}))
    header = secs[2][:ALPHA1] + secs[2][BETA1:BETA1 + 64] + secs[2][ALPHA1 + 64:DELTA1] + other_secs[2][DELTA1:DELTA1 + 64] + secs[2][DELTA1 + 64:]
    add("alpha1-is-beta1-and-delta1-of-another-key", [2], 2, "zkey: header: alpha1 is not the powers of tau's", PC.with_sections(key, {2: header}))
    return out


INVALID_IDS = tuple("swap-%d" % s for s in (5, 6, 7, 3, 8, 9)) + (
    "plus-minus-5", "other-delta-8", "other-delta-9", "delta1-of-another-key", "alpha1-is-beta1", "section-4-byte",
    "dev-setup-against-power-5", "ptau-of-tau-plus-1", "r1cs-c-coefficient-private", "r1cs-c-coefficient-public")
COMPOUND_IDS = ("section-4-byte-swap-3-other-delta-9", "swap-3-and-5")
HEADER_ORDER_IDS = ("gamma2-and-delta1-at-infinity", "alpha1-is-beta1-and-delta1-of-another-key")


@functools.lru_cache(maxsize=None)
def all_public_case():
    """(r1cs, ptau, zkey): a circuit whose every wire is public (nVars = nPublic + 1), so the key's section 8 is empty; its key is
    setup_from_ptau's and valid"""
    import ultragroth_amd as ug
    rows = [({1: 1}, {2: 1}, {3: 1}), ({3: 1, 0: R - 1}, {1: 1}, {2: 5, 0: 7})]
    r1cs = synth.r1cs_file(4, 1, 2, rows)
    ptau = PC.ptau(6)
    zkey = ug.setup_from_ptau(r1cs, ptau, delta=FIXED_DELTA, device=-1)[0]
    assert SC.zkey_header(zkey)[:2] == (4, 3) and dict(RC.sections(zkey))[8] == b""
    return r1cs, ptau, zkey


@functools.lru_cache(maxsize=None)
def refusals():
    """{id: (r1cs, ptau, zkey, the message's text)}"""
    r1cs = circuit("odd12")[0]
    ptau = PC.ptau(6)
    key = ptau_key("odd12", 6, FIXED_DELTA)
    secs = dict(RC.sections(key))
    b2 = records(secs[7], 128)
    at = [i for i, r in enumerate(b2) if any(r)][2]
    b2[at] = off_subgroup_record()
    return {
        "b2-off-subgroup": (r1cs, ptau, PC.with_sections(key, {7: b"".join(b2)}), "zkey: section 7 point %d: not in the subgroup of order r" % at),
        "key-of-another-circuit": (r1cs, ptau, ptau_key("odd300", 10, FIXED_DELTA), "zkey: header: nVars "),
        "unprepared-ptau": (r1cs, PC.ptau(6, prepared=False), key, "ptau: not prepared for phase 2"),
        "ptau-power-below-domain": (r1cs, PC.ptau(4), key, "ptau: power 4 is below the circuit's 5"),
        "protocol-1337": (RC.trapdoor()[2], PC.ptau(11), RC.golden("ultra.zkey"), "zkey: protocol 1337 keys are not checked"),
        "truncated-section-8": (r1cs, ptau, PC.with_sections(key, {8: secs[8][:-1]}), "zkey: Section 8 is shorter than the header implies"),
    }


REFUSAL_IDS = ("b2-off-subgroup", "key-of-another-circuit", "unprepared-ptau", "ptau-power-below-domain", "protocol-1337", "truncated-section-8")
