"""Shared case builders of the UltraGroth phase-2 setup tests (test_ultra_keys_host.py on host threads, test_gpu_ultra_keys.py on
the device): include/ultragroth_hip.h ug_ultra_setup_ptau_* / ug_points_scale_segments through ultragroth_amd.ultra_setup_from_ptau /
points_scale_segments. Every comparison is byte for byte. The references: for a key, dev_setup's host path for protocol 1337 and
the trapdoor (tau, alpha, beta, gamma = 1, delta_round, delta_final), which test_setup_host.py pins against the committed
fixture; for the segments, setup_ptau_cases.scale_reference (the CPU oracle's multiplication of Python-integer products), taken
per segment through the segment's index list. Every builder is deterministic and cached, so the two files share one copy."""
import functools
import random
import struct

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC

R = SC.R
FIXED_DELTA = PC.FIXED_DELTA
OTHER_DELTA = 0x1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f809 % R
DELTA_PAIRS = ((1, 1), (FIXED_DELTA, 1), (FIXED_DELTA, OTHER_DELTA))


def trapdoor(d_round, d_final):
    return dict(SC.trapdoor_dict(), gamma="1", delta_round=str(d_round), delta_final=str(d_final))


def _frozen(spec):
    return spec["rand_indx"], tuple(spec["round_signals"]), tuple(spec["final_signals"])


@functools.lru_cache(maxsize=None)
def _dev_key(r1cs, frozen, d_round, d_final, log_domain):
    import ultragroth_amd as ug
    spec = {"rand_indx": frozen[0], "round_signals": list(frozen[1]), "final_signals": list(frozen[2])}
    return ug.dev_setup(r1cs, trapdoor(d_round, d_final), "ultragroth", log_domain=log_domain, device=-1, ultra=spec)[:2]


def dev_key(r1cs, spec, d_round, d_final, log_domain=0):
    """(zkey, vkey) of dev_setup's host path for protocol 1337 and (tau, alpha, beta, gamma = 1, d_round, d_final)"""
    return _dev_key(r1cs, _frozen(spec), d_round, d_final, log_domain)


def delta_arg(d_round, d_final):
    return None if (d_round, d_final) == (1, 1) else (d_round, d_final)


# ------------------------------------------------------------------------------------------- circuits and specs
def fixture():
    """(r1cs, spec, power, log_domain) of the trapdoor fixture's circuit"""
    return RC.trapdoor()[2], SC.ultra_spec(), 11, 10


@functools.lru_cache(maxsize=None)
def _irregular():
    n_wires, _, r1cs = SC.odd_circuit(12, 1, 2)
    return n_wires, r1cs


def irregular(kind="alternating"):
    """SC.odd_circuit(12, 1, 2) (three public signals, domain 2^5) with a spec over its private wires 4 .. n_wires - 1:
    alternating (test_gpu_setup.py's lists), no-round / no-final (an empty list), descending (both lists from the top down)"""
    n_wires, r1cs = _irregular()
    private = list(range(4, n_wires))
    lists = {"alternating": (private[1::2], private[0::2]), "no-round": ([], private), "no-final": (private, []),
             "descending": (private[1::2][::-1], private[0::2][::-1])}[kind]
    return r1cs, {"rand_indx": 3, "round_signals": lists[0], "final_signals": lists[1]}


@functools.lru_cache(maxsize=None)
def _long_column():
    return SC.long_column_circuit(257)


def long_column():
    """SC.long_column_circuit(257): wire 0's column of C has 257 terms (the piece path of the combinations), one public input
    (wire 1, the rand signal here); every third private wire is a round signal"""
    n_wires, _, r1cs = _long_column()
    private = list(range(2, n_wires))
    return r1cs, {"rand_indx": 1, "round_signals": private[::3], "final_signals": [s for i, s in enumerate(private) if i % 3]}


# ------------------------------------------------------------------------------------------- points_scale_segments
N_SOURCE = 520                                   # the source records of every case: scale_points(520), infinity at 0, 63 and 519
SEGMENT_COUNTS = ((0, 5, 8), (5, 0, 8), (1, 1, 1), (127, 129, 128), (128, 128, 256), (300, 65, 512))
# (scalar of C1, of C2, of H) per case: different ones, equal ones, 0 and 1 among them; all of PC.scale_scalars(1000) occur
SEGMENT_SCALARS = ((PC.SEVENS, PC.NINES, 2), (R - 1, R - 1, R - 1), (0, 1, PC.NINES), (1, PC.SEVENS, 0), ((1 << 253) - 1, 2, 2),
                   (PC.NINES, PC.SEVENS, R - 1))
assert set(PC.scale_scalars(1000)) <= {s for t in SEGMENT_SCALARS for s in t}


@functools.lru_cache(maxsize=None)
def segment_case(which):
    """((scalar, index, count) x 3, source records). C1's list is a sparse random choice with repeats left out, C2's a permutation
    of a stretch, H's None (the first count records); each list names an infinity (record 0, 63 or 519) at its first and at its
    last place where it has two places."""
    counts, scalars = SEGMENT_COUNTS[which], SEGMENT_SCALARS[which]
    rng = random.Random(0x5E6 + which)
    _, pts = PC.scale_points(N_SOURCE)
    sparse = rng.sample(range(1, N_SOURCE - 1), counts[0])
    perm = list(range(200, 200 + counts[1]))
    rng.shuffle(perm)
    for lst in (sparse, perm):
        if len(lst) >= 2:
            lst[0], lst[-1] = 63, N_SOURCE - 1
        elif lst:
            lst[0] = 0
    return ((scalars[0], tuple(sparse), counts[0]), (scalars[1], tuple(perm), counts[1]), (scalars[2], None, counts[2])), pts


def segment_reference(which):
    segments, _ = segment_case(which)
    out = []
    for scalar, index, count in segments:
        ref = PC.scale_reference(N_SOURCE, scalar)
        out.append([ref[j] for j in (index if index is not None else range(count))])
    return out


# ------------------------------------------------------------------------------------------- r1cs_fold_classes
CLASS_MAPS = ("all-round", "all-final", "alternating", "random")


@functools.lru_cache(maxsize=None)
def class_map(n_wires, n_public, kind):
    """one class per wire: the public wires 0, the private ones by `kind`; alternating and random change class inside a row"""
    rng = random.Random(0xC1A5 + n_wires)
    private = {"all-round": lambda i: 1, "all-final": lambda i: 2, "alternating": lambda i: 1 + i % 2, "random": lambda i: rng.randrange(1, 3)}[kind]
    return tuple(0 if s <= n_public else private(s) for s in range(n_wires))


def fold_classes_reference(rows, n_public, rho, cls, log_n):
    """the eleven vectors by Python integers: 3 m + t is matrix t over class m; 9 is a, 10 is b"""
    n = 1 << log_n
    out = [[0] * n for _ in range(11)]
    for k, row in enumerate(rows):
        for t in range(3):
            for s, co in RC.terms_of(row[t]):
                v = 3 * cls[s] + t
                out[v][k] = (out[v][k] + co * rho[s]) % R
                if t < 2:
                    out[9 + t][k] = (out[9 + t][k] + co * rho[s]) % R
    for s in range(n_public + 1):
        out[0][len(rows) + s] = out[9][len(rows) + s] = rho[s] % R
    return tuple(out)


# ------------------------------------------------------------------------------------------- ultra_zkey_verify
SECTION_TEXT = "zkey: section %d: does not match the circuit and the powers of tau"
ULTRA_HEADER_POINTS = 4 + 32 + 4 + 32 + 12 + 12  # section 2 of a protocol-1337 key: ..., nVars, nPublic, domain, n1, n2, rand_indx; then the points
DELTA_C1 = ULTRA_HEADER_POINTS + 64 + 64 + 128 + 128
GAMMA2 = ULTRA_HEADER_POINTS + 64 + 64 + 128


def section_message(sid):
    return SECTION_TEXT % sid + {8: " under the key's round delta", 9: " under the key's final delta", 12: " under the key's final delta"}.get(sid, "")


@functools.lru_cache(maxsize=None)
def made_key(kind, d_round, d_final):
    """ultra_setup_from_ptau's key of irregular(kind) on PC.ptau(6), host threads"""
    import ultragroth_amd as ug
    r1cs, spec = irregular(kind)
    return ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta=delta_arg(d_round, d_final), device=-1)[0]


@functools.lru_cache(maxsize=None)
def fixture_key():
    import ultragroth_amd as ug
    r1cs, spec, power, log_domain = fixture()
    return ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta=(FIXED_DELTA, OTHER_DELTA), log_domain=log_domain, device=-1)[0]


# (id, r1cs, ptau, key, the spec the key was made with)
VALID_IDS = ("fixture", "golden-own-gamma", "alternating-ones", "alternating", "no-round", "no-final", "descending")


def valid_case(case_id):
    if case_id == "fixture":
        return fixture()[0], PC.ptau(11), fixture_key(), fixture()[1]
    if case_id == "golden-own-gamma":            # dev_setup's committed key: its gamma is the trapdoor's, not 1
        return fixture()[0], PC.ptau(11), RC.golden("ultra.zkey"), fixture()[1]
    if case_id == "alternating-ones":
        return irregular()[0], PC.ptau(6), made_key("alternating", 1, 1), irregular()[1]
    r1cs, spec = irregular(case_id)
    return r1cs, PC.ptau(6), made_key(case_id, FIXED_DELTA, OTHER_DELTA), spec


def _records(sec, size=64):
    return [sec[i:i + size] for i in range(0, len(sec), size)]


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """{id: (r1cs, ptau, zkey, spec or None, failing sections ascending, first failing section, message)}: ONE planted change each to the
    key of irregular("alternating") under (FIXED_DELTA, OTHER_DELTA), whose effect on every relation is known in advance"""
    import zkey_verify_cases as ZC
    r1cs, spec = irregular()
    ptau = PC.ptau(6)
    key = made_key("alternating", FIXED_DELTA, OTHER_DELTA)
    secs = dict(RC.sections(key))
    both_final = dict(RC.sections(made_key("alternating", OTHER_DELTA, OTHER_DELTA)))     # its C1 is K / delta_final
    both_round = dict(RC.sections(made_key("alternating", FIXED_DELTA, FIXED_DELTA)))     # its H is P / delta_round
    out = {}

    def add(name, failing, first, message, zkey=key, r1cs=r1cs, use_spec=None):
        out[name] = (r1cs, ptau, zkey, use_spec, list(failing), first, message)

    add("c1-records-swapped", [8], 8, section_message(8), PC.with_sections(key, {8: ZC.swapped(secs[8], 64)}))
    # the list's entries swapped under the same records: the fold's classes are unchanged, C1's weights are not
    rs = list(spec["round_signals"])
    c1 = _records(secs[8])
    i, j = [k for k in range(len(rs)) if any(c1[k])][:2]
    assert c1[i] != c1[j]
    rs[i], rs[j] = rs[j], rs[i]
    swapped10 = PC.with_sections(key, {10: struct.pack("<%dI" % len(rs), *rs)})
    add("section-10-entries-swapped", [8], 8, section_message(8), swapped10)
    add("section-10-entries-swapped-with-spec", [8, 10], 10, "zkey: section 10: does not match the spec", swapped10, use_spec=spec)
    # a live round signal and its record moved to the end of the final side, the counts adjusted: still a partition, and the
    # record is K / delta_round in a section that stands under delta_final
    k = [k for k in range(len(c1)) if any(c1[k])][-1]
    rs, fs = list(spec["round_signals"]), list(spec["final_signals"])
    moved = rs.pop(k)
    fs.append(moved)
    header = bytearray(secs[2])
    struct.pack_into("<II", header, ULTRA_HEADER_POINTS - 12, len(rs), len(fs))
    moved_key = PC.with_sections(key, {2: bytes(header), 8: b"".join(c1[:k] + c1[k + 1:]), 9: secs[9] + c1[k],
                                       10: struct.pack("<%dI" % len(rs), *rs), 11: struct.pack("<%dI" % len(fs), *fs)})
    add("signal-moved-to-the-final-round", [9], 9, section_message(9), moved_key)
    add("signal-moved-to-the-final-round-with-spec", [9, 10, 11], 10, "zkey: section 10: does not match the spec", moved_key, use_spec=spec)
    add("c1-under-delta-final", [8], 8, section_message(8), PC.with_sections(key, {8: both_final[8]}))
    add("h-under-delta-round", [12], 12, section_message(12), PC.with_sections(key, {12: both_round[12]}))
    header = secs[2][:DELTA_C1] + both_final[2][DELTA_C1:DELTA_C1 + 64] + secs[2][DELTA_C1 + 64:]
    add("delta-c1-pair-disagrees", [2], 2, "zkey: header: delta_c1's G1 and G2 points are not the same delta", PC.with_sections(key, {2: header}))
    # C is in no section of the key: only the K sum of the wire's class sees it
    rows = SC.odd_circuit(12, 1, 2)[1]
    wire = RC.terms_of(rows[3][2])[0][0]
    sid = 8 if wire in spec["round_signals"] else 9
    assert wire > 3
    add("r1cs-c-coefficient", [sid], sid, section_message(sid), r1cs=ZC.c_coefficient_changed(r1cs, 3, 0))
    other = irregular("descending")[1]
    add("spec-lists-differ", [10, 11], 10, "zkey: section 10: does not match the spec", use_spec=other)
    add("spec-rand-indx-differs", [2], 2, "zkey: header: rand_indx does not match the spec", use_spec=dict(spec, rand_indx=2))
    # ---- several planted changes in one key (COMPOUND_IDS): every failing section is reported, the first relation in the check's
    # order -- header, section 4, the spec (2, 10, 11), then 5, 6, 7, 3, 8, 9, 12 -- gives `first` and the message
    record = 17
    coefs = bytearray(secs[4])
    assert len(coefs) > 4 + 44 * (record + 1)
    coefs[4 + 44 * record + 12 + 5] ^= 0x10
    add("section-4-byte-c2-swapped-h-under-delta-round-other-spec", [4, 9, 10, 11, 12], 4, "zkey: section 4 record %d: does not match the circuit" % record,
        PC.with_sections(key, {4: bytes(coefs), 9: ZC.swapped(secs[9], 64), 12: both_round[12]}), use_spec=other)
    add("c1-under-delta-final-h-under-delta-round", [8, 12], 8, section_message(8), PC.with_sections(key, {8: both_final[8], 12: both_round[12]}))
    # ---- the header's rules in their order (HEADER_ORDER_IDS): gamma2 is tried before the deltas. The point check lets an all-zero
    # record (infinity) through; gamma2 at infinity also fails section 3, delta_c1's G1 point is in no relation but the header's own
    header = bytearray(secs[2])
    header[GAMMA2:GAMMA2 + 128] = bytes(128)
    header[DELTA_C1:DELTA_C1 + 64] = bytes(64)
    add("gamma2-and-delta-c1-at-infinity", [2, 3], 2, "zkey: header: gamma2 is the point at infinity", PC.with_sections(key, {2: bytes(header)}))
    return out


INVALID_IDS = ("c1-records-swapped", "section-10-entries-swapped", "section-10-entries-swapped-with-spec", "signal-moved-to-the-final-round",
               "signal-moved-to-the-final-round-with-spec", "c1-under-delta-final", "h-under-delta-round", "delta-c1-pair-disagrees",
               "r1cs-c-coefficient", "spec-lists-differ", "spec-rand-indx-differs")
COMPOUND_IDS = ("section-4-byte-c2-swapped-h-under-delta-round-other-spec", "c1-under-delta-final-h-under-delta-round")
HEADER_ORDER_IDS = ("gamma2-and-delta-c1-at-infinity",)


@functools.lru_cache(maxsize=None)
def refusals():
    """{id: (r1cs, ptau, zkey, validate, the message's text)}"""
    import zkey_verify_cases as ZC
    r1cs, spec = irregular()
    ptau = PC.ptau(6)
    key = made_key("alternating", FIXED_DELTA, OTHER_DELTA)
    secs = dict(RC.sections(key))
    rs, fs = spec["round_signals"], spec["final_signals"]
    repeated = struct.pack("<%dI" % len(rs), *([fs[0]] + list(rs[1:])))
    c1 = _records(secs[8])
    at = [k for k in range(len(c1)) if any(c1[k])][1]
    bent = bytearray(secs[8]); bent[64 * at + 3] ^= 1
    b2 = _records(secs[7], 128)
    g2_at = [k for k, r in enumerate(b2) if any(r)][2]
    b2[g2_at] = ZC.off_subgroup_record()
    header = bytearray(secs[2])
    struct.pack_into("<I", header, ULTRA_HEADER_POINTS - 4, 4)
    return {
        "groth16-key": (r1cs, ptau, ZC.ptau_key("odd12", 6, FIXED_DELTA), 2, "zkey: zkey file is not ultragroth"),
        "lists-do-not-partition": (r1cs, ptau, PC.with_sections(key, {10: repeated}), 2,
                                   "zkey: the round and final signal lists do not partition the private signals: signal %d" % fs[0]),
        "rand-indx-not-public": (r1cs, ptau, PC.with_sections(key, {2: bytes(header)}), 2, "zkey: rand_indx 4 is not a public signal"),
        "off-curve-c1": (r1cs, ptau, PC.with_sections(key, {8: bytes(bent)}), 2, "zkey: section 8 point %d: not on the curve" % at),
        "b2-off-subgroup": (r1cs, ptau, PC.with_sections(key, {7: b"".join(b2)}), 2, "zkey: section 7 point %d: not in the subgroup of order r" % g2_at),
        "unprepared-ptau": (r1cs, PC.ptau(6, prepared=False), key, 2, "ptau: not prepared for phase 2"),
    }


REFUSAL_IDS = ("groth16-key", "lists-do-not-partition", "rand-indx-not-public", "off-curve-c1", "b2-off-subgroup", "unprepared-ptau")
