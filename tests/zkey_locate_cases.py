"""Shared case builders of the locate tests: the ratio test alone (test_points_ratio_host.py on host threads,
test_gpu_points_ratio.py on the device: ultragroth_amd.points_ratio_mask) and locating inside the key check
(test_zkey_locate_host.py, test_gpu_zkey_locate.py: ultragroth_amd.zkey_locate / ultra_zkey_locate).

Every expected answer is written down by construction, before any code under test runs. The ratio cases are X_i = k_i G,
Y_i = d k_i G, Q = d G2 for fixed d and k_i, with planted deviations whose places are the expected masks. A key case is ONE planted
change (or two) to a key of setup_from_ptau / ultra_setup_from_ptau / dev_setup, made on host threads, whose wrong records are known
from how it was planted. Builders are deterministic and cached; nobody changes what they return."""
import functools

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ultra_keys_cases as UC
import zkey_verify_cases as ZC
from ultragroth_amd import synth

R = SC.R
BLOCK = 256
D = 0x0123456789abcdef0fedcba9876543210123456789abcdef0fedcba987654321 % R          # the ratio of every honest pair
SHIFT = 0xD15C0                                                                        # the D of X_i + D, X_j - D
SIZES = (1, 255, 256, 257, 513)
INF = bytes(64)


def k_of(i):
    """the fixed logarithm of X_i: never 0 mod r"""
    return (0x9e3779b97f4a7c15f39cc0605cedc835 * (i + 1) + 0x1234567) % R


@functools.lru_cache(maxsize=None)
def honest(n, d=D):
    """(X, Y, Q): n records k_i G, n records d k_i G, and d G2"""
    import ultragroth_amd as ug
    x = ug.generator_mul([k_of(i) for i in range(n)], device=-1)
    y = ug.generator_mul([d * k_of(i) % R for i in range(n)], device=-1)
    q = ug.generator_mul([d], g2=True, device=-1)[0]
    return tuple(x), tuple(y), q


@functools.lru_cache(maxsize=None)
def point(k):
    import ultragroth_amd as ug
    return ug.generator_mul([k % R], device=-1)[0]


def blocks_of(n):
    return (n + BLOCK - 1) // BLOCK


def expected(n, wrong, max_blocks=64):
    """(record_mask, block_mask, report) of n pairs whose wrong records are `wrong`"""
    wrong = sorted(set(wrong))
    bad = sorted({i // BLOCK for i in wrong})
    resolved = bad[:max_blocks]
    rec = b"".join(bytes(1 if i in wrong else 0 for i in range(b * BLOCK, min(n, (b + 1) * BLOCK))) for b in resolved)
    blk = bytes(1 if b in bad else 0 for b in range(blocks_of(n)))
    seen = [i for i in wrong if i // BLOCK in resolved]
    return rec, blk, {"blocks": blocks_of(n), "bad_blocks": len(bad), "resolved_blocks": len(resolved), "exact": int(len(resolved) == len(bad)),
                      "bad_records": len(seen), "index": seen[:16]}


@functools.lru_cache(maxsize=None)
def ratio_cases():
    """{id: (X, Y, Q, max_blocks, expected wrong records)}"""
    out = {}

    def add(name, n, change=None, wrong=(), max_blocks=0, d=D):
        x, y, q = honest(n, d)
        x, y = list(x), list(y)
        if change:
            change(x, y)
        out[name] = (tuple(x), tuple(y), q, max_blocks, tuple(wrong))

    def replace_x(i):
        def f(x, y):
            x[i] = point(k_of(i) + 1)
        return f

    for n in SIZES:
        add("honest-%d" % n, n)
        add("wrong-first-%d" % n, n, replace_x(0), [0])
        add("wrong-last-%d" % n, n, replace_x(n - 1), [n - 1])          # 257, 513: n - 1 in a short last block
    add("wrong-last-lane-of-block-513", 513, replace_x(255), [255])
    add("wrong-first-lane-of-next-block-513", 513, replace_x(256), [256])
    add("wrong-y-257", 257, lambda x, y: y.__setitem__(100, point(5)), [100])

    def plus_minus(x, y):                        # X_i + D and X_j - D in one block: the plain sum of the block is unchanged
        x[3], x[200] = point(k_of(3) + SHIFT), point(k_of(200) - SHIFT)
    add("plus-minus-in-one-block-257", 257, plus_minus, [3, 200])

    def infinities(x, y):
        x[5], y[5] = INF, INF                    # holds
        x[6] = INF                               # X infinity, Y real: wrong
        y[300] = INF                             # the reverse: wrong
    add("infinities-513", 513, infinities, [6, 300])

    def cancelling(x, y):                        # every pair of block 1 is infinity: both sums of the block are infinity, and it holds
        for i in range(256, 512):
            x[i], y[i] = INF, INF
    add("block-of-infinities-513", 513, cancelling, [])
    add("q-is-g2-257", 257, replace_x(256), [256], d=1)

    def three_blocks(x, y):
        for i in (1, 2, 300, 512):
            x[i] = point(k_of(i) + 7)
    add("max-blocks-1-of-3-513", 513, three_blocks, [1, 2, 300, 512], max_blocks=1)
    add("three-blocks-513", 513, three_blocks, [1, 2, 300, 512])
    return out


RATIO_IDS = tuple("%s-%d" % (k, n) for n in SIZES for k in ("honest", "wrong-first", "wrong-last")) + (
    "wrong-last-lane-of-block-513", "wrong-first-lane-of-next-block-513", "wrong-y-257", "plus-minus-in-one-block-257", "infinities-513",
    "block-of-infinities-513", "q-is-g2-257", "max-blocks-1-of-3-513", "three-blocks-513")


def check_ratio(case_id, device):
    """runs one ratio case and holds it to its expected masks and report"""
    import ultragroth_amd as ug
    x, y, q, max_blocks, wrong = ratio_cases()[case_id]
    got = ug.points_ratio_mask(list(x), list(y), q, device=device, max_blocks=max_blocks)
    want = expected(len(x), wrong, max_blocks or 64)
    assert got[2] == want[2], case_id
    assert got[1] == want[1], case_id
    assert got[0] == want[0], case_id
    return got


# ------------------------------------------------------------------------------------------- keys
N_CHAIN = 590                                    # the squaring chain below: 593 wires, three blocks with the last one short


@functools.lru_cache(maxsize=None)
def chain():
    """(n_wires, n_public, rows, r1cs): x_(i+1) = x_i^2 + i + 1 over N_CHAIN constraints, one public output, and one private wire at the
    end that appears in NO constraint (its A, B1, B2 and C records are infinity in an honest key)"""
    n = N_CHAIN
    n_wires = n + 3                              # 0: one, 1: the output (= the last x), 2 .. n + 1: x_0 .. x_(n-1), n + 2: unused
    rows = []
    for i in range(n):
        src = 2 + i
        dst = 2 + i + 1 if i + 1 < n else 1
        rows.append(({src: 1}, {src: 1}, {dst: 1, 0: R - (i + 1)}))
    return n_wires, 1, tuple(rows), synth.r1cs_file(n_wires, 1, 0, rows)


CHAIN_POWER = 10                                 # 590 constraints + 2 public rows: domain 2^10
UNUSED_WIRE = N_CHAIN + 2


@functools.lru_cache(maxsize=None)
def chain_key(delta=ZC.FIXED_DELTA):
    import ultragroth_amd as ug
    return ug.setup_from_ptau(chain()[3], PC.ptau(CHAIN_POWER), delta=delta, device=-1)[0]


def with_records(key, sid, changes):
    """the key with records {index: bytes} of section sid replaced"""
    size = ZC.SECTION_RECORD.get(sid, 64)
    sec = bytearray(dict(RC.sections(key))[sid])
    for i, rec in changes.items():
        assert len(rec) == size
        sec[i * size:(i + 1) * size] = rec
    return PC.with_sections(key, {sid: bytes(sec)})


def record(key, sid, i):
    size = ZC.SECTION_RECORD.get(sid, 64)
    return dict(RC.sections(key))[sid][i * size:(i + 1) * size]


def entry(records, method, wrong, max_blocks=64, max_listed=16):
    """the located entry of a section of `records` records whose wrong records are `wrong` (all of them resolved unless max_blocks cuts)"""
    _, _, rep = expected(records, wrong, max_blocks)
    seen = [i for i in sorted(set(wrong)) if i // BLOCK in sorted({j // BLOCK for j in wrong})[:max_blocks]]
    return {"records": records, "method": method, "blocks": rep["blocks"], "bad_blocks": rep["bad_blocks"], "resolved_blocks": rep["resolved_blocks"],
            "exact": rep["exact"], "bad_records": rep["bad_records"], "index": seen[:max_listed]}


METHOD = {3: "ratio", 5: "bytes", 6: "bytes", 7: "bytes", 8: "ratio", 9: "ratio", 12: "ratio"}


@functools.lru_cache(maxsize=None)
def g2_point(k):
    import ultragroth_amd as ug
    return ug.generator_mul([k % R], g2=True, device=-1)[0]


@functools.lru_cache(maxsize=None)
def planted_cases():
    """{id: (r1cs, ptau, zkey, {section: wrong records}, kwargs of zkey_locate)} on the chain (593 wires: sections 5 - 7 have three
    blocks, section 8 has 591 records, H 1 024) and on zkey_verify_cases' odd12 circuit"""
    n_wires, n_public, _, r1cs = chain()
    ptau = PC.ptau(CHAIN_POWER)
    key = chain_key()
    pub = n_public + 1
    out = {}

    def add(name, zkey, wrong, r1cs=r1cs, ptau=ptau, **kw):
        out[name] = (r1cs, ptau, zkey, {s: tuple(w) for s, w in wrong.items()}, kw)

    some = point(0xC0FFEE)
    for sid in (5, 6, 8, 9):
        top = {5: n_wires, 6: n_wires, 8: n_wires - pub, 9: 1 << CHAIN_POWER}[sid]
        i, j = 255, 256                          # the last lane of a block and the first of the next
        add("replaced-%d" % sid, with_records(key, sid, {i: some}), {sid: [i]})
        a, b = record(key, sid, i), record(key, sid, j)
        assert a != b and any(a) and any(b)
        add("swapped-%d" % sid, with_records(key, sid, {i: b, j: a}), {sid: [i, j]})
        add("infinity-%d" % sid, with_records(key, sid, {top - 2: INF}), {sid: [top - 2]})      # in the short last block
    # a real point on the wire that appears in no constraint: the honest record is infinity
    for sid, at in ((5, UNUSED_WIRE), (6, UNUSED_WIRE), (8, UNUSED_WIRE - pub)):
        assert not any(record(key, sid, at))
        add("unused-wire-%d" % sid, with_records(key, sid, {at: some}), {sid: [at]})
    assert not any(record(key, 7, UNUSED_WIRE))
    add("unused-wire-7", with_records(key, 7, {UNUSED_WIRE: g2_point(77)}), {7: [UNUSED_WIRE]})
    add("replaced-7", with_records(key, 7, {256: g2_point(78)}), {7: [256]})
    a, b = record(key, 7, 255), record(key, 7, 256)
    add("swapped-7", with_records(key, 7, {255: b, 256: a}), {7: [255, 256]})
    add("infinity-7", with_records(key, 7, {n_wires - 2: bytes(128)}), {7: [n_wires - 2]})
    # section 3: two records only
    add("replaced-3", with_records(key, 3, {1: some}), {3: [1]})
    add("swapped-3", with_records(key, 3, {0: record(key, 3, 1), 1: record(key, 3, 0)}), {3: [0, 1]})
    add("infinity-3", with_records(key, 3, {0: INF}), {3: [0]})
    # H of another delta: every record is wrong
    other = chain_key(ZC.OTHER_DELTA)
    h_other = PC.with_sections(key, {9: dict(RC.sections(other))[9]})
    n_h = 1 << CHAIN_POWER
    add("h-of-another-delta", h_other, {9: range(n_h)})
    add("h-of-another-delta-max-blocks-2", h_other, {9: range(n_h)}, max_blocks=2)
    # two sections at once
    add("two-sections-5-and-8", with_records(with_records(key, 5, {17: some}), 8, {300: some, 590: some}), {5: [17], 8: [300, 590]})
    add("many-listed-8", with_records(key, 8, {i: some for i in range(100, 140)}), {8: range(100, 140)}, max_listed=40)
    # a changed C coefficient of the .r1cs: K of the wire it stands on changes. Constraint 3's C is {wire 6: 1, wire 0: r - 4}
    add("r1cs-c-coefficient-private", key, {8: [6 - pub]}, r1cs=ZC.c_coefficient_changed(r1cs, 3, 0))
    add("r1cs-c-coefficient-public", key, {3: [0]}, r1cs=ZC.c_coefficient_changed(r1cs, 3, 1))
    return out


PLANTED_IDS = tuple("%s-%d" % (k, s) for s in (5, 6, 8, 9) for k in ("replaced", "swapped", "infinity")) + (
    "unused-wire-5", "unused-wire-6", "unused-wire-8", "unused-wire-7", "replaced-7", "swapped-7", "infinity-7",
    "replaced-3", "swapped-3", "infinity-3", "h-of-another-delta", "h-of-another-delta-max-blocks-2", "two-sections-5-and-8",
    "many-listed-8", "r1cs-c-coefficient-private", "r1cs-c-coefficient-public")
# the subset the device repeats (the host twin runs them all): one per section and method, the caps, two sections, the .r1cs change
GPU_PLANTED_IDS = ("replaced-5", "swapped-6", "unused-wire-7", "infinity-3", "swapped-8", "unused-wire-8", "infinity-9", "h-of-another-delta",
                   "h-of-another-delta-max-blocks-2", "two-sections-5-and-8", "many-listed-8", "r1cs-c-coefficient-private")


def section_count(sid, n_wires, pub, n_h):
    return {3: pub, 5: n_wires, 6: n_wires, 7: n_wires, 8: n_wires - pub, 9: n_h}[sid]


def check_planted(case_id, device):
    """zkey_locate on one planted case: the exact located dict, and zkey_verify's own answer in front"""
    import ultragroth_amd as ug
    r1cs, ptau, zkey, wrong, kw = planted_cases()[case_id]
    n_wires, n_public = chain()[0], chain()[1]
    got = ug.zkey_locate(r1cs, ptau, zkey, device=device, **kw)
    verdict = ug.zkey_verify(r1cs, ptau, zkey, device=device)
    assert got is not None and got[:3] == verdict, case_id
    assert got[1] == sorted(wrong), case_id
    assert got[0] == min(wrong, key=(5, 6, 7, 3, 8, 9).index) and got[2] == ZC.section_message(got[0])
    located = {s: {k: v for k, v in e.items() if k != "kernel_ms"} for s, e in got[3].items()}
    want = {s: entry(section_count(s, n_wires, n_public + 1, 1 << CHAIN_POWER), METHOD[s], w, kw.get("max_blocks", 0) or 64, kw.get("max_listed", 16))
            for s, w in wrong.items()}
    assert located == want, case_id
    return got


# ------------------------------------------------------------------------------------------- UltraGroth keys
@functools.lru_cache(maxsize=None)
def chain_spec():
    """the chain's rounds: the output carries the challenge; the private wires with an odd number are round signals, listed from the
    top DOWN (so a list position is not a wire number in disguise), the others final signals, ascending"""
    n_wires = chain()[0]
    private = list(range(2, n_wires))
    return {"rand_indx": 1, "round_signals": [s for s in reversed(private) if s % 2], "final_signals": [s for s in private if not s % 2]}


@functools.lru_cache(maxsize=None)
def ultra_chain_key(d_round=UC.FIXED_DELTA, d_final=UC.OTHER_DELTA):
    import ultragroth_amd as ug
    return ug.ultra_setup_from_ptau(chain()[3], PC.ptau(CHAIN_POWER), chain_spec(), delta=(d_round, d_final), device=-1)[0]


def live(key, sid):
    """the places of a section's records that are not infinity"""
    return [i for i, r in enumerate(ZC.records(dict(RC.sections(key))[sid], 64)) if any(r)]


@functools.lru_cache(maxsize=None)
def ultra_cases():
    """{id: (r1cs, ptau, zkey, {section: wrong records}, kwargs)} on the chain under (FIXED_DELTA, OTHER_DELTA)"""
    r1cs, ptau, key = chain()[3], PC.ptau(CHAIN_POWER), ultra_chain_key()
    both_round = ultra_chain_key(UC.FIXED_DELTA, UC.FIXED_DELTA)         # its C2 and H stand under delta_round
    spec = chain_spec()
    out = {}
    at = 257
    assert spec["round_signals"][at] != at + 2 and any(record(key, 8, at))
    out["c1-record-replaced"] = (r1cs, ptau, with_records(key, 8, {at: point(0xC0FFEE)}), {8: (at,)}, {})
    # a record under the other delta is wrong wherever it is not infinity (the wire that is in no constraint stays infinity)
    out["c2-under-delta-round"] = (r1cs, ptau, PC.with_sections(key, {9: dict(RC.sections(both_round))[9]}), {9: tuple(live(key, 9))}, {})
    out["h-under-delta-round"] = (r1cs, ptau, PC.with_sections(key, {12: dict(RC.sections(both_round))[12]}), {12: tuple(live(key, 12))}, {})
    assert UNUSED_WIRE in spec["final_signals"] and len(live(key, 9)) == len(spec["final_signals"]) - 1 and len(live(key, 12)) == 1 << CHAIN_POWER
    return out


ULTRA_IDS = ("c1-record-replaced", "c2-under-delta-round", "h-under-delta-round")


def check_ultra(case_id, device):
    import ultragroth_amd as ug
    r1cs, ptau, zkey, wrong, kw = ultra_cases()[case_id]
    spec = chain_spec()
    got = ug.ultra_zkey_locate(r1cs, ptau, zkey, device=device, **kw)
    assert got is not None and got[:3] == ug.ultra_zkey_verify(r1cs, ptau, zkey, device=device), case_id
    (sid, places), = wrong.items()
    assert got[:3] == (sid, [sid], UC.section_message(sid))
    count = {8: len(spec["round_signals"]), 9: len(spec["final_signals"]), 12: 1 << CHAIN_POWER}[sid]
    located = {s: {k: v for k, v in e.items() if k != "kernel_ms"} for s, e in got[3].items()}
    assert located == {sid: entry(count, "ratio", places)}, case_id
    return got
