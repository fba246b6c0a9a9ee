"""The EVM and COMPRESSED record layouts (include/verifier.h) with device = -1: ug_proof_record_convert / ug_inputs_convert against the
layouts restated in Python (verify_formats_cases), the host's f2_sqrt, and ug_*_verify_batch_records_fmt. No GPU. Proofs are the
oracle's, of the trapdoor fixtures; every expected verdict is the single verifier's on the text of the PLAIN record a record stands
for."""
import ctypes as C
import json
import os
import re

import pytest

import oracle as O
import verify_batch_cases as VB
import verify_records_cases as VR
import verify_formats_cases as VF
from verify_batch_cases import VALID, INVALID, ERROR
from verify_formats_cases import PLAIN, EVM, COMPRESSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {EVM: "evm", COMPRESSED: "compressed"}


@pytest.fixture(scope="module")
def g16():
    zkey, wtns, vk = VB.load("groth16.zkey"), VB.load("groth16.wtns"), json.loads(VB.load("groth16_vkey.json", "r"))
    pairs = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(33)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    recs, blocks = [VR.pack(p) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert VR.expected(False, recs, blocks, vk) == [VALID] * 33
    return proofs, pubs, recs, blocks, vk


@pytest.fixture(scope="module")
def ultra():
    zkey, uwtns, vk = VB.load("ultra.zkey"), VB.load("ultra.uwtns"), json.loads(VB.load("ultra_vkey.json", "r"))
    pairs = [O.ultra_groth_prove(zkey, uwtns, 10 + i, 200 + i, 3000 + i)[:2] for i in range(33)]
    proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
    recs, blocks = [VR.pack(p, True) for p in proofs], [VR.pack_inputs(s) for s in pubs]
    assert VR.expected(True, recs, blocks, vk) == [VALID] * 33
    return proofs, pubs, recs, blocks, vk


def _conversion_cases(recs, is_ultra):
    """PLAIN records whose points are all on their curves: the fixtures, the other sign of pi_a, a coordinate + q, infinity in each
    position"""
    cases = list(recs[:4])
    cases += [VR._put(r, 32, VF.Q - VR._get(r, 32)) for r in recs[:4]]                # A.y negated: both signs of one x
    cases.append(VR._put(recs[4], 0, VR._get(recs[4], 0) + VF.Q))
    cases.append(VR._put(recs[4], 160, VR._get(recs[4], 160) + VF.Q))
    cases.append(VR._put(VR._put(recs[5], 192, VF.Q), 224, VF.Q))                     # (q, q) reduces to infinity
    for lo, hi in [(0, 64), (64, 192), (192, 256)] + ([(256, 320)] if is_ultra else []):
        cases.append(recs[6][:lo] + bytes(hi - lo) + recs[6][hi:])
    cases.append(bytes(len(recs[0])))
    return cases


@pytest.mark.parametrize("is_ultra", [False, True])
def test_conversions_equal_the_reference(g16, ultra, is_ultra):
    recs, blocks = (ultra if is_ultra else g16)[2:4]
    signs = set()
    for rec in _conversion_cases(recs, is_ultra):
        want = {PLAIN: VF.reduced(rec), EVM: VF.to_evm(rec), COMPRESSED: VF.to_compressed(rec)}
        assert want[COMPRESSED] is not None and len(want[COMPRESSED]) == VF.size(is_ultra, COMPRESSED)
        signs.add(want[COMPRESSED][31] & 0xc0)
        for fmt in (PLAIN, EVM, COMPRESSED):
            assert VF.convert(is_ultra, PLAIN, rec, fmt) == (0, want[fmt]), fmt
            for back in (PLAIN, EVM, COMPRESSED):                                 # every pair of layouts, and the round trips of them
                assert VF.convert(is_ultra, fmt, want[fmt], back) == (0, want[back]), (fmt, back)
        assert VF.to_plain(EVM, want[EVM], blocks[0])[0] == want[PLAIN]
        assert VF.to_plain(COMPRESSED, want[COMPRESSED], blocks[0], is_ultra)[0] == want[PLAIN]
    assert signs == {0, 0x40, 0x80}                                               # both signs of pi_a and its infinity were met
    raw = VF._raw_evm(VR._put(recs[4], 0, VR._get(recs[4], 0) + VF.Q))            # an EVM record with an unreduced coordinate
    assert VF.convert(is_ultra, EVM, raw, PLAIN) == (0, VF.reduced(recs[4]))


def test_inputs_convert(g16):
    blocks = g16[3]
    block = VR._put(blocks[0], 0, VR._get(blocks[0], 0) + VF.PR.R)                # values are not reduced on the way
    for a in (PLAIN, EVM, COMPRESSED):
        for b in (PLAIN, EVM, COMPRESSED):
            want = VF.evm_inputs(block) if (a == EVM) != (b == EVM) else block
            assert VF.convert_inputs(a, block, b) == (0, want)
    L = VB.lib()
    out = C.create_string_buffer(32)
    assert L.ug_inputs_convert(7, block, 1, PLAIN, out) == 2 and L.ug_inputs_convert(PLAIN, block, 1, -1, out) == 2
    assert L.ug_inputs_convert(PLAIN, None, 1, EVM, out) == 2 and L.ug_inputs_convert(PLAIN, block, 1, EVM, None) == 2
    assert L.ug_inputs_convert(PLAIN, block, 0, EVM, out) == 2


@pytest.mark.parametrize("is_ultra", [False, True])
def test_return_codes(g16, ultra, is_ultra):
    proofs, pubs, recs, blocks, vk = ultra if is_ultra else g16
    untouched = lambda fmt: b"\x55" * VF.size(is_ultra, fmt)
    off, _ = VR.bad_record("C off curve", proofs[0], pubs[0], is_ultra)
    assert VF.to_compressed(off) is None
    assert VF.convert(is_ultra, PLAIN, off, COMPRESSED) == (1, untouched(COMPRESSED))
    assert VF.convert(is_ultra, EVM, VF.to_evm(off), COMPRESSED) == (1, untouched(COMPRESSED))
    assert VF.convert(is_ultra, PLAIN, off, EVM) == (0, VF.to_evm(off))           # PLAIN <-> EVM never fails
    off_b = VR._put(recs[0], 96, VR._get(recs[0], 96) ^ 1)                        # pi_b off the twist
    assert VF.convert(is_ultra, PLAIN, off_b, COMPRESSED)[0] == 1
    comp = VF.to_compressed(recs[1])
    for position in range(4 if is_ultra else 3):                                  # an x with no root, in each position
        bad = VF.without_root(comp, position, is_ultra)
        assert bad != comp and VF.to_plain(COMPRESSED, bad, blocks[1], is_ultra)[0] is None
        assert VF.convert(is_ultra, COMPRESSED, bad, PLAIN) == (1, untouched(PLAIN))
        assert VF.convert(is_ultra, COMPRESSED, bad, EVM) == (1, untouched(EVM))
        junk = VF.as_infinity_with_junk(comp, position, is_ultra)                 # the flag decides, whatever the other bits say
        want = VF.to_plain(COMPRESSED, junk, blocks[1], is_ultra)[0]
        lo, hi = [(0, 64), (64, 192), (192, 256), (256, 320)][position]
        assert want == VF.reduced(recs[1])[:lo] + bytes(hi - lo) + VF.reduced(recs[1])[hi:]
        assert VF.convert(is_ultra, COMPRESSED, junk, PLAIN) == (0, want)
        junk_and_rootless = VF.as_infinity_with_junk(bad, position, is_ultra)
        assert VF.convert(is_ultra, COMPRESSED, junk_and_rootless, PLAIN) == (0, want)
    moved = [VF.x_plus_q(VF.to_compressed(r), p, is_ultra) for r in recs for p in range(3)]
    moved = [m for m in moved if m is not None]
    assert moved                                                                  # x + q inside the 254 bits reduces to x
    for m in moved[:4]:
        assert VF.convert(is_ultra, COMPRESSED, m, PLAIN) == (0, VF.to_plain(COMPRESSED, m, blocks[0], is_ultra)[0])
    L = VB.lib()
    out = C.create_string_buffer(320)
    for a, b in ((3, PLAIN), (PLAIN, 3), (-1, EVM), (COMPRESSED, 99)):
        assert L.ug_proof_record_convert(int(is_ultra), a, recs[0], b, out) == 2
    assert L.ug_proof_record_convert(int(is_ultra), PLAIN, None, EVM, out) == 2 and L.ug_proof_record_convert(int(is_ultra), PLAIN, recs[0], EVM, None) == 2
    assert [L.ug_proof_record_bytes(int(is_ultra), f) for f in (PLAIN, EVM, COMPRESSED, 3, -1)] == [VF.size(is_ultra, f) for f in (PLAIN, EVM, COMPRESSED)] + [0, 0]


def test_fq2_sqrt_host():
    values = VF.sqrt_inputs()
    roots, has = VF.fq2_sqrt(-1, values)
    VF.check_sqrt(values, roots, has)
    assert has[:9] == [1] * 9 and has.count(0) >= 24                              # zero, the reals and the purely imaginary all have roots
    assert roots[3][0] == 0 and roots[3][1] != 0 and roots[1][1] == 0             # a real non-residue: a purely imaginary root
    assert any(r[1] == 0 and r[0] != 0 for r in roots) and any(r[1] != 0 for r in roots)


@pytest.mark.parametrize("is_ultra", [False, True])
@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
def test_host_ingest_reads_the_layouts(g16, ultra, fmt, is_ultra):
    """ug_test_records_ingest with device = -1, the reference of the device test: status and plain records as the layouts say"""
    recs = (ultra if is_ultra else g16)[2]
    batch = VF.ingest_batch(fmt, recs, is_ultra, 32)
    plain, status = VF.ingest(-1, fmt, is_ultra, batch)
    k = 4 if is_ultra else 3
    for i in range(32):
        kind = i % 16
        assert status[i] == (VF.OFF_CURVE if 6 <= kind < 6 + k else VF.OFF_SUBGROUP if kind == 5 else VF.OK), i
        stands = VF.to_plain(fmt, batch[i], b"", is_ultra)[0]
        if status[i] != VF.OFF_CURVE:
            assert plain[i] == stands, i
        else:                                                                     # the point that failed is zeros, the others are there
            lo, hi = [(0, 64), (64, 192), (192, 256), (256, 320)][kind - 6]
            good = VF.reduced(recs[i])
            assert plain[i] == good[:lo] + bytes(hi - lo) + good[hi:], i
            assert stands is None or fmt == EVM


@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
@pytest.mark.parametrize("kind", VR.KINDS + VR.BINARY_KINDS)
def test_kinds_of_bad_record(g16, fmt, kind):
    proofs, pubs, recs, blocks, vk = g16
    at = 17
    pairs = [VF.to_format(fmt, r, b) for r, b in zip(recs[:19], blocks[:19])]
    out_r, out_b = [r for r, _ in pairs], [b for _, b in pairs]
    stands = [(r, b, None) for r, b in zip(recs[:19], blocks[:19])]
    out_r[at], out_b[at], stands[at] = VF.expressed(fmt, kind, recs[at], blocks[at], proofs[at], pubs[at])
    expect = [VALID] * 19
    expect[at] = VF.expected_one(False, stands[at], vk)
    if kind in VR.KINDS:
        assert expect[at] == INVALID
    rc, msg, verdicts, stats = VF.batch_fmt(False, fmt, out_r, out_b, vk)
    rc_p, msg_p, verdicts_p, stats_p = VF.plain_call_on(False, stands, vk)
    assert verdicts == expect and (rc, msg, verdicts) == (rc_p, msg_p, verdicts_p)
    assert rc == expect[at] and msg == ("" if rc == VALID else "proof %d: invalid proof" % at)
    assert stats["off_subgroup"] == stats_p["off_subgroup"] == (1 if kind == "B off subgroup" else 0)
    if kind == "C off curve" or stands[at][0] is None:                            # answered without a pairing: the other 18 hold
        assert stats["single_checks"] == 0 and stats["batch_checks"] == 1


def test_all_zero_compressed_record_is_what_the_reference_says():
    """x = 0: 3 is no square mod q, so the G1 points have no y and the record stands for nothing"""
    assert pow(3, (VF.Q - 1) // 2, VF.Q) == VF.Q - 1
    pts, failed = VF.from_compressed(bytes(128))
    assert failed[0] and failed[2] and failed[1] == (VB.f2_sqrt(VF.B2) is None)
    assert VF.convert(False, COMPRESSED, bytes(128), PLAIN)[0] == 1


@pytest.mark.parametrize("is_ultra", [False, True])
@pytest.mark.parametrize("judge", [0, 1])
@pytest.mark.parametrize("fmt", [EVM, COMPRESSED], ids=lambda f: NAMES[f])
def test_mixed_batch(g16, ultra, fmt, judge, is_ultra):
    proofs, pubs, recs, blocks, vk = ultra if is_ultra else g16
    out_r, out_b, stands, expect = VF.mixed(fmt, recs, blocks, proofs, pubs, vk, is_ultra)
    assert [i for i, v in enumerate(expect) if v != VALID] == [0, 15, 16, 31, 32] and expect.count(INVALID) == 5
    opt = VR.options(judge, judge_min=1)
    rc, msg, verdicts, stats = VF.batch_fmt(is_ultra, fmt, out_r, out_b, vk, opt=opt)
    rc_p, msg_p, verdicts_p, stats_p = VF.plain_call_on(is_ultra, stands, vk, opt=opt)
    assert (rc, msg, verdicts) == (rc_p, msg_p, verdicts_p) == (INVALID, "proof 0: invalid proof", expect)
    assert stats["off_subgroup"] == stats_p["off_subgroup"] == 1
    assert (stats["judged"] > 0) == (stats_p["judged"] > 0) == bool(judge)


def test_ultragroth_challenge_follows_pi_r(ultra):
    """another proof's round commitment in a compressed record: the challenge moves and the proof fails, as in PLAIN"""
    proofs, pubs, recs, blocks, vk = ultra
    recs = list(recs[:5])
    recs[4] = recs[4][:256] + recs[0][256:]
    comp = [VF.to_compressed(r) for r in recs]
    expect = VR.expected(True, recs, blocks[:5], vk)
    assert expect == [VALID] * 4 + [INVALID]
    assert VF.batch_fmt(True, COMPRESSED, comp, blocks[:5], vk)[2] == expect


def test_call_errors(g16):
    proofs, pubs, recs, blocks, vk = g16
    L = VB.lib()
    key = json.dumps(vk).encode()
    n_pub = len(blocks[0]) // 32
    same = VR.mixed_batch(recs, blocks, proofs, pubs)                             # _fmt with PLAIN is the old entry point
    old = VR.batch_records(False, same[0], same[1], vk, opt=VR.options(0))
    new = VF.batch_fmt(False, PLAIN, same[0], same[1], vk, opt=VR.options(0))
    counters = lambda st: {k: v for k, v in st.items() if not k.endswith("_ms")}
    assert old[:3] == new[:3] and counters(old[3]) == counters(new[3]) and old[0] == INVALID
    for fmt in (EVM, COMPRESSED):
        pairs = [VF.to_format(fmt, r, b) for r, b in zip(recs[:2], blocks[:2])]
        rb, ib = pairs[0][0] + pairs[1][0], pairs[0][1] + pairs[1][1]
        for args, text in (((fmt, 2, None, ib, n_pub, key), "null argument"), ((fmt, 2, rb, None, n_pub, key), "null argument"),
                           ((fmt, 2, rb, ib, n_pub, None), "null argument"), ((fmt, -1, rb, ib, n_pub, key), "null argument"),
                           ((fmt, 2, rb, ib, 0, key), "invalid inputs data"),
                           ((fmt, 2, rb, ib, n_pub + 1, key), "len(inputs)+1 != len(vk.IC)"),
                           ((3, 2, rb, ib, n_pub, key), "format"), ((-1, 2, rb, ib, n_pub, key), "format"),
                           ((fmt, 2, rb, ib, n_pub, key[:len(key) // 2]), "invalid verification key data")):
            verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
            err = C.create_string_buffer(256)
            f, count, r, i, np_, k = args
            assert L.ug_groth16_verify_batch_records_fmt(-1, f, count, r, i, np_, k, verdicts, None, None, err, 255) == ERROR
            got = err.value.decode()
            assert (got.startswith("format:") if text == "format" else got == text) and list(verdicts) == [VB.SENTINEL] * 2
        verdicts = (C.c_int * 2)(VB.SENTINEL, VB.SENTINEL)
        assert L.ug_groth16_verify_batch_records_fmt(-1, fmt, 2, rb, ib, n_pub, key, verdicts, None, None, None, 0) == VALID and list(verdicts) == [VALID] * 2
        assert L.ug_groth16_verify_batch_records_fmt(-1, fmt, 0, None, None, n_pub, key, None, None, None, None, 0) == VALID
        assert L.ug_ultra_groth_verify_batch_records_fmt(-1, fmt, 2, rb, ib, n_pub, key, verdicts, None, None, None, 0) == ERROR     # a Groth16 key


def test_python_entry_points(g16):
    import ultragroth_amd as ug
    proofs, pubs, recs, blocks, vk = g16
    assert (ug.RECORDS_PLAIN, ug.RECORDS_EVM, ug.RECORDS_COMPRESSED) == (PLAIN, EVM, COMPRESSED)
    comp = ug.proof_record_convert(recs[0], ug.RECORDS_PLAIN, ug.RECORDS_COMPRESSED)
    assert comp == VF.to_compressed(recs[0]) and ug.proof_record_convert(comp, ug.RECORDS_COMPRESSED, ug.RECORDS_EVM) == VF.to_evm(recs[0])
    assert ug.inputs_convert(blocks[0], ug.RECORDS_PLAIN, ug.RECORDS_EVM) == VF.evm_inputs(blocks[0])
    with pytest.raises(ValueError):
        ug.proof_record_convert(VF.without_root(comp, 0), ug.RECORDS_COMPRESSED, ug.RECORDS_PLAIN)
    with pytest.raises(ValueError):
        ug.proof_record_convert(recs[0], ug.RECORDS_PLAIN, 5)
    with pytest.raises(ValueError):
        ug.proof_record_convert(recs[0], ug.RECORDS_COMPRESSED, ug.RECORDS_PLAIN)       # 256 bytes are no compressed record
    n_pub = len(blocks[0]) // 32
    three = b"".join(VF.to_compressed(r) for r in recs[:3])
    verdicts, stats = ug.groth16_verify_batch_records(three, b"".join(blocks[:3]), n_pub, vk, device=-1, format=ug.RECORDS_COMPRESSED)
    assert verdicts == [VALID] * 3 and stats["batch_checks"] == 1
    verdicts, stats = ug.groth16_verify_batch_records(b"".join(VF.to_evm(r) for r in recs[:3]), b"".join(VF.evm_inputs(b) for b in blocks[:3]), n_pub, vk,
                                                      device=-1, format=ug.RECORDS_EVM)
    assert verdicts == [VALID] * 3
    with pytest.raises(ValueError):
        ug.groth16_verify_batch_records(three + b"\0", b"".join(blocks[:3]), n_pub, vk, device=-1, format=ug.RECORDS_COMPRESSED)
    with pytest.raises(ValueError):
        ug.groth16_verify_batch_records(three, b"".join(blocks[:3]), n_pub, vk, device=-1, format=9)
    assert ug.groth16_verify_batch_records(b"".join(recs[:3]), b"".join(blocks[:3]), n_pub, vk, device=-1)[0] == [VALID] * 3


def test_symbols_and_kernels():
    import ultragroth_amd as ug
    from ultragroth_amd import _lib
    lib = ug.load()
    header = open(os.path.join(ROOT, "include", "verifier.h")).read()
    for name in ("ug_proof_record_bytes", "ug_groth16_verify_batch_records_fmt", "ug_ultra_groth_verify_batch_records_fmt",
                 "ug_proof_record_convert", "ug_inputs_convert", "ug_test_records_ingest", "ug_test_fq2_sqrt"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.VERIFIER_SYMBOLS and hasattr(lib, name), name
    assert "caller's to convert" not in header
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"records_decompress_kernel" in blob and b"fq2_sqrt_kernel" in blob and blob.count(b"records_ingest_kernel") >= 2
