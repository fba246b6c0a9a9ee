"""Shared by tests/test_verify_formats_host.py and tests/test_gpu_verify_formats.py: the record layouts of include/verifier.h
(UG_RECORDS_EVM, UG_RECORDS_COMPRESSED) restated in Python on oracle.pairing's integers, independent of the library, the raw calls of
the _fmt entry points, the conversion calls and the two test hooks. Expected verdicts are the single verifier's on the unpacked text
of the PLAIN record a record stands for (verify_records_cases.single), never the batch code's."""
import ctypes as C
import random

import verify_batch_cases as VB
import verify_records_cases as VR
from verify_batch_cases import INVALID, SENTINEL
from oracle import pairing as PR

PLAIN, EVM, COMPRESSED = 0, 1, 2
NEW_FORMATS = [EVM, COMPRESSED]
Q = PR.P
HALF = (Q - 1) // 2
FLAG_INF, FLAG_LARGER = 0x40, 0x80
B2 = PR.f2_muls(PR.f2_inv(PR.XI), 3)                                  # the twist's constant term, 3 / (9 + u)
OK, OFF_CURVE, OFF_SUBGROUP = 0, 2, 3                                 # UG_POINT_* of include/ultragroth_hip.h


def size(ultra, fmt):
    return {PLAIN: (256, 320), EVM: (256, 320), COMPRESSED: (128, 160)}[fmt][1 if ultra else 0]


# ---- the layouts, from their description -------------------------------------------------------------------------------------
def coords(rec):
    """the 8 (10) integers of a PLAIN record, as stored"""
    return [int.from_bytes(rec[at:at + 32], "little") for at in range(0, len(rec), 32)]


def points(rec):
    """a PLAIN record as points on reduced integers: [a, b, c] or [a, b, f, r]; None = infinity; b = ((x0, x1), (y0, y1))"""
    v = [c % Q for c in coords(rec)]
    g1 = lambda x, y: None if (x, y) == (0, 0) else (x, y)
    b = None if v[2:6] == [0, 0, 0, 0] else ((v[2], v[3]), (v[4], v[5]))
    return [g1(v[0], v[1]), b] + [g1(v[at], v[at + 1]) for at in range(6, len(v), 2)]


def _le(x):
    return x.to_bytes(32, "little")


def _be(x):
    return x.to_bytes(32, "big")


def from_points(pts):
    """points -> the PLAIN record of reduced coordinates"""
    out = b""
    for i, p in enumerate(pts):
        if i == 1:
            out += bytes(128) if p is None else _le(p[0][0]) + _le(p[0][1]) + _le(p[1][0]) + _le(p[1][1])
        else:
            out += bytes(64) if p is None else _le(p[0]) + _le(p[1])
    return out


def reduced(rec):
    return from_points(points(rec))


def to_evm(rec):
    out = b""
    for i, p in enumerate(points(rec)):
        if i == 1:
            out += bytes(128) if p is None else _be(p[0][1]) + _be(p[0][0]) + _be(p[1][1]) + _be(p[1][0])
        else:
            out += bytes(64) if p is None else _be(p[0]) + _be(p[1])
    return out


def evm_inputs(block):
    return b"".join(block[at:at + 32][::-1] for at in range(0, len(block), 32))


def larger1(y):
    return y > HALF


def larger2(y):
    return y[1] > HALF if y[1] else y[0] > HALF


def _flagged(body, flags):
    return body[:-1] + bytes([body[-1] | flags])


def to_compressed(rec):
    """None when a point is off its curve: a sign bit cannot stand for it"""
    out = b""
    for i, p in enumerate(points(rec)):
        if p is None:
            out += _flagged(bytes(64 if i == 1 else 32), FLAG_INF)
        elif i == 1:
            if not PR.g2_on_curve(p):
                return None
            out += _flagged(_le(p[0][0]) + _le(p[0][1]), FLAG_LARGER if larger2(p[1]) else 0)
        else:
            if not PR.g1_on_curve(p):
                return None
            out += _flagged(_le(p[0]), FLAG_LARGER if larger1(p[1]) else 0)
    return out


def f1_sqrt(a):
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def from_compressed(rec, ultra=False):
    """(points, which of them had no root): a point without a root is left as None"""
    pts, failed, at = [], [], 0
    for i in range(4 if ultra else 3):
        n = 64 if i == 1 else 32
        body = rec[at:at + n]
        at += n
        flags, body = body[-1] & 0xc0, body[:-1] + bytes([body[-1] & 0x3f])
        if flags & FLAG_INF:
            pts.append(None)
        elif i == 1:
            x = (int.from_bytes(body[:32], "little") % Q, int.from_bytes(body[32:], "little") % Q)
            y = VB.f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), B2))
            if y is not None and larger2(y) != bool(flags & FLAG_LARGER):
                y = PR.f2_neg(y)
            pts.append(None if y is None else (x, y))
            failed.append(y is None)
            continue
        else:
            x = int.from_bytes(body, "little") % Q
            y = f1_sqrt(x * x * x + 3)
            if y is not None and larger1(y) != bool(flags & FLAG_LARGER):
                y = Q - y
            pts.append(None if y is None else (x, y))
            failed.append(y is None)
            continue
        failed.append(False)
    return pts, failed


def to_format(fmt, rec, block):
    """(record, input block) of the PLAIN pair in layout `fmt`; the record None when it has no such form"""
    if fmt == EVM:
        return to_evm(rec), evm_inputs(block)
    if fmt == COMPRESSED:
        return to_compressed(rec), block
    return rec, block


def to_plain(fmt, rec, block, ultra=False):
    """the PLAIN pair a record of layout `fmt` stands for (the reference's reading); the record None for an x without a root"""
    if fmt == EVM:
        v = [int.from_bytes(rec[at:at + 32], "big") for at in range(0, len(rec), 32)]
        v[2], v[3], v[4], v[5] = v[3], v[2], v[5], v[4]
        return reduced(b"".join(_le(c) for c in v)), evm_inputs(block)
    if fmt == COMPRESSED:
        pts, failed = from_compressed(rec, ultra)
        return (None if any(failed) else from_points(pts)), block
    return rec, block


def rootless_g1_x(x):
    """the next x above `x` whose x^3 + 3 is no square (checked by Euler's criterion)"""
    while True:
        x = (x + 1) % Q
        if pow((x * x * x + 3) % Q, (Q - 1) // 2, Q) == Q - 1:
            return x


def rootless_g2_x(x):
    """... and for the twist: x.c0 stepped until x^3 + b2 is no square in Fq2 (its norm is none in Fq)"""
    while True:
        x = ((x[0] + 1) % Q, x[1])
        a = PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), B2)
        if pow((a[0] * a[0] + a[1] * a[1]) % Q, (Q - 1) // 2, Q) == Q - 1:
            assert VB.f2_sqrt(a) is None
            return x


def point_slices(ultra):
    """byte ranges of the points of a COMPRESSED record: pi_a, pi_b, pi_c / pi_f [, pi_r]"""
    return [(0, 32), (32, 96), (96, 128)] + ([(128, 160)] if ultra else [])


def without_root(comp, position, ultra=False):
    """the COMPRESSED record with the x of point `position` moved to one without a y on the curve"""
    lo, hi = point_slices(ultra)[position]
    body = comp[lo:hi]
    flags = body[-1] & FLAG_LARGER
    body = body[:-1] + bytes([body[-1] & 0x3f])
    if position == 1:
        x = rootless_g2_x((int.from_bytes(body[:32], "little"), int.from_bytes(body[32:], "little")))
        body = _le(x[0]) + _le(x[1])
    else:
        body = _le(rootless_g1_x(int.from_bytes(body, "little")))
    return comp[:lo] + _flagged(body, flags) + comp[hi:]


def as_infinity_with_junk(comp, position, ultra=False):
    lo, hi = point_slices(ultra)[position]
    return comp[:lo] + _flagged(comp[lo:hi], FLAG_INF) + comp[hi:]


def x_plus_q(comp, position, ultra=False):
    """x + q where that still fits the 254 bits (q < 2^254 < 2 q, so only an x below 2^254 - q does); else None"""
    lo, hi = point_slices(ultra)[position]
    body = comp[hi - 32:hi]
    flags = body[-1] & 0xc0
    x = int.from_bytes(body[:-1] + bytes([body[-1] & 0x3f]), "little") + Q
    if x >> 254:
        return None
    return comp[:hi - 32] + _flagged(_le(x), flags) + comp[hi:]


# ---- raw calls ------------------------------------------------------------------------------------------------------------------
def convert(ultra, from_fmt, rec, to_fmt, out_size=None):
    """(return code, bytes written): the output buffer starts as 0x55 bytes, so an untouched one shows"""
    n = out_size or size(ultra, to_fmt) or 320
    out = C.create_string_buffer(b"\x55" * n, n)
    rc = VB.lib().ug_proof_record_convert(1 if ultra else 0, from_fmt, rec, to_fmt, out)
    return rc, out.raw


def convert_inputs(from_fmt, block, to_fmt):
    out = C.create_string_buffer(len(block))
    rc = VB.lib().ug_inputs_convert(from_fmt, block, len(block) // 32, to_fmt, out)
    return rc, out.raw


def batch_fmt(ultra, fmt, recs, blocks, vk, device=-1, opt=None, n_pub=None):
    """raw call of ug_*_verify_batch_records_fmt: (rc, message, verdicts, stats dict)"""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_records_fmt if ultra else L.ug_groth16_verify_batch_records_fmt
    n = len(recs)
    if n_pub is None:
        n_pub = len(blocks[0]) // 32 if blocks else len(vk["IC"]) - 1
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStatsEx(), C.create_string_buffer(512)
    rc = fn(device, fmt, n, b"".join(recs) or b"\0", b"".join(blocks) or b"\0", n_pub, VB._enc(vk), verdicts,
            C.byref(opt) if opt is not None else None, C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), VR._stats(stats)


def ingest(device, fmt, ultra, recs):
    """ug_test_records_ingest: (the plain records the arrays hold, the status bytes)"""
    n = len(recs)
    out, status = C.create_string_buffer(VR.rec_size(ultra) * n), C.create_string_buffer(n)
    assert VB.lib().ug_test_records_ingest(device, fmt, 1 if ultra else 0, n, b"".join(recs), out, status) == 0
    w = VR.rec_size(ultra)
    return [out.raw[i * w:(i + 1) * w] for i in range(n)], list(status.raw)


def fq2_sqrt(device, values):
    """ug_test_fq2_sqrt of (c0, c1) pairs: (roots as pairs, has_root bytes)"""
    n = len(values)
    data = b"".join(_le(a) + _le(b) for a, b in values)
    out, has = C.create_string_buffer(64 * n), C.create_string_buffer(n)
    assert VB.lib().ug_test_fq2_sqrt(device, n, data, out, has) == 0
    roots = [(int.from_bytes(out.raw[64 * i:64 * i + 32], "little"), int.from_bytes(out.raw[64 * i + 32:64 * i + 64], "little")) for i in range(n)]
    return roots, list(has.raw)


def sqrt_inputs():
    """the degenerate inputs of f2_sqrt and a few dozen random squares and non-squares; fixed seed"""
    rng = random.Random(20240607)
    non_residue = next(a for a in range(2, 50) if pow(a, (Q - 1) // 2, Q) == Q - 1)
    residue = next(a for a in range(2, 50) if pow(a, (Q - 1) // 2, Q) == 1)
    vals = [(0, 0), (residue, 0), (4, 0), (non_residue, 0), (Q - 1, 0), (0, 1), (0, 5), (0, Q - 2), (1, 1), B2]
    for _ in range(24):
        r = (rng.randrange(Q), rng.randrange(Q))
        vals.append(PR.f2_mul(r, r))
    while len(vals) < 10 + 24 + 24:
        v = (rng.randrange(Q), rng.randrange(Q))
        if VB.f2_sqrt(v) is None:
            vals.append(v)
    vals.append((residue + Q, Q))                                                 # values at or above q reduce first
    return vals


def check_sqrt(values, roots, has):
    for v, r, h in zip(values, roots, has):
        v = (v[0] % Q, v[1] % Q)
        want = VB.f2_sqrt(v)
        assert h == (0 if want is None else 1), v
        if want is None:
            assert r == (0, 0)
        else:
            assert PR.f2_mul(r, r) == v and r[0] < Q and r[1] < Q, v
            assert r == (0, 0) or not larger2(r), v


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def expressed(fmt, kind, rec, block, proof, pub, ultra=False):
    """the bad record of `kind` (verify_records_cases) in layout `fmt`, as (record, block, stands): stands = (the PLAIN record it
    stands for or None when it stands for none, the PLAIN block, a PLAIN record with a point off its curve -- what a record that
    stands for none is handled like). The EVM record holds the PLAIN record's integers as they are, NOT reduced, so a coordinate
    + q or 2^256 - 1 and an input + r reach the call as such, and `stands` is the unreduced PLAIN pair: the single verifier and the
    PLAIN call judge the text with the same values. An off-curve point has no compressed form: there the kind becomes "x with no
    root" in the same position; the all-zero record is, compressed, points with x = 0."""
    if kind in VR.KINDS:
        bad, bad_block = VR.bad_record(kind, proof, pub, ultra)
    else:
        bad, bad_block = VR.binary_record(kind, rec, block)
    off_curve = VR._put(rec, 224, VR._get(rec, 224) ^ 1)
    if fmt == COMPRESSED and kind == "all-zero record":
        comp = bytes(size(ultra, COMPRESSED))
        return comp, bad_block, (to_plain(COMPRESSED, comp, bad_block, ultra)[0], bad_block, off_curve)
    if fmt == EVM:
        out, out_block = _raw_evm(bad), evm_inputs(bad_block)
        top = max(int.from_bytes(out[at:at + 32], "big") for at in range(0, len(out), 32))
        if kind in ("pi_a.x + q", "pi_b.y.c1 + q", "coordinate 2^256 - 1"):
            assert top >= Q and (kind != "coordinate 2^256 - 1" or top == (1 << 256) - 1)      # the value at or above q is in the record sent
        if kind == "input + r":
            assert int.from_bytes(out_block[:32], "big") >= PR.R
        return out, out_block, (bad, bad_block, off_curve)
    out, out_block = to_format(fmt, bad, bad_block)
    if out is None:                                                               # COMPRESSED: each point off its curve -> an x with no root
        out = to_compressed(rec)
        for position, p in enumerate(points(bad)):
            if p is not None and not (PR.g2_on_curve(p) if position == 1 else PR.g1_on_curve(p)):
                out = without_root(out, position, ultra)
        assert to_plain(COMPRESSED, out, bad_block, ultra)[0] is None
        return out, out_block, (None, bad_block, off_curve)
    return out, out_block, (bad, bad_block, off_curve)


def expected_one(ultra, stands, vk):
    """the single verifier's word on the PLAIN pair; a record that stands for none is INVALID, like a point off its curve"""
    rec, block, off_curve = stands
    if rec is None:
        assert VR.single(ultra, off_curve, block, vk) == INVALID
        return INVALID
    return VR.single(ultra, rec, block, vk)


def mixed(fmt, recs, blocks, proofs, pubs, vk, ultra=False):
    """verify_records_cases.mixed_batch in layout `fmt`: (records, blocks, what they stand for as in expressed(), expected verdicts)"""
    places = {0: "A.y negated", 15: "C off curve", 16: "C = generator", 31: "B off subgroup", 32: "A = infinity"}
    out_r, out_b, plain = [], [], []
    for i, (rec, block) in enumerate(zip(recs, blocks)):
        if i in places:
            r, b, pair = expressed(fmt, places[i], rec, block, proofs[i], pubs[i], ultra)
        else:
            (r, b), pair = to_format(fmt, rec, block), (rec, block, None)
        out_r.append(r)
        out_b.append(b)
        plain.append(pair)
    expect = [expected_one(ultra, pair, vk) if i in places else VB.VALID for i, pair in enumerate(plain)]
    return out_r, out_b, plain, expect


def plain_call_on(ultra, plain, vk, device=-1, opt=None):
    """the PLAIN call on the converted records; a record that stands for none goes in as one with a point off its curve, which is
    what it is handled like"""
    recs = [off_curve if rec is None else rec for rec, _, off_curve in plain]
    return VR.batch_records(ultra, recs, [block for _, block, _ in plain], vk, device=device, opt=opt)


def ingest_batch(fmt, recs, ultra, count):
    """`count` records of layout `fmt` from the valid PLAIN `recs`: valid ones of both signs, infinity flags, x >= q, an x with no root
    in each point position (COMPRESSED) or a point off its curve in each (EVM), and a pi_b off the subgroup"""
    k = 4 if ultra else 3
    off_b = VR.pack(VB.bad_proof("B off subgroup", VR.unpack(recs[0], ultra), "[\"1\"]", ultra)[0], ultra)
    out = []
    for i in range(count):
        rec = recs[i % len(recs)]
        kind = i % 16
        if kind == 1:                                                             # the other sign of pi_a
            rec = VR._put(rec, 32, Q - VR._get(rec, 32))
        if kind == 5:
            rec = rec[:64] + off_b[64:192] + rec[192:]
        if fmt == EVM:
            if kind == 2:
                rec = VR._put(rec, 0, VR._get(rec, 0) + Q)                        # x >= q
            if kind == 3:
                rec = bytes(64) + rec[64:]                                        # pi_a = infinity
            if kind == 4:
                rec = rec[:64] + bytes(128) + rec[192:]
            if 6 <= kind < 6 + k:                                                 # one point off its curve, each position in turn
                at = (32, 160, 224, 288)[kind - 6]
                rec = VR._put(rec, at, VR._get(rec, at) ^ 1)
            out.append(_raw_evm(rec))
            continue
        if kind == 2:                                                             # x >= q: the next record with an x that + q still fits 254 bits
            moved = None
            for j in range(len(recs)):
                rec = recs[(i + j) % len(recs)]
                for position in range(k):
                    moved = moved or x_plus_q(to_compressed(rec), position, ultra)
                if moved:
                    break
            assert moved is not None and moved != to_compressed(rec) and to_plain(COMPRESSED, moved, b"", ultra)[0] == reduced(rec)
            out.append(moved)
            continue
        comp = to_compressed(rec)
        if kind == 3:
            comp = as_infinity_with_junk(comp, 0, ultra)
        if kind == 4:
            comp = as_infinity_with_junk(comp, 1, ultra)
        if 6 <= kind < 6 + k:
            comp = without_root(comp, kind - 6, ultra)
        out.append(comp)
    return out


def _raw_evm(rec):
    """a PLAIN record's integers in the EVM order, NOT reduced (so a coordinate + q stays one)"""
    v = coords(rec)
    v[2], v[3], v[4], v[5] = v[3], v[2], v[5], v[4]
    return b"".join(_be(c) for c in v)
