"""Point validation on the device (check.hip): field range, curve equation and G2 subgroup membership of zkey records, through the
inner call (ug_points_check), the creation switch (ug_ctx_check_points), ULTRAGROTH_VALIDATE on every kind of prover, and the
standalone ug_zkey_check. Reference points come from oracle/pairing.py arithmetic plus the Fq2 square root below."""
import ctypes as C
import os
import struct

import pytest

from conftest import fixed_rs, GOLDEN
from oracle import pairing as PR

pytestmark = pytest.mark.gpu

Q, R = PR.P, PR.R
MONT = 1 << 256
T_UNREDUCED, T_CURVE, T_SUBGROUP = ("coordinate not below the field modulus", "not on the curve", "not in the subgroup of order r")


# ---- reference arithmetic ------------------------------------------------------------------------------------------------
def raw(v):
    return int(v).to_bytes(32, "little")


def mont(x):
    return raw(x * MONT % Q)


def g1_rec(p):
    return bytes(64) if p is None else mont(p[0]) + mont(p[1])


def g2_rec(p):
    return bytes(128) if p is None else mont(p[0][0]) + mont(p[0][1]) + mont(p[1][0]) + mont(p[1][1])


def coords(rec):
    """the raw 256-bit integers of a record"""
    return [int.from_bytes(rec[k:k + 32], "little") for k in range(0, len(rec), 32)]


def from_coords(cs):
    return b"".join(raw(c) for c in cs)


def bump_y(rec):
    """y + 1 (the first component of y for G2), still canonical: off the curve"""
    cs = coords(rec)
    k = len(cs) // 2
    cs[k] = (cs[k] + MONT) % Q
    return from_coords(cs)


def unreduced(rec, k):
    """component k as the raw integer + q: the same point, below 2^256, not below q"""
    cs = coords(rec)
    cs[k] += Q
    assert cs[k] < MONT
    return from_coords(cs)


def f2_sqrt(a):
    """square root in Fq2 = Fq[u]/(u^2+1), q = 3 mod 4 (complex method); None when a is no square"""
    if a == (0, 0):
        return a
    a1 = PR.f2_pow(a, (Q - 3) // 4)
    x0 = PR.f2_mul(a1, a)
    alpha = PR.f2_mul(a1, x0)
    if alpha == (Q - 1, 0):
        x = PR.f2_mul((0, 1), x0)
    else:
        x = PR.f2_mul(PR.f2_pow(PR.f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    return x if PR.f2_mul(x, x) == a else None


def g2_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = PR.g2_dbl(acc)
        if bit == "1":
            acc = PR.g2_add(acc, p)
    return acc


@pytest.fixture(scope="module")
def twist():
    """P: on the twist, outside the subgroup; Qc = [r]P: of order dividing the cofactor 2q - r; S = [2q - r]P: in the subgroup"""
    b2 = PR.f2_muls(PR.f2_inv(PR.XI), 3)
    x = (1, 0)
    y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), b2))
    assert y is not None
    P = (x, y)
    assert PR.g2_on_curve(P)
    Qc = g2_mul(P, R)
    assert Qc is not None and PR.g2_on_curve(Qc)
    S = g2_mul(P, 2 * Q - R)
    assert S is not None and g2_mul(S, R) is None
    return {"P": g2_rec(P), "Q": g2_rec(Qc), "S": g2_rec(S)}


@pytest.fixture(scope="module")
def good(device):
    """good points, computed once: 257 synthetic ones per curve"""
    from ultragroth_amd import synth
    return {False: bytes(synth.synth_points(device, 257, 0x1234, g2=False)), True: bytes(synth.synth_points(device, 257, 0x4321, g2=True))}


def put(recs, i, rec):
    n = len(rec)
    return recs[:i * n] + rec + recs[(i + 1) * n:]


# ---- inner call: each rule, each curve ------------------------------------------------------------------------------------
def test_good_points_pass(device, good, twist):
    from ultragroth_amd import synth
    g1 = (1, 2)
    pts1 = good[False] + g1_rec(g1) + g1_rec((1, Q - 2)) + bytes(64)
    assert device.check_points(pts1, len(pts1) // 64, g2=False, level=2) is None
    G = synth.G2_GEN
    neg = (G[0], PR.f2_neg(G[1]))
    pts2 = good[True] + g2_rec(G) + g2_rec(neg) + bytes(128) + twist["S"]
    assert device.check_points(pts2, len(pts2) // 128, g2=True, level=1) is None
    assert device.check_points(pts2, len(pts2) // 128, g2=True, level=2) is None


def test_unreduced_coordinate(device, good):
    """the raw words decide: x + q is the same point once reduced"""
    import ultragroth_amd as ug
    pick = lambda g2, ok: next(i for i in range(257) if ok(coords(good[g2][i * (128 if g2 else 64):][: 128 if g2 else 64])))
    i = pick(False, lambda cs: cs[0] + Q < MONT)
    rec = unreduced(good[False][i * 64:(i + 1) * 64], 0)
    assert device.check_points(put(good[False], i, rec), 257, level=1) == (i, ug.UG_POINT_UNREDUCED)
    for k in range(4):
        i = pick(True, lambda cs: cs[k] + Q < MONT)
        rec = unreduced(good[True][i * 128:(i + 1) * 128], k)
        assert device.check_points(put(good[True], i, rec), 257, g2=True, level=1) == (i, ug.UG_POINT_UNREDUCED), k


def test_off_curve(device, good):
    import ultragroth_amd as ug
    assert device.check_points(put(good[False], 100, bump_y(good[False][6400:6464])), 257) == (100, ug.UG_POINT_OFF_CURVE)
    assert device.check_points(put(good[True], 100, bump_y(good[True][12800:12928])), 257, g2=True) == (100, ug.UG_POINT_OFF_CURVE)
    assert device.check_points(put(good[True], 100, bump_y(good[True][12800:12928])), 257, g2=True, level=2) == (100, ug.UG_POINT_OFF_CURVE)


def test_off_subgroup(device, good, twist):
    import ultragroth_amd as ug
    for name in ("P", "Q"):
        pts = put(good[True], 7, twist[name])
        assert device.check_points(pts, 257, g2=True, level=1) is None
        assert device.check_points(pts, 257, g2=True, level=2) == (7, ug.UG_POINT_OFF_SUBGROUP)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_shapes(device, good, twist, n):
    import ultragroth_amd as ug
    for at in sorted({0, n // 2, n - 1}):
        assert device.check_points(put(good[False][:n * 64], at, bump_y(good[False][at * 64:(at + 1) * 64])), n) == (at, ug.UG_POINT_OFF_CURVE)
        assert device.check_points(put(good[True][:n * 128], at, twist["P"]), n, g2=True, level=2) == (at, ug.UG_POINT_OFF_SUBGROUP)


def test_lowest_index_and_first_rule_win(device, good, twist):
    import ultragroth_amd as ug
    pts = put(put(good[False], 200, bump_y(good[False][200 * 64:201 * 64])), 31, bump_y(good[False][31 * 64:32 * 64]))
    assert device.check_points(pts, 257) == (31, ug.UG_POINT_OFF_CURVE)
    pts = put(put(good[True], 40, twist["P"]), 41, bump_y(good[True][41 * 128:42 * 128]))      # the lower index, not the lower reason
    assert device.check_points(pts, 257, g2=True, level=2) == (40, ug.UG_POINT_OFF_SUBGROUP)
    i = next(i for i in range(257) if coords(good[False][i * 64:(i + 1) * 64])[0] + Q < MONT)
    both = unreduced(bump_y(good[False][i * 64:(i + 1) * 64]), 0)                               # breaks rules 1 and 2
    assert device.check_points(put(good[False], i, both), 257) == (i, ug.UG_POINT_UNREDUCED)


def test_upload_chunk_boundary(device, twist):
    """the staging chunk is 8 MiB (StagedUploader::CHUNK): 131072 G1 records, 65536 G2 records; the bad point lies in the second chunk"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    n = 131072 + 5
    pts = bytearray(synth.synth_points(device, n, 0x99, g2=False))
    at = 131072 + 2
    pts[at * 64:(at + 1) * 64] = bump_y(bytes(pts[at * 64:(at + 1) * 64]))
    assert device.check_points(bytes(pts), n) == (at, ug.UG_POINT_OFF_CURVE)
    n = 65536 + 3
    pts = bytearray(synth.synth_points(device, n, 0x77, g2=True))
    assert device.check_points(bytes(pts), n, g2=True, level=2) is None
    at = 65536 + 1
    pts[at * 128:(at + 1) * 128] = twist["P"]
    assert device.check_points(bytes(pts), n, g2=True, level=2) == (at, ug.UG_POINT_OFF_SUBGROUP)


# ---- creation switch ------------------------------------------------------------------------------------------------------
def _create(dev, name, *args):
    L = dev._L
    h = C.c_void_p()
    rc = getattr(L, name)(dev._h, *args, C.byref(h))
    if rc != 0:
        assert not h.value                                                 # *out untouched
        return L.ug_last_error().decode()
    L.ug_bases_destroy(h)
    return None


def test_creation_switch(good, twist):
    import ultragroth_amd as ug
    dev = ug.Device(0)
    try:
        L = dev._L
        L.ug_bases_create_tables_g1.argtypes = L.ug_bases_create_tables_g2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        bad1 = put(good[False], 9, bump_y(good[False][9 * 64:10 * 64]))
        bad2 = put(good[True], 11, twist["P"])
        hosts = lambda a, b: (C.c_void_p * 2)(C.cast(C.c_char_p(a), C.c_void_p), C.cast(C.c_char_p(b), C.c_void_p))
        ns, firsts = (C.c_uint64 * 2)(257, 257), (C.c_uint64 * 2)(500, 520)
        calls = [("ug_bases_create_g1", (bad1, 257, 1000), "point 1009: " + T_CURVE),
                 ("ug_bases_create_g2", (bad2, 257, 1000), "point 1011: " + T_SUBGROUP),
                 ("ug_bases_create_tables_g1", (bad1, 257, 70, 16), "point 79: " + T_CURVE),
                 ("ug_bases_create_tables_g2", (bad2, 257, 70, 16), "point 81: " + T_SUBGROUP),
                 ("ug_bases_create_group_g1", (2, hosts(good[False], bad1), ns, firsts, 500, 300, 0), "member 1 point 529: " + T_CURVE)]
        for name, args, _ in calls:                                        # level 0, the default: as today
            assert _create(dev, name, *args) is None, name
        dev.check_on_create(2)
        free = []
        for name, args, msg in calls:
            assert _create(dev, name, *args) == msg, name
            free.append(dev.mem_info()[0])
        for _ in range(2):                                                 # three failing creations in a row leave the free bytes alone
            assert _create(dev, *calls[1][:1], *calls[1][1]) == calls[1][2]
            free.append(dev.mem_info()[0])
        assert len(set(free)) == 1, free
        assert _create(dev, "ug_bases_create_g2", good[True], 257, 0) is None      # good sets still create
        dev.check_on_create(1)
        assert _create(dev, "ug_bases_create_g2", bad2, 257, 1000) is None         # level 1 does not look at the subgroup
        dev.check_on_create(0)
        assert _create(dev, "ug_bases_create_g1", bad1, 257, 1000) is None
    finally:
        dev.close()


# ---- provers ---------------------------------------------------------------------------------------------------------------
def sections(zkey):
    """section id -> offset of its payload"""
    out, pos = {}, 12
    for _ in range(struct.unpack_from("<I", zkey, 8)[0]):
        sid, size = struct.unpack_from("<IQ", zkey, pos)
        out.setdefault(sid, pos + 12)
        pos += 12 + size
    return out


def tamper(zkey, section, index, g2=False, rec=None):
    n = 128 if g2 else 64
    at = sections(zkey)[section] + index * n
    return zkey[:at] + (rec if rec is not None else bump_y(zkey[at:at + n])) + zkey[at + n:]


def _read(*path):
    return open(os.path.join(GOLDEN, *path), "rb").read()


def _fails(fn, text):
    import ultragroth_amd as ug
    with pytest.raises(ug.ProverError) as e:
        fn()
    assert e.value.code == ug.PROVER_ERROR and e.value.message == text, e.value.message


def _every_way(cls, one_shot, bad, wtns, text):
    """create, the one-shot call, Registry.load and zkey_check refuse the key with the same message"""
    import ultragroth_amd as ug
    _fails(lambda: cls(bad), text)
    _fails(lambda: one_shot(bad, wtns), text)
    with ug.Registry(0) as reg:
        _fails(lambda: reg.load("bad", bad), text)
    got = ug.zkey_check(bad)
    assert got is not None and got[3] == text


def test_clean_keys_prove_the_same(device, zkey, wtns, monkeypatch):
    import ultragroth_amd as ug
    r, s = fixed_rs()
    keys = [(ug.Groth16Prover, zkey, wtns, r + s), (ug.Groth16Prover, _read("trapdoor", "groth16.zkey"), _read("trapdoor", "groth16.wtns"), r + s),
            (ug.UltraGrothProver, _read("trapdoor", "ultra.zkey"), _read("trapdoor", "ultra.uwtns"), s + r + s)]
    for cls, zk, wt, blind in keys:
        got = []
        for level in (None, "2"):
            if level:
                monkeypatch.setenv("ULTRAGROTH_VALIDATE", level)
            else:
                monkeypatch.delenv("ULTRAGROTH_VALIDATE", raising=False)
            p = cls(zk)
            ug.set_test_blinding(blind)
            try:
                got.append(p.prove(wt))
            finally:
                ug.set_test_blinding(b"")
                p.close()
        assert got[0] == got[1]
        assert ug.zkey_check(zk) is None


def test_tampered_groth16_sections(device, zkey, wtns, monkeypatch):
    import ultragroth_amd as ug
    for section, index, g2 in ((5, 3, False), (6, 700, False), (7, 5, True), (8, 11, False), (9, 1023, False)):
        bad = tamper(zkey, section, index, g2)
        monkeypatch.delenv("ULTRAGROTH_VALIDATE", raising=False)
        ug.Groth16Prover(bad).close()                                      # the default has not moved
        monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
        _every_way(ug.Groth16Prover, ug.groth16_prover, bad, wtns, "zkey: section %d point %d: %s" % (section, index, T_CURVE))
    at = sections(zkey)[2] + 84 + 128                                      # beta2, behind alpha1 and beta1
    bad = zkey[:at] + bump_y(zkey[at:at + 128]) + zkey[at + 128:]
    _every_way(ug.Groth16Prover, ug.groth16_prover, bad, wtns, "zkey: header point beta2: " + T_CURVE)
    assert ug.zkey_check(bad)[:3] == (2, 2, ug.UG_POINT_OFF_CURVE)
    bad = tamper(zkey, 3, 1)                                               # IC: no prover uploads it, the standalone check reads it
    ug.Groth16Prover(bad).close()
    assert ug.zkey_check(bad) == (3, 1, ug.UG_POINT_OFF_CURVE, "zkey: section 3 point 1: " + T_CURVE)
    with pytest.raises(ug.ProverError):
        ug.zkey_check(zkey[:len(zkey) // 2])                               # unparsable: the loaders' message, no fault


def test_tampered_ultragroth_sections(device, monkeypatch):
    import ultragroth_amd as ug
    zk, wt = _read("trapdoor", "ultra.zkey"), _read("trapdoor", "ultra.uwtns")
    for section in (8, 9, 12):
        bad = tamper(zk, section, 1)
        monkeypatch.delenv("ULTRAGROTH_VALIDATE", raising=False)
        ug.UltraGrothProver(bad).close()
        monkeypatch.setenv("ULTRAGROTH_VALIDATE", "2")
        _every_way(ug.UltraGrothProver, ug.ultra_groth_prover, bad, wt, "zkey: section %d point 1: %s" % (section, T_CURVE))


def test_b2_point_outside_the_subgroup(device, zkey, twist, monkeypatch):
    import ultragroth_amd as ug
    bad = tamper(zkey, 7, 17, True, twist["P"])
    for level in ("0", "1"):
        monkeypatch.setenv("ULTRAGROTH_VALIDATE", level)
        ug.Groth16Prover(bad).close()
    assert ug.zkey_check(bad, level=1) is None
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "2")
    _fails(lambda: ug.Groth16Prover(bad), "zkey: section 7 point 17: " + T_SUBGROUP)
    assert ug.zkey_check(bad, level=2) == (7, 17, ug.UG_POINT_OFF_SUBGROUP, "zkey: section 7 point 17: " + T_SUBGROUP)


def _real_behind_infinity(zk, section, rec, lo=1000, hi=3000):
    """index of a real point of the section that has at least 100 points at infinity before it: in a compacted set it sits at a
    position at least 100 lower, so a message with this index cannot come from the compacted position"""
    off = sections(zk)[section]
    real = [any(zk[off + i * rec:off + (i + 1) * rec]) for i in range(hi)]
    i = next(i for i in range(lo, hi) if real[i])
    assert real[:i].count(False) >= 100
    return i


def test_sparse_b_reports_the_zkey_index(device, monkeypatch):
    """circuits of >= 2^14 signals with many B points at infinity keep B1 / B2 compacted (sparse B): nVars = 2^15 - 1 here. The clean
    key shows the third schedule group that only the sparse form has; the tampered key names the index in the zkey section, which
    differs from the compacted position by the infinities before it, and the dense form (ULTRAGROTH_SPARSE_B=0) says the same."""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zk, _, info = synth.build_circuit(device, 15, b_zero=0.5)
    zk = bytes(zk)
    assert info["nVars"] >= 1 << 14
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    for sparse, groups in (("1", 3), ("0", 2)):
        monkeypatch.setenv("ULTRAGROTH_SPARSE_B", sparse)
        with ug.Groth16Prover(zk) as p:
            assert len(p.table_plan()) == groups                            # the compacted sets have a schedule group of their own
    i = _real_behind_infinity(zk, 7, 128)
    for sparse in ("1", "0"):
        monkeypatch.setenv("ULTRAGROTH_SPARSE_B", sparse)
        _fails(lambda: ug.Groth16Prover(tamper(zk, 7, i, True)), "zkey: section 7 point %d: %s" % (i, T_CURVE))
        _fails(lambda: ug.Groth16Prover(tamper(zk, 6, i)), "zkey: section 6 point %d: %s" % (i, T_CURVE))
        _fails(lambda: ug.Groth16Prover(tamper(zk, 8, i)), "zkey: section 8 point %d: %s" % (i, T_CURVE))      # C rides in the [A | C] group


def test_sparse_b_ultragroth_reports_the_zkey_index(device, monkeypatch):
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zk, _, info = synth.build_ultra_circuit(device, 15, b_zero=0.5)
    zk = bytes(zk)
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    i = _real_behind_infinity(zk, 7, 128)
    for sparse in ("1", "0"):
        monkeypatch.setenv("ULTRAGROTH_SPARSE_B", sparse)
        ug.UltraGrothProver(zk).close()
        _fails(lambda: ug.UltraGrothProver(tamper(zk, 7, i, True)), "zkey: section 7 point %d: %s" % (i, T_CURVE))
        _fails(lambda: ug.UltraGrothProver(tamper(zk, 6, i)), "zkey: section 6 point %d: %s" % (i, T_CURVE))
        _fails(lambda: ug.UltraGrothProver(tamper(zk, 5, i)), "zkey: section 5 point %d: %s" % (i, T_CURVE))


def test_sharded_slices_report_section_indices(device, monkeypatch):
    """two ranks on one device, the bad point in rank 1's slice of A: the index is the section's, not the slice's"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    log_domain, world = 12, 2
    nv, n_dom = (1 << log_domain) - 1, 1 << log_domain
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    rg = [ug.ShardedGroth16Prover.shard_ranges(nv, 1, n_dom, k, world) for k in range(world)]
    header, coefs, slices = synth.build_circuit_slices(device, log_domain, rg[0])
    ug.ShardedGroth16Prover.from_slices(header, coefs, 4 * n_dom, slices, 0, 0, world, public_size=86).close()
    header, coefs, slices = synth.build_circuit_slices(device, log_domain, rg[1])
    assert rg[1][0][0] > 0 and rg[1][2][0] > 0
    a = bytes(slices[0])
    bad_a = (C.c_char * len(a)).from_buffer_copy(put(a, 5, bump_y(a[5 * 64:6 * 64])))
    _fails(lambda: ug.ShardedGroth16Prover.from_slices(header, coefs, 4 * n_dom, (bad_a,) + tuple(slices[1:]), 0, 1, world, public_size=86),
           "zkey: section 5 point %d: %s" % (rg[1][0][0] + 5, T_CURVE))
    h = bytes(slices[4])
    bad_h = (C.c_char * len(h)).from_buffer_copy(put(h, 7, bump_y(h[7 * 64:8 * 64])))
    _fails(lambda: ug.ShardedGroth16Prover.from_slices(header, coefs, 4 * n_dom, tuple(slices[:4]) + (bad_h,), 0, 1, world, public_size=86),
           "zkey: section 9 point %d: %s" % (rg[1][2][0] + 7, T_CURVE))


# ---- the other ways in --------------------------------------------------------------------------------------------------------
def test_ultragroth_header_points(device, monkeypatch):
    """round_delta1 / round_delta2 sit between gamma2 and delta1 in an UltraGroth header (96 bytes of sizes and counts, then the points)"""
    import ultragroth_amd as ug
    zk = _read("trapdoor", "ultra.zkey")
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    base = sections(zk)[2] + 96 + 64 + 64 + 128 + 128
    for name, at, n, which in (("round_delta1", base, 64, 6), ("round_delta2", base + 64, 128, 7), ("delta1", base + 192, 64, 4)):
        bad = zk[:at] + bump_y(zk[at:at + n]) + zk[at + n:]
        text = "zkey: header point %s: %s" % (name, T_CURVE)
        _fails(lambda: ug.UltraGrothProver(bad), text)
        assert ug.zkey_check(bad) == (2, which, ug.UG_POINT_OFF_CURVE, text)


def test_one_shot_from_a_file(device, zkey, wtns, tmp_path, monkeypatch):
    import ultragroth_amd as ug
    L = ug.load()
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    for name, fn, zk, wt, size in (("g.zkey", L.groth16_prover_zkey_file, zkey, wtns, 810),
                                   ("u.zkey", L.ultra_groth_prover_zkey_file, _read("trapdoor", "ultra.zkey"), _read("trapdoor", "ultra.uwtns"), 1400)):
        path = str(tmp_path / name)
        open(path, "wb").write(tamper(zk, 5, 2))
        psz, qsz = C.c_ulonglong(size), C.c_ulonglong(1 << 16)
        proof, pub, err = C.create_string_buffer(size), C.create_string_buffer(1 << 16), C.create_string_buffer(256)
        assert fn(path.encode(), wt, len(wt), proof, C.byref(psz), pub, C.byref(qsz), err, 255) == ug.PROVER_ERROR
        assert err.value.decode() == "zkey: section 5 point 2: " + T_CURVE


def test_many_device_prover(device, zkey, monkeypatch):
    """ULTRAGROTH_DEVICES: two ranks on the one device behind groth16_prover_create; a bad point of the second rank's range is named by
    its place in the section"""
    import ultragroth_amd as ug
    n_vars = struct.unpack_from("<I", zkey, sections(zkey)[2] + 72)[0]
    monkeypatch.setenv("ULTRAGROTH_DEVICES", "0,0")
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "2")
    ug.Groth16Prover(zkey).close()
    for section, index, g2 in ((5, n_vars - 3, False), (7, n_vars - 2, True), (9, 1022, False)):
        _fails(lambda: ug.Groth16Prover(tamper(zkey, section, index, g2)), "zkey: section %d point %d: %s" % (section, index, T_CURVE))


def test_registry_reload_checks_again(device, zkey, wtns, tmp_path, monkeypatch):
    """a circuit that came from a file and was evicted returns by itself with the next proof: that load is checked too"""
    import ultragroth_amd as ug
    monkeypatch.setenv("ULTRAGROTH_TABLES", "0")
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "1")
    paths = [str(tmp_path / n) for n in ("one.zkey", "two.zkey")]
    for p in paths:
        open(p, "wb").write(zkey)
    with ug.Registry(0) as reg:
        reg.load_file(paths[0])
        core = reg.info("one")[0]
    with ug.Registry(0, int(core * 1.5)) as reg:
        reg.load_file(paths[0])
        reg.load_file(paths[1])
        assert reg.info("one")[1] == ug.Registry.EVICTED
        open(paths[0], "wb").write(tamper(zkey, 9, 4))                      # the file changes under the registry
        _fails(lambda: reg.prove("one", wtns), "zkey: section 9 point 4: " + T_CURVE)
        assert reg.prove("two", wtns)[0]


def test_refused_creates_leave_the_device_as_it_was(device, zkey, twist, monkeypatch):
    """free device bytes after a first refused create == after the third, for every place a key can be bad in"""
    import ultragroth_amd as ug
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "2")
    at = sections(zkey)[2] + 84
    bads = [tamper(zkey, 5, 0), tamper(zkey, 7, 9, True, twist["P"]), tamper(zkey, 9, 1000), zkey[:at] + bump_y(zkey[at:at + 64]) + zkey[at + 64:]]
    for bad in bads:
        free = []
        for _ in range(3):
            with pytest.raises(ug.ProverError):
                ug.Groth16Prover(bad)
            free.append(device.mem_info()[0])
        assert len(set(free)) == 1, free


def test_unknown_setting_is_refused(device, zkey, monkeypatch):
    import ultragroth_amd as ug
    for value in ("3", "on", "2 "):
        monkeypatch.setenv("ULTRAGROTH_VALIDATE", value)
        with pytest.raises(ug.ProverError, match="ULTRAGROTH_VALIDATE must be 0, 1 or 2"):
            ug.Groth16Prover(zkey)
    monkeypatch.setenv("ULTRAGROTH_VALIDATE", "0")
    ug.Groth16Prover(zkey).close()


def test_key_without_section_3(device, zkey):
    """no prover reads IC, so a key without it is a key: the standalone check takes it as well"""
    import ultragroth_amd as ug
    n = struct.unpack_from("<I", zkey, 8)[0]
    out, pos = b"", 12
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", zkey, pos)
        if sid != 3:
            out += zkey[pos:pos + 12 + size]
        pos += 12 + size
    stripped = zkey[:8] + struct.pack("<I", n - 1) + out
    ug.Groth16Prover(stripped).close()
    assert ug.zkey_check(stripped) is None
    assert ug.zkey_check(tamper(stripped, 8, 3))[:3] == (8, 3, ug.UG_POINT_OFF_CURVE)


def test_last_fault_accessor(good):
    """ug_ctx_last_point_fault: the numbers behind the creation's message, cleared by the next creation"""
    import ultragroth_amd as ug
    dev = ug.Device(0)
    try:
        L = dev._L
        dev.check_on_create(1)
        bad = put(good[False], 9, bump_y(good[False][9 * 64:10 * 64]))
        f, m = ug._PointFault(), C.c_int(7)
        assert _create(dev, "ug_bases_create_g1", bad, 257, 1000) == "point 1009: " + T_CURVE
        assert L.ug_ctx_last_point_fault(dev._h, C.byref(m), C.byref(f)) == 0 and (m.value, f.index, f.reason) == (-1, 1009, ug.UG_POINT_OFF_CURVE)
        assert L.ug_point_reason_text(f.reason).decode() == T_CURVE
        assert _create(dev, "ug_bases_create_g1", good[False], 257, 1000) is None
        assert L.ug_ctx_last_point_fault(dev._h, C.byref(m), C.byref(f)) == 0 and f.reason == ug.UG_POINT_OK
    finally:
        dev.close()
