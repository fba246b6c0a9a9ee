"""ug_points_check_mask on the device (check.hip, the mask form): one status byte per record, for every record. The reference
reasons are computed here with oracle/pairing.py arithmetic from the raw records, rule by rule in the order of DESIGN.md section 5.5;
about ten distinct points per curve are replicated to fill n."""
import pytest

from oracle import pairing as PR
from test_gpu_validate import Q, R, MONT, g1_rec, g2_rec, coords, bump_y, unreduced, f2_sqrt, g2_mul

pytestmark = pytest.mark.gpu

OK, UNREDUCED, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3
MONT_INV = pow(MONT, -1, Q)
_cache = {}


def reason(rec, g2, level):
    """the first rule a raw zkey record breaks"""
    key = (rec, level)
    if key in _cache:
        return _cache[key]
    cs = coords(rec)
    if not any(cs):
        out = OK
    elif any(c >= Q for c in cs):
        out = UNREDUCED
    else:
        v = [c * MONT_INV % Q for c in cs]
        if not g2:
            out = OK if (v[1] * v[1] - v[0] ** 3 - 3) % Q == 0 else OFF_CURVE
        else:
            p = ((v[0], v[1]), (v[2], v[3]))
            if not PR.g2_on_curve(p):
                out = OFF_CURVE
            else:
                out = OFF_SUBGROUP if level == 2 and g2_mul(p, R) is not None else OK
    _cache[key] = out
    return out


@pytest.fixture(scope="module")
def points():
    """per curve: the good points that fill a buffer and one bad point per reason"""
    from ultragroth_amd.synth import G2_GEN
    assert PR.g2_on_curve(G2_GEN) and g2_mul(G2_GEN, R) is None
    g = (1, 2)
    good1 = [g1_rec(PR.g1_mul(g, k)) for k in (1, 2, 3, 5, 7)] + [bytes(64)]
    small1 = next(r for r in good1 if any(r) and coords(r)[0] + Q < MONT)
    bad1 = {UNREDUCED: unreduced(small1, 0), OFF_CURVE: bump_y(good1[1])}
    b2 = PR.f2_muls(PR.f2_inv(PR.XI), 3)
    x = (1, 0)
    y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), b2))
    P = (x, y)                                                                    # on the twist, outside the subgroup
    S = g2_mul(P, 2 * Q - R)                                                      # in the subgroup
    good2 = [g2_rec(g2_mul(G2_GEN, k)) for k in (1, 2, 3)] + [g2_rec(S), bytes(128)]
    small2 = next(r for r in good2 if any(r) and coords(r)[3] + Q < MONT)
    bad2 = {UNREDUCED: unreduced(small2, 3), OFF_CURVE: bump_y(good2[0]), OFF_SUBGROUP: g2_rec(P)}
    for g2, good, bad in ((False, good1, bad1), (True, good2, bad2)):
        assert all(reason(r, g2, 2) == OK for r in good) and all(reason(r, g2, 2) == why for why, r in bad.items())
    return {False: (good1, bad1), True: (good2, bad2)}


def build(points, g2, n, at):
    """n records of good points with one bad point of each kind at the positions `at` that exist (the kinds rotate with n)"""
    good, bad = points[g2]
    recs = [good[i % len(good)] for i in range(n)]
    kinds = sorted(bad)
    for j, pos in enumerate(sorted({p for p in at if 0 <= p < n})):
        recs[pos] = bad[kinds[(j + n) % len(kinds)]]
    return recs


def lowest(expect):
    return next(((i, why) for i, why in enumerate(expect) if why), None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("g2", [False, True])
def test_mask_equals_the_reference(device, points, g2, level, n):
    recs = build(points, g2, n, (0, 63, 64, n - 1))
    expect = bytes(reason(r, g2, level) for r in recs)
    buf = b"".join(recs)
    assert device.points_check_mask(buf, n, g2=g2, level=level) == expect
    assert device.check_points(buf, n, g2=g2, level=level) == lowest(expect)
    assert any(expect) and (n < 65 or len(set(expect)) >= 3)


def test_every_reason_at_every_marked_position(device, points):
    """n = 129 under every rotation of the kinds: each reason has sat at 0, 63, 64 and n - 1"""
    good, bad = points[True]
    kinds = sorted(bad)
    for shift in range(len(kinds)):
        recs = [good[i % len(good)] for i in range(129)]
        for j, pos in enumerate((0, 63, 64, 128)):
            recs[pos] = bad[kinds[(j + shift) % len(kinds)]]
        expect = bytes(reason(r, True, 2) for r in recs)
        assert device.points_check_mask(b"".join(recs), 129, g2=True, level=2) == expect
        assert device.check_points(b"".join(recs), 129, g2=True, level=2) == (0, kinds[shift])


def test_every_point_off_the_subgroup(device, points):
    """what ug_points_check needs 129 calls for"""
    P = points[True][1][OFF_SUBGROUP]
    assert device.points_check_mask(P * 129, 129, g2=True, level=2) == bytes([OFF_SUBGROUP]) * 129
    assert device.points_check_mask(P * 129, 129, g2=True, level=1) == bytes(129)
    assert device.check_points(P * 129, 129, g2=True, level=2) == (0, OFF_SUBGROUP)


def test_across_a_staging_piece(device, points):
    """64 MiB of G2 records are 2^19: the bad points sit on both sides of the piece boundary and at the very end"""
    good, bad = points[True]
    n = (1 << 19) + 3
    block = b"".join(good)
    buf = bytearray((block * (n // len(good) + 1))[:n * 128])
    expect = bytearray((bytes(reason(r, True, 1) for r in good) * (n // len(good) + 1))[:n])
    for pos, why in (((1 << 19) - 1, OFF_CURVE), (1 << 19, UNREDUCED), (n - 1, OFF_CURVE)):
        buf[pos * 128:(pos + 1) * 128] = bad[why]
        expect[pos] = why
    got = device.points_check_mask(bytes(buf), n, g2=True, level=1)
    assert got == bytes(expect) and [i for i, v in enumerate(got) if v] == [(1 << 19) - 1, 1 << 19, n - 1]


def test_empty_and_bad_arguments(device):
    import ultragroth_amd as ug
    assert device.points_check_mask(b"", 0) == b""
    with pytest.raises(ug.DeviceError):
        device.points_check_mask(bytes(64), 1, level=3)
