"""G2 bucket accumulation with the accumulator's zz / zzz parked in LDS (msm.hip, TailLds): the G2 products of the ug_* entry
points against the CPU oracle at the sizes and inputs where the parked state could go wrong -- partial waves and lanes that
leave before they touch LDS, exactly one workgroup and one segment more, buckets cut by segment boundaries, and runs that take
every exceptional branch of the mixed addition. Every case runs on window tables and on classic windows.

Small schedules have segments of 32 entries (segment_log), a workgroup of the accumulation has 256 lanes: 8 192 entries fill one.
A scalar below 2^(c-1) has ONE non-zero digit, in window 0, whatever the window width c >= 6 is (tables: 16; classic: the cost
model's choice among 6 .. 22), so a test that gives every scalar a value in 1 .. 31 knows its entries: one per scalar, bucket
`value - 1`, in index order inside the bucket (the partition is stable), the buckets one after the other in the sorted list.
"""
import os
import random
import subprocess
import sys

import pytest

import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 32                      # entries per lane of a small schedule
WORKGROUP = 256 * SEG         # entries of one full workgroup
MODES = [16, 0]               # table_c: window tables of width 16, classic windows
INF = bytes(128)              # the point at infinity as a zkey record


@pytest.fixture(scope="module")
def g2_points(zkey):
    """the fixture's B2 section without its infinity records: 128-byte records, all distinct finite points"""
    off, sz = O.section(zkey, "zkey", 7)
    recs = [zkey[off + 128 * i:off + 128 * (i + 1)] for i in range(sz // 128)]
    recs = [r for r in recs if r != INF]
    assert len(set(recs)) == len(recs) and len(recs) > 900
    return recs


def _neg(rec):
    """-P of a finite G2 record (x.a, x.b, y.a, y.b; Montgomery form, so q - v negates)"""
    ya, yb = O.from_le(rec[64:96]), O.from_le(rec[96:128])
    return rec[:64] + O.to_le((O.Q_MOD - ya) % O.Q_MOD) + O.to_le((O.Q_MOD - yb) % O.Q_MOD)


def _cycle(recs, n, start=0):
    return [recs[(start + i) % len(recs)] for i in range(n)]


def _msm(device, recs, vals, table_c):
    assert len(recs) == len(vals)
    return device.msm_g2(b"".join(recs), b"".join(O.to_le(v) for v in vals), len(vals), table_c=table_c)


def _oracle(recs, vals):
    return O.g2_msm(b"".join(recs), b"".join(O.to_le(v) for v in vals), len(vals))


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_partial_waves(device, g2_points, n, table_c):
    """a handful of segments: most lanes of the only workgroup return before they touch the LDS area. Uniform scalars (every
    window has a digit) and one-digit scalars (n entries: 1, 63 and 65 of them are two or three segments)"""
    rng = random.Random(100 * n + table_c)
    recs = _cycle(g2_points, n, start=n)
    for vals in ([rng.randrange(O.R_MOD) for _ in range(n)], [rng.randrange(1, 32) for _ in range(n)]):
        assert _msm(device, recs, vals, table_c) == _oracle(recs, vals)


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("entries", [WORKGROUP, WORKGROUP + SEG])
def test_one_workgroup_and_one_segment_more(device, g2_points, entries, table_c):
    """one entry per scalar: exactly 256 full segments, and 257 -- a second workgroup with one busy lane. Thirty-one buckets of
    about 265 entries: each is cut by eight or nine segment boundaries (start-cut, end-cut and whole-segment runs, slot_pts)"""
    rng = random.Random(entries + table_c)
    vals = [rng.randrange(1, 32) for _ in range(entries)]
    assert all(0 < v < 32 for v in vals) and len(vals) % SEG == 0
    recs = _cycle(g2_points, entries)
    assert _msm(device, recs, vals, table_c) == _oracle(recs, vals)


def _exceptional_cases(g2_points, filler):
    """points and one-digit scalars whose first buckets hold, in this order and each inside the first segment:
         bucket of 1:  P, P            the doubling branch
         bucket of 2:  P, -P, Q        infinity in the middle of a run, then xyzz_from_affine
         bucket of 3:  infinity, R     a run that begins with a point-at-infinity record
         bucket of 4:  infinity x 2    a run that never leaves infinity: the bucket is written as infinity
       then eight scalars that are zero (no entry at all), then `filler` scalars of 5 .. 7: three long buckets cut many times"""
    P, Q, R, S = g2_points[3], g2_points[4], g2_points[5], g2_points[6]
    recs = [P, P, P, _neg(P), Q, INF, R, INF, INF] + [S] * 8
    vals = [1, 1, 2, 2, 2, 3, 3, 4, 4] + [0] * 8
    rng = random.Random(filler)
    recs += _cycle(g2_points, filler, start=10)
    vals += [rng.randrange(5, 8) for _ in range(filler)]
    return recs, vals


@pytest.mark.parametrize("table_c", MODES)
def test_exceptional_branches_inside_one_segment(device, g2_points, table_c):
    recs, vals = _exceptional_cases(g2_points, 3000)
    # the cases are there by construction: the nine entries of the buckets of 1 .. 4 are the first nine of the sorted list, i.e.
    # one lane's, and no other scalar shares those buckets
    assert [v for v in vals if 0 < v < 5] == [1, 1, 2, 2, 2, 3, 3, 4, 4] and vals[:9] == [1, 1, 2, 2, 2, 3, 3, 4, 4] and 9 < SEG
    assert recs[0] == recs[1] != INF                                      # P twice in a row
    assert recs[3] == _neg(recs[2]) and recs[4] not in (recs[2], recs[3], INF)
    assert recs[5] == INF != recs[6] and recs[7] == recs[8] == INF
    assert vals[9:17] == [0] * 8 and all(5 <= v <= 7 for v in vals[17:])
    assert _msm(device, recs, vals, table_c) == _oracle(recs, vals)
    # each case alone (other buckets empty): 2P, Q, R, infinity, infinity
    assert _msm(device, recs[:2], vals[:2], table_c) == _oracle(recs[:2], vals[:2]) != INF
    mid = _msm(device, recs[2:5], vals[2:5], table_c)
    assert mid == _oracle(recs[2:5], vals[2:5]) == O.g2_msm(recs[4], O.to_le(2), 1)
    assert _msm(device, recs[5:7], vals[5:7], table_c) == O.g2_msm(recs[6], O.to_le(3), 1)
    assert _msm(device, recs[7:9], vals[7:9], table_c) == INF
    assert _msm(device, recs[9:17], vals[9:17], table_c) == INF


@pytest.mark.parametrize("table_c", MODES)
def test_uniform_scalars_with_repeats(device, g2_points, table_c):
    """every window busy: 2 000 uniform scalars, among them neighbours with the same point and scalar (a doubling in every
    window) and with P, -P (infinity in every window), infinity records and zero scalars"""
    rng = random.Random(77 + table_c)
    n = 2000
    recs, vals = _cycle(g2_points, n), [rng.randrange(O.R_MOD) for _ in range(n)]
    for i in range(40, n - 1, 97):
        recs[i + 1], vals[i + 1] = recs[i], vals[i]
    for i in range(60, n - 1, 131):
        recs[i + 1], vals[i + 1] = _neg(recs[i]), vals[i]
    for i in range(5, n, 211):
        recs[i] = INF
    for i in range(300, 340):
        vals[i] = 0
    assert _msm(device, recs, vals, table_c) == _oracle(recs, vals)


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import ultragroth_amd as ug
pts, sc = open(sys.argv[2], "rb").read(), open(sys.argv[3], "rb").read()
d = ug.Device(0)
print("result", d.msm_g2(pts, sc, len(sc) // 32).hex())
d.close()
"""


def test_forced_narrow_classic_window(g2_points, tmp_path):
    """UG_MSM_C=4: 64 windows of 8 buckets, about 375 entries per bucket -- every bucket is cut by a dozen segment boundaries,
    most lanes hold one whole-segment run. The library reads the knob once per process, so this product runs in a process of
    its own. Same repeats as above: with four-bit windows a repeated (point, scalar) doubles in every one of the 64 windows."""
    rng = random.Random(4)
    recs, vals = _exceptional_cases(g2_points, 0)          # (values 0 .. 4: one digit at this width too)
    n = 3000
    recs += _cycle(g2_points, n, start=50)
    vals += [rng.randrange(O.R_MOD) for _ in range(n)]
    for i in range(40, len(recs) - 1, 97):
        recs[i + 1], vals[i + 1] = recs[i], vals[i]
    for i in range(60, len(recs) - 1, 131):
        recs[i + 1], vals[i + 1] = _neg(recs[i]), vals[i]
    pf, sf = tmp_path / "points.bin", tmp_path / "scalars.bin"
    pf.write_bytes(b"".join(recs))
    sf.write_bytes(b"".join(O.to_le(v) for v in vals))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(pf), str(sf)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, UG_MSM_C="4"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("result ")]
    assert got == [_oracle(recs, vals).hex()]
