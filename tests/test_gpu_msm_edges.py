"""The prover's multi-scalar multiplication at the edges of its branches, byte for byte against the CPU oracle (builders and their
host checks: msm_edge_cases.py, test_msm_edge_cases.py):

  A  digit edges      csrc/sort.hip recode_scalar: a scalar family that takes every branch of the signed-digit recoding in every
                      window -- on window tables of every width 16 .. 24 (strided too), on classic windows forced to the widths
                      5, 15 (pair form), 16 (fused, runtime width), 20 and 22 (compile-time widths), over several scalar vectors
                      (the reciprocal that splits an index into vector and element) and with bucket classes
  B  tail classes     csrc/msm.hip: buckets cut by the 32-entry segments into exactly 1, 2, 32 | 33, 65, 4096 | 4097 and 5121
                      pieces: whole, fix-up, medium and heavy buckets at the borders between the paths, a last task of one piece,
                      two heavy buckets in one schedule
  C  exceptional sums runs of equal, opposite and infinity records inside a segment (G1 and the group kernel), tails whose pieces
                      are all equal (every addition doubles) or cancel (sums pass through infinity), a running sum of the bucket
                      reduction that meets its equal or its negative, one point read from two different tables

One distinct point per scalar in A (a wrong bucket, sign or table changes the sum); points that cycle over five records in B, so
that the oracle multiplies five points (msm_edge_cases.collapse). Every schedule runs on window tables and on classic windows."""
import functools
import os
import random
import subprocess
import sys

import pytest

import oracle as O
import msm_edge_cases as MC
from test_gpu_parity import _class_tilings

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [16, 0]                 # table_c: window tables of width 16, classic windows
MAX_WINDOWS = 43                # of a classic schedule: the cost model's narrowest window has 6 bits
SEG_LIMIT = 1 << 26             # entries from which the segments grow beyond 32 (msm_edge_cases.one_digit)
GROUPS = [False, True]          # g2


@pytest.fixture(scope="module")
def g1_points(zkey):
    """the fixture's H section: 64-byte records, all distinct finite points"""
    off, sz = O.section(zkey, "zkey", 9)
    recs = MC.finite_records(zkey[off:off + sz], 64)
    assert len(recs) >= 1000
    return recs


@pytest.fixture(scope="module")
def g2_points(zkey):
    """the fixture's B2 section without its infinity records"""
    off, sz = O.section(zkey, "zkey", 7)
    recs = MC.finite_records(zkey[off:off + sz], 128)
    assert len(recs) > 900
    return recs


@pytest.fixture(scope="module")
def points(g1_points, g2_points):
    return {False: g1_points, True: g2_points}


def _msm(device, recs, vals, table_c, g2=False):
    """the product over a list of records and a list of integers"""
    assert len(recs) == len(vals)
    return (device.msm_g2 if g2 else device.msm_g1)(b"".join(recs), MC.scalar_bytes(vals), len(vals), table_c=table_c)


_family_cache = {}


def _family_case(pts, c, g2=False):
    """(point bytes, scalar bytes, n, the oracle's product) of the family of width c on the first n points; computed once"""
    key = (c, g2)
    if key not in _family_cache:
        fam = _family(c)
        n = len(fam)
        assert n <= len(pts)
        pb, sb = b"".join(pts[:n]), MC.scalar_bytes(fam)
        _family_cache[key] = (pb, sb, n, (O.g2_msm if g2 else O.g1_msm)(pb, sb, n))
    return _family_cache[key]


@functools.lru_cache(maxsize=None)
def _family(c):
    """width 0 (classic windows at the cost model's width, 7 or 8 bits for this count): the families of the narrow widths and of 16
    -- more than 661 scalars, from which on the model leaves its narrowest window (43 digits per scalar: three vectors of them
    do not fit one result block) for 37 digits or fewer"""
    if c:
        return MC.digit_family(c)
    fam = MC.digit_family(7) + MC.digit_family(8) + MC.digit_family(9) + MC.digit_family(16)
    assert 661 < len(fam) < 1000
    return fam


# ------------------------------------------------------------------------------------------- A. digit edges
@pytest.mark.parametrize("c", range(16, 25))
def test_digit_family_on_window_tables_g1(device, g1_points, c):
    pb, sb, n, exp = _family_case(g1_points, c)
    assert device.msm_g1(pb, sb, n, table_c=c) == exp != MC.G1_INF
    if c in (16, 20, 22):
        v = device.dvec(n, sb)
        for stride in (2, MC.window_count(c)):             # two bucket sets; one set per window, every table the point itself
            b = device.bases(pb, n, table_c=c, table_stride=stride)
            assert device.msm(b, device.schedule(v, 0, n, table_c=c, table_stride=stride)) == exp, stride


@pytest.mark.parametrize("c", [16, 22])
def test_digit_family_on_window_tables_g2(device, g2_points, c):
    pb, sb, n, exp = _family_case(g2_points, c, g2=True)
    assert device.msm_g2(pb, sb, n, table_c=c) == exp != MC.G2_INF


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import ultragroth_amd as ug
pts, sc = open(sys.argv[2], "rb").read(), open(sys.argv[3], "rb").read()
d = ug.Device(0)
fn = d.msm_g2 if sys.argv[4] == "g2" else d.msm_g1
print("result", fn(pts, sc, len(sc) // 32).hex())
d.close()
"""


@pytest.mark.parametrize("c,g2", [(5, False), (15, False), (16, False), (20, False), (22, False), (15, True), (22, True)])
def test_digit_family_on_forced_classic_windows(points, tmp_path, c, g2):
    """UG_MSM_C = c: 5 -- 51 windows, and 5 divides 255: the top window has full width -- and 15 -- 17 windows, the widest -- take the
    pair form (digit_pairs_kernel); 16 is the first fused width (CW = 0); 20 and 22 are the compile-time instantiations of the
    histogram and of the first pass, which the cost model reaches only from 2^20 scalars on. The library reads the knob once
    per process, so each width runs in a process of its own, with that width's own family."""
    pb, sb, n, exp = _family_case(points[g2], c, g2)
    pf, sf = tmp_path / "points.bin", tmp_path / "scalars.bin"
    pf.write_bytes(pb)
    sf.write_bytes(sb)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(pf), str(sf), "g2" if g2 else "g1"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, UG_MSM_C=str(c)))
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("result ")]
    assert got == [exp.hex()]


@pytest.mark.parametrize("table_c", [0, 16, 20, 22])
def test_digit_family_over_three_vectors(device, g1_points, table_c):
    """vector 0 zeros, vector 1 the family, vector 2 the family reversed, with a gap between the vectors: record v is the product
    of vector v"""
    fam = _family(table_c)
    count, gap = len(fam), 77
    assert 3 * MC.window_count(7) <= 127                    # (classic: the result block holds the window sets of all vectors)
    vecs = [[0] * count, list(fam), list(reversed(fam))]
    pb = b"".join(g1_points[:count])
    exp = [O.g1_msm(pb, MC.scalar_bytes(v), count) for v in vecs]
    assert exp[0] == MC.G1_INF and len(set(exp)) == 3
    dv = device.dvec(3 * (count + gap), b"".join(MC.scalar_bytes(v) + bytes(32 * gap) for v in vecs))
    sch = device.schedule_vectors(dv, 0, count, 3, count + gap, table_c=table_c)
    got = device.msm(device.bases(pb, count, table_c=table_c), sch)
    assert [got[64 * v:64 * (v + 1)] for v in range(3)] == exp


@pytest.mark.parametrize("V", [2, 16])
@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_vector_counts_around_a_power_of_two(device, g1_points, count, V):
    """index -> (vector, element) by a multiply-high reciprocal of the count: a count of 1, a power of two and both sides of it.
    Vector v holds the `count` scalars of the family, each value once, from position v on (the first ones: the small values,
    r - 1, the digits of window 0), so no two vectors have the same product"""
    fam, gap = list(dict.fromkeys(MC.digit_family(16))), 77
    vecs = [list(fam[v:v + count]) for v in range(V)]
    pb = b"".join(g1_points[:count])
    exp = [O.g1_msm(pb, MC.scalar_bytes(v), count) for v in vecs]
    assert len(set(exp)) == V
    dv = device.dvec(V * (count + gap), b"".join(MC.scalar_bytes(v) + bytes(32 * gap) for v in vecs))
    sch = device.schedule_vectors(dv, 0, count, V, count + gap, table_c=16)
    got = device.msm(device.bases(pb, count, table_c=16), sch)
    assert [got[64 * v:64 * (v + 1)] for v in range(V)] == exp


@pytest.mark.parametrize("table_c,q_log,parts,specials", [(16, 3, 8, 16), (20, 6, 4, 1)])
def test_class_border_digits_add_up(device, g1_points, table_c, q_log, parts, specials):
    """bucket classes: single digits on the borders of the classes -- the last special bucket and the first regular ones, a residue
    that wraps, the last two buckets of the set -- in every window, over uneven tilings of the residues and of the scalars: the
    products of the classes add up to the oracle's product"""
    vals = MC.single_digits(table_c, MC.class_digits(table_c, q_log, specials))
    n = len(vals)
    pb, sb = b"".join(g1_points[:n]), MC.scalar_bytes(vals)
    exp = O.g1_msm(pb, sb, n)
    b, v = device.bases(pb, n, table_c=table_c), device.dvec(n, sb)
    rng = random.Random(100 * table_c + q_log)
    for _ in range(2):
        res, sp = _class_tilings(rng, q_log, parts, n)
        acc = MC.G1_INF
        for (r0, r1), (s0, s1) in zip(res, sp):
            sch = device.schedule(v, 0, n, table_c=table_c, classes=(q_log, r0, r1 - r0, specials, s0, s1 - s0))
            acc = O.g1_add(acc, device.msm(b, sch))
        assert acc == exp != MC.G1_INF, (res, sp)


# ------------------------------------------------------------------------------------------- B. tail classes
def _run_schedule(device, five, spec, wants, table_c, g2):
    scalars, layout = MC.one_digit(spec)
    n = len(scalars)
    assert {v: layout[v][2] for v in wants} == wants          # the boundaries are there by construction
    assert n * MAX_WINDOWS < SEG_LIMIT and all(0 < s < 32 for s in scalars)
    exp = MC.oracle_msm(*MC.collapse_cycled(five, scalars), g2)
    fn = device.msm_g2 if g2 else device.msm_g1
    assert fn(MC.cycled_bytes(five, n), MC.scalar_bytes(scalars), n, table_c=table_c) == exp != bytes(len(exp))


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("filler", [0, 1, 31])
@pytest.mark.parametrize("g2", GROUPS)
def test_whole_fixup_and_medium_buckets_at_their_borders(device, points, g2, filler, table_c):
    """buckets of exactly 1, 2, 32 | 33 and 65 pieces behind a leading bucket of 0, 1 or 31 entries"""
    spec, wants = MC.small_schedule(filler)
    _run_schedule(device, points[g2][:5], spec, wants, table_c, g2)


@pytest.mark.parametrize("table_c", MODES)
def test_medium_and_heavy_bucket_at_their_border(device, g1_points, table_c):
    """4096 pieces (one wave) beside 4097 (five tasks, the last of one piece)"""
    spec, wants = MC.medium_heavy_schedule()
    _run_schedule(device, g1_points[:5], spec, wants, table_c, False)


@pytest.mark.parametrize("table_c", MODES)
def test_two_heavy_buckets(device, g1_points, table_c):
    """five and six tasks: a task finds its bucket by a search over the task offsets"""
    spec, wants = MC.two_heavy_schedule()
    _run_schedule(device, g1_points[5:10], spec, wants, table_c, False)


@pytest.mark.parametrize("table_c", MODES)
def test_heavy_bucket_g2(device, g2_points, table_c):
    """the heavy path with G2's workgroup of 128 lanes"""
    spec, wants = MC.heavy_alone_schedule()
    _run_schedule(device, g2_points[:5], spec, wants, table_c, True)


# ------------------------------------------------------------------------------------------- C. exceptional additions
@pytest.mark.parametrize("table_c", MODES)
def test_exceptional_branches_inside_one_segment_g1(device, g1_points, table_c):
    """segment_accumulate_kernel<G1Cfg> (accumulator in registers, records prefetched): P, P | P, -P, Q | infinity, R | infinity,
    infinity | zero scalars, each inside the first segment; the whole case and each case alone"""
    recs, vals = MC.exceptional_cases(g1_points, 3000)
    assert [v for v in vals if 0 < v < 5] == [1, 1, 2, 2, 2, 3, 3, 4, 4] and vals[:9] == [1, 1, 2, 2, 2, 3, 3, 4, 4] and 9 < MC.SEG
    assert recs[0] == recs[1] != MC.G1_INF and recs[3] == MC.neg(recs[2]) and recs[4] not in (recs[2], recs[3], MC.G1_INF)
    assert recs[5] == MC.G1_INF != recs[6] and recs[7] == recs[8] == MC.G1_INF
    assert _msm(device, recs, vals, table_c) == MC.oracle_msm(recs, vals)
    for (lo, hi), exp in zip(MC.EXCEPTIONAL_SLICES, MC.exceptional_expected(recs, vals)):
        assert _msm(device, recs[lo:hi], vals[lo:hi], table_c) == exp, (lo, hi)


@pytest.mark.parametrize("table_c", MODES)
def test_exceptional_branches_in_the_group_kernel(device, g1_points, table_c):
    """segment_accumulate_group_kernel<3>: at the same entries member 0 doubles, member 1 passes through infinity and member 2
    reads infinity records -- and the other way round in the next bucket; the two-member form on the first two"""
    members, vals = MC.group_case(g1_points, 500)
    n = len(vals)
    exp = [MC.oracle_msm(m, vals) for m in members]
    v = device.dvec(n, MC.scalar_bytes(vals))
    sch = device.schedule(v, 0, n, table_c=table_c)
    grp = device.bases_group([(b"".join(m), n, 0) for m in members], 0, n, table_c=table_c)
    assert device.msm_group(grp, sch) == exp
    pair = device.bases_group([(b"".join(m), n, 0) for m in members[:2]], 0, n, table_c=table_c)
    assert device.msm_group(pair, sch) == exp[:2]
    # the six entries alone: every other bucket empty
    head = device.bases_group([(b"".join(m[:6]), 6, 0) for m in members], 0, 6, table_c=table_c)
    exp6 = [MC.oracle_msm(m[:6], vals[:6]) for m in members]
    assert device.msm_group(head, device.schedule(device.dvec(6, MC.scalar_bytes(vals[:6])), 0, 6, table_c=table_c)) == exp6


TAIL_CASES = [(False, 2), (False, 33), (False, 65), (False, 4097), (True, 2), (True, 33), (True, 65)]


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("g2,k", TAIL_CASES)
def test_equal_pieces_double_in_every_tail(device, points, g2, k, table_c):
    """one bucket of k equal pieces: fix-up, medium, medium with two strides, heavy -- every addition of the fix-up loop, of the wave
    butterfly and of the workgroup tree takes the doubling branch"""
    P = points[g2][11]
    recs, vals, mult = MC.equal_pieces_case(P, k)
    n = len(vals)
    assert MC.pieces(0, n) == k and n * MAX_WINDOWS < SEG_LIMIT
    fn = device.msm_g2 if g2 else device.msm_g1
    assert fn(P * n, MC.scalar_bytes(vals), n, table_c=table_c) == MC.oracle_mul(P, mult, g2)


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("g2,k", TAIL_CASES)
def test_cancelling_pieces_pass_through_infinity(device, points, g2, k, table_c):
    """pieces that alternate between 32 P and -32 P: infinity for an even number of them, 32 v P for an odd one"""
    P = points[g2][12]
    recs, vals, mult = MC.cancelling_case(P, k)
    assert MC.pieces(0, len(vals)) == k
    exp = MC.oracle_mul(P, mult, g2) if mult else bytes(len(P))
    assert (exp == bytes(len(P))) == (k % 2 == 0)
    assert _msm(device, recs, vals, table_c, g2) == exp


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("g2", GROUPS)
def test_fixup_goes_on_after_infinity(device, points, g2, table_c):
    P, Q = points[g2][13], points[g2][14]
    recs, vals, mult = MC.cancel_then_point_case(P, Q)
    assert MC.pieces(0, len(vals)) == 3
    assert _msm(device, recs, vals, table_c, g2) == MC.oracle_mul(Q, mult, g2)


@pytest.mark.parametrize("table_c", MODES)
@pytest.mark.parametrize("g2", GROUPS)
def test_bucket_reduction_meets_its_equal_and_its_negative(device, points, g2, table_c):
    """bucket_chunk_reduce_kernel: the running sum returns to infinity, doubles, leaves a chunk with a weight offset as infinity
    below a chunk that is not empty, and the weighted sum meets the negative of the running sum"""
    P, Q = points[g2][15], points[g2][16]
    add = O.g2_add if g2 else O.g1_add
    for name, (recs, vals) in MC.reduction_cases(P, Q).items():
        a, b = MC.REDUCTION_EXPECTED[name]
        exp = add(MC.oracle_mul(P, a, g2), MC.oracle_mul(Q, b, g2) if b else bytes(len(P)))
        assert MC.oracle_msm(recs, vals, g2) == exp
        assert _msm(device, recs, vals, table_c, g2) == exp, name


@pytest.mark.parametrize("d", [1, 1234, 1 << 15])
def test_same_point_read_from_two_tables(device, g1_points, d):
    """Q = 2^16 P beside P, scalars d 2^16 on P and d on Q: bucket d - 1 holds the same coordinates twice, once from table 1 of P
    and once from table 0 of Q, so the mixed addition must double. Expected 2 d 2^16 P"""
    P = g1_points[17]
    Q = O.g1_mul(P, 1 << 16)
    exp = O.g1_mul(P, 2 * d << 16)
    assert MC.oracle_msm([P, Q], [d << 16, d]) == exp
    assert _msm(device, [P, Q], [d << 16, d], 16) == exp
    assert _msm(device, [Q, P], [d, d << 16], 16) == exp
