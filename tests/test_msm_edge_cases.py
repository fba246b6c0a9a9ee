"""The case builders of the MSM edge tests (msm_edge_cases.py), checked on the host: the recoding restated there is a recoding,
the scalar families reach every branch of it in every window of every width the device tests use, the one-digit schedules cut
their buckets into exactly the piece counts the tail paths change at, collapsing repeated points leaves the oracle's product
unchanged, and the oracle alone gives what each exceptional case is built to give. No GPU."""
import random

import pytest

import oracle as O
import msm_edge_cases as MC

R = O.R_MOD
WIDTHS = (5, 15) + tuple(range(16, 25))              # every width test_gpu_msm_edges.py runs: classic 5, 15, 16, 20, 22; tables 16 .. 24
OTHER_WIDTHS = (4, 7, 8, 9)                           # the classic vector schedule's family is made of narrow widths


@pytest.fixture(scope="module")
def g1_points(zkey):
    off, sz = O.section(zkey, "zkey", 9)
    return MC.finite_records(zkey[off:off + sz], 64)


@pytest.fixture(scope="module")
def g2_points(zkey):
    off, sz = O.section(zkey, "zkey", 7)
    return MC.finite_records(zkey[off:off + sz], 128)


@pytest.mark.parametrize("c", WIDTHS + OTHER_WIDTHS)
def test_recode_is_a_recoding_of_every_family_scalar(c):
    half, W = 1 << (c - 1), MC.window_count(c)
    fam = MC.digit_family(c)
    assert 89 <= len(fam) <= 407
    for s in fam + MC.single_digits(c, MC.class_digits(c, 3, 16)):
        digits, names, carry = MC.recode(s, c)
        assert len(digits) == len(names) == W and carry == 0
        assert all(-half < d <= half for d in digits)
        assert sum(d << (c * w) for w, d in enumerate(digits)) % R == s % R
        for d, name in zip(digits, names):
            assert name in MC.BRANCHES
            assert (d == 0) == (name in ("zero", "zero_carry")) and (d < 0) == (name in ("neg", "neg_max"))
            assert (d == half) == (name == "pos_half") and (d == 1 - half) == (name == "neg_max")


@pytest.mark.parametrize("c", WIDTHS + OTHER_WIDTHS)
def test_family_reaches_every_branch_in_every_window(c):
    """every branch in every window, with exactly two exceptions that follow from r < 2^254: the top window only ever takes a small
    positive digit (or none), and no carry comes into window 0"""
    assert MC.family_coverage(c) == MC.expected_coverage(c)


def test_family_holds_the_reduction_edges():
    """scalars >= r: k r + e needs k subtractions, 2^256 - 1 needs five; a carry chain that runs through every window"""
    fam = MC.digit_family(16)
    assert {s // R for s in fam} == {0, 1, 2, 3, 4, 5} and (1 << 256) - 1 in fam and ((1 << 256) - 1) // R == 5
    chain = (1 << (16 * 15)) - 1
    assert chain in fam and MC.recode(chain, 16)[1] == ["neg"] + ["zero_carry"] * 14 + ["pos"]
    fullest = (R >> 240) << 240
    assert MC.recode(fullest - 1, 16)[1][-2:] == ["zero_carry", "pos"] and MC.recode(fullest - 1, 16)[0][-1] == R >> 240


def test_class_digits_sit_on_the_class_borders():
    for c, q_log, specials in ((16, 3, 16), (20, 6, 1)):
        sc = MC.single_digits(c, MC.class_digits(c, q_log, specials))
        W = MC.window_count(c)
        assert len(sc) >= 8 * (W - 1) + 1
        mags = {abs(d) for s in sc for d in MC.recode(s, c)[0] if d}
        assert {1, specials, specials + 1, 1 << q_log, (1 << q_log) + 1, (1 << (c - 1)) - 1, 1 << (c - 1)} <= mags


def test_pieces():
    assert MC.pieces(0, 1) == MC.pieces(0, 32) == MC.pieces(31, 1) == 1
    assert MC.pieces(0, 33) == MC.pieces(31, 2) == 2 and MC.pieces(31, 34) == 3
    for start in (0, 1, 31, 32, 1000):
        for want in (1, 2, 32, 33, 65, 4096, 4097):
            for extra in (0, 7, 31):
                n = MC.count_for(start, want, extra)
                assert MC.pieces(start, n) == want
                brute = len({e // 32 for e in range(start, start + n)}) if n < 5000 else want
                assert brute == want


@pytest.mark.parametrize("filler", [0, 1, 31])
def test_small_schedule_piece_counts(filler):
    spec, wants = MC.small_schedule(filler)
    scalars, layout = MC.one_digit(spec)
    assert {v: layout[v][2] for v in wants} == {2: 1, 3: 2, 4: 32, 5: 33, 6: 65}
    assert layout[2][0] == filler and len(scalars) == sum(n for _, n in spec) < 5000
    assert all(0 < s < 32 for s in scalars)
    # brute force: the segments each value's entries fall into when the entries are laid out bucket after bucket
    order = sorted(scalars)
    for v in wants:
        assert len({i // 32 for i, s in enumerate(order) if s == v}) == wants[v]


def test_large_schedule_piece_counts():
    spec, wants = MC.medium_heavy_schedule()
    scalars, layout = MC.one_digit(spec)
    got = {v: layout[v][2] for v in wants}
    assert got == wants and sorted(got.values())[-2:] == [4096, 4097]
    assert 255_000 < len(scalars) < 270_000
    assert MC.heavy_tasks(4096) == 4 and MC.heavy_tasks(4097) == 5 and 4097 - 4 * MC.HEAVY_TASK == 1        # a last task of one piece
    spec, wants = MC.two_heavy_schedule()
    scalars, layout = MC.one_digit(spec)
    assert {v: layout[v][2] for v in wants} == wants
    heavy = sorted(p for p in wants.values() if p > MC.MEDIUM_MAX)
    assert heavy == [4097, 5121] and [MC.heavy_tasks(p) for p in heavy] == [5, 6]
    between = [wants[v] for v in sorted(wants) if layout[6][0] < layout[v][0] < layout[9][0]]
    assert wants[6] == 4097 and wants[9] == 5121 and between == [50, 7]                                      # a medium and a fix-up bucket between them
    assert 285_000 < len(scalars) < 300_000
    spec, wants = MC.heavy_alone_schedule()
    scalars, layout = MC.one_digit(spec)
    assert layout[9] == (0, 4096 * 32 + 1, 4097) and len(scalars) == 4096 * 32 + 1


def test_collapse_keeps_the_product(g1_points, g2_points):
    """n = 2000 with repeats, negatives, infinity records and scalars >= r: the product over the distinct records equals the
    oracle's product over the full input"""
    n = 2000
    for g2, pts in ((False, g1_points), (True, g2_points)):
        rng = random.Random(41 + g2)
        five = pts[:5]
        pool = five + [MC.neg(five[0]), MC.neg(five[3]), bytes(len(five[0]))]
        recs = [pool[rng.randrange(len(pool))] for _ in range(n)]
        vals = [rng.choice([0, 1, 31, R - 1, R + 5, rng.randrange(R)]) for _ in range(n)]
        full = (O.g2_msm if g2 else O.g1_msm)(b"".join(recs), MC.scalar_bytes(vals), n)
        d_recs, d_vals = MC.collapse(recs, vals)
        assert len(d_recs) == 7 and MC.neg(five[0]) in d_recs and five[0] in d_recs
        assert MC.oracle_msm(d_recs, d_vals, g2) == full != bytes(len(five[0]))
        # the cycled form the long schedules use
        vals = [rng.randrange(1, 32) for _ in range(n)]
        c_recs, c_vals = MC.collapse_cycled(five, vals)
        assert (c_recs, c_vals) == MC.collapse(MC.cycle(five, n), vals)
        assert MC.cycled_bytes(five, n) == b"".join(MC.cycle(five, n))
        assert MC.oracle_msm(c_recs, c_vals, g2) == (O.g2_msm if g2 else O.g1_msm)(MC.cycled_bytes(five, n), MC.scalar_bytes(vals), n)


def test_oracle_on_the_exceptional_cases(g1_points, g2_points):
    for g2, pts in ((False, g1_points), (True, g2_points)):
        inf = bytes(len(pts[0]))
        mul = lambda rec, k: O.g2_mul(rec, k) if g2 else O.g1_mul(rec, k)
        add = O.g2_add if g2 else O.g1_add
        P, Q = pts[3], pts[4]
        assert add(P, MC.neg(P)) == inf and add(P, P) == mul(P, 2) == MC.oracle_mul(P, 2, g2) and MC.neg(MC.neg(P)) == P
        recs, vals = MC.exceptional_cases(pts, 50)
        assert vals[:17] == [1, 1, 2, 2, 2, 3, 3, 4, 4] + [0] * 8 and all(5 <= v <= 7 for v in vals[17:])
        assert recs[0] == recs[1] and recs[3] == MC.neg(recs[2]) and recs[5] == recs[7] == recs[8] == inf
        exp = MC.exceptional_expected(recs, vals, g2)
        assert exp[:3] == [mul(P, 2), mul(Q, 2), mul(pts[5], 3)] and inf not in exp[:3]
        for (lo, hi), e in zip(MC.EXCEPTIONAL_SLICES, exp):
            assert MC.oracle_msm(recs[lo:hi], vals[lo:hi], g2) == e
        for k in (2, 33):
            recs, vals, mult = MC.equal_pieces_case(P, k)
            assert len(recs) == 32 * k and MC.oracle_msm(*MC.collapse(recs, vals), g2) == mul(P, mult) == mul(P, 32 * k * 3)
            recs, vals, mult = MC.cancelling_case(P, k)
            assert recs[:32] == [P] * 32 and recs[32:64] == [MC.neg(P)] * 32
            assert MC.oracle_msm(*MC.collapse(recs, vals), g2) == (mul(P, 96) if k % 2 else inf) and mult == (96 if k % 2 else 0)
        recs, vals, mult = MC.cancel_then_point_case(P, Q)
        assert MC.oracle_msm(*MC.collapse(recs, vals), g2) == mul(Q, mult) == mul(Q, 96)
        for name, (recs, vals) in MC.reduction_cases(P, Q).items():
            a, b = MC.REDUCTION_EXPECTED[name]
            assert all(8 <= v - 1 <= 15 or v == 21 for v in vals)                       # one chunk with a weight offset, one above it
            assert MC.oracle_msm(recs, vals, g2) == add(mul(P, a), mul(Q, b) if b else inf), name
        # a group's members: the cases at the same indices
        members, vals = MC.group_case(pts, 20)
        assert vals[:6] == [1, 1, 1, 2, 2, 2] and all(len(m) == len(vals) for m in members)
        assert members[0][:3] == [P, P, pts[5]] and members[1][:3] == [P, MC.neg(P), Q] and members[2][:3] == [inf] * 3
        assert members[1][3:6] == members[0][:3] and members[2][3:6] == members[1][:3] and members[0][3:6] == [inf] * 3
    # the same point through two tables: Q = 2^16 P
    P = g1_points[7]
    Q = O.g1_mul(P, 1 << 16)
    d = 1234
    assert MC.oracle_msm([P, Q], [d << 16, d]) == O.g1_mul(P, 2 * d << 16)
