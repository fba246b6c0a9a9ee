"""Shared case builders of the MSM edge tests (test_msm_edge_cases.py checks the builders on the host, test_gpu_msm_edges.py runs
them on the device). Every comparison in those files is byte for byte against the CPU oracle. The builders are pure Python:

  recode / digit_family    a plain restatement of the signed-digit recoding of csrc/sort.hip (recode_scalar) and, per window
                           width, a scalar family that takes every branch of it in every window
  pieces / one_digit       one-digit scalars whose buckets are cut by the 32-entry segments of the accumulation into a KNOWN number
                           of pieces: the tail paths of csrc/msm.hip (fix-up 2 .. 32, medium 33 .. 4096, heavy above, tasks of 1024)
                           at their class boundaries
  collapse                 the oracle's input for a product whose points repeat: one scalar per distinct record
  the *_case builders      runs of equal, opposite and infinity records for the exceptional branches of the additions

Every builder is deterministic and cached where it is shared."""
import functools
import random

import oracle as O

R = O.R_MOD
SEG = 32                       # entries per segment of a small schedule (see one_digit)
FIX_MAX, MEDIUM_MAX, HEAVY_TASK = 32, 4096, 1024          # msm.hip: the piece counts at which the tail path changes
BRANCHES = ("zero", "pos", "pos_half", "neg", "neg_max", "zero_carry")
G1_INF, G2_INF = bytes(64), bytes(128)


def window_count(c):
    return (255 + c - 1) // c


# ------------------------------------------------------------------------------------------- recoding
def recode(s, c):
    """Signed-digit recoding of s mod r for window width c: W = ceil(255 / c) digits in (-2^(c-1), 2^(c-1)], a raw window value
    above half becomes raw - 2^c with a carry into the next window. Returns (digits, branch names, carry out of the top window).
    Branches: zero | pos | pos_half (raw == half, the last bucket of a set) | neg | neg_max (raw == half + 1, the digit -(half - 1))
    | zero_carry (raw == 2^c: all ones and a carry in -- magnitude 0, carry out)."""
    s %= R
    half, full = 1 << (c - 1), 1 << c
    digits, names, carry = [], [], 0
    for w in range(window_count(c)):
        raw = ((s >> (c * w)) & (full - 1)) + carry
        if raw > half:
            d, carry = raw - full, 1
            names.append("zero_carry" if d == 0 else "neg_max" if d == -(half - 1) else "neg")
        else:
            d, carry = raw, 0
            names.append("zero" if d == 0 else "pos_half" if d == half else "pos")
        digits.append(d)
    return digits, names, carry


@functools.lru_cache(maxsize=None)
def digit_family(c):
    """Scalars that take every branch of recode in every window of width c (the top window only ever holds a small positive
    digit, and window 0 has no carry in: both follow from r < 2^254). Values >= r are part of it: the device reduces them."""
    W, half, full = window_count(c), 1 << (c - 1), 1 << c
    top = c * (W - 1)
    out = [0, 1, 2, R - 1, R - 2]
    for w in range(W):
        out += [d << (c * w) for d in (1, half - 1, half, half + 1, full - 1) if (d << (c * w)) < R]
    # -1 in window 0, zero-with-carry in windows 1 .. w, +1 above
    out += [(1 << (c * (w + 1))) - 1 for w in range(W) if (1 << (c * (w + 1))) - 1 < R]
    cut = (1 << 253) - 1
    for even, odd in ((half, half), (half + 1, half + 1), (half, half + 1), (full - 1, half)):
        out.append(sum((odd if w & 1 else even) << (c * w) for w in range(W)) & cut)
    fullest = (R >> top) << top                      # the fullest top window a scalar below r allows: alone, and with a carry in
    out += [fullest, fullest - 1]
    out += [k * R + e for k in range(1, 6) for e in (0, 1, (half + 1) << c) if k * R + e < 1 << 256]
    out += [(1 << 256) - 1, 1 << 255]
    assert all(0 <= s < 1 << 256 for s in out)
    return tuple(out)


def family_coverage(c):
    """per window: the set of branch names the family of width c reaches"""
    seen = [set() for _ in range(window_count(c))]
    for s in digit_family(c):
        for w, name in enumerate(recode(s, c)[1]):
            seen[w].add(name)
    return seen


def expected_coverage(c):
    W = window_count(c)
    return [set(BRANCHES) - {"zero_carry"}] + [set(BRANCHES)] * (W - 2) + [{"zero", "pos"}]


def single_digits(c, digits):
    """d * 2^(c w) for every window w and every d of `digits`, kept when below r"""
    return tuple(d << (c * w) for w in range(window_count(c)) for d in digits if 0 < d << (c * w) < R)


def class_digits(c, q_log, specials):
    """the digits around the borders of a schedule with bucket classes: the last special bucket and the first regular ones, a
    residue wrap, the last two buckets of the set"""
    half = 1 << (c - 1)
    return (1, specials, specials + 1, specials + 2, 1 << q_log, (1 << q_log) + 1, half - 1, half)


# ------------------------------------------------------------------------------------------- tails
def pieces(start, count, seg=SEG):
    """segments that hold the entries [start, start + count) of the sorted list: the pieces the accumulation cuts a bucket into"""
    return (start + count - 1) // seg - start // seg + 1


def one_digit(spec):
    """spec: (value, count) pairs, value in 1 .. 31, every value at most once. Returns (scalars, layout): `count` scalars equal to
    `value` for every pair, in the order given, and layout[value] = (start, count, pieces) of the bucket of that value.

    A scalar below 2^(c-1) has ONE non-zero digit, in window 0, whatever the window width c >= 6 is (tables: 16 .. 24; classic:
    the cost model's choice among 6 .. 22). So the schedule holds one entry per scalar, the entry of `value` goes to bucket
    value - 1, the buckets follow each other in the sorted list (index order inside a bucket: the partition is stable), and
    segments have 32 entries: segment_log (msm.hip) stays at 5 while n * windows < 2^26 with the default UG_SEG_LANES_LOG = 20 --
    a longer segment needs 2^20 lanes of twice the length. A test that uses this builder asserts n * windows < 2^26."""
    assert len({v for v, _ in spec}) == len(spec) and all(1 <= v <= 31 and n >= 0 for v, n in spec)
    scalars = [v for v, n in spec for _ in range(n)]
    layout, start = {}, 0
    for v, n in sorted(spec):
        layout[v] = (start, n, pieces(start, n) if n else 0)
        start += n
    return scalars, layout


def count_for(start, want, extra=0):
    """the entry count that makes a bucket beginning at `start` exactly `want` pieces: its last entry is entry `extra` (0 .. 31) of
    the last segment; a one-piece bucket has up to three entries and ends inside its segment"""
    if want == 1:
        return min(3, SEG - start % SEG)
    n = (start // SEG + want - 1) * SEG - start + 1 + extra
    assert 0 <= extra < SEG and pieces(start, n) == want
    return n


def boundary_spec(first_value, start, wants, extra=7):
    """(value, count) pairs for consecutive values from first_value whose buckets, laid out from entry `start`, have the piece
    counts `wants`"""
    spec = []
    for k, want in enumerate(wants):
        n = count_for(start, want, extra)
        spec.append((first_value + k, n))
        start += n
    return spec


def small_schedule(filler):
    """a leading bucket of `filler` entries (0, 1 or 31: three alignments of what follows), then buckets of exactly 1, 2, 32, 33
    and 65 pieces: whole, fix-up least and most, medium least, medium with lanes that stride twice"""
    spec = ([(1, filler)] if filler else []) + boundary_spec(2, filler, (1, 2, FIX_MAX, FIX_MAX + 1, 65))
    return spec, {2: 1, 3: 2, 4: FIX_MAX, 5: FIX_MAX + 1, 6: 65}


def medium_heavy_schedule():
    """the widest medium bucket and the narrowest heavy one -- 4096 and 4097 pieces, five tasks with a last task of ONE piece --
    with a whole bucket, a fix-up bucket and a small medium one around them"""
    wants = (1, 3, MEDIUM_MAX, 2, MEDIUM_MAX + 1, 40, 1)
    return boundary_spec(3, 0, wants), dict(zip(range(3, 10), wants))


def two_heavy_schedule():
    """two heavy buckets of five and six tasks (4097 and 5121 = 5 * 1024 + 1 pieces) with a medium and a fix-up bucket between them:
    the task -> bucket search of heavy_partial_kernel has two buckets to tell apart"""
    wants = (2, MEDIUM_MAX + 1, 50, 7, 5 * HEAVY_TASK + 1, 1)
    return boundary_spec(5, 0, wants), dict(zip(range(5, 11), wants))


def heavy_alone_schedule():
    return boundary_spec(9, 0, (MEDIUM_MAX + 1,), extra=0), {9: MEDIUM_MAX + 1}


def heavy_tasks(n_pieces):
    return (n_pieces + HEAVY_TASK - 1) // HEAVY_TASK


# ------------------------------------------------------------------------------------------- points
def neg(rec):
    """-P of a finite record, G1 (x, y) or G2 (x.a, x.b, y.a, y.b): Montgomery form, so q - v negates"""
    h = len(rec) // 2
    assert len(rec) in (64, 128) and any(rec)
    return rec[:h] + b"".join(O.to_le((O.Q_MOD - O.from_le(rec[k:k + 32])) % O.Q_MOD) for k in range(h, len(rec), 32))


def finite_records(buf, size):
    """the distinct finite records of a zkey section, in order"""
    recs = [bytes(buf[k:k + size]) for k in range(0, len(buf) - size + 1, size)]
    recs = [r for r in recs if any(r)]
    assert len(set(recs)) == len(recs)
    return recs


def cycle(recs, n, start=0):
    return [recs[(start + i) % len(recs)] for i in range(n)]


def cycled_bytes(recs, n):
    """b"".join(cycle(recs, n)) without building n objects"""
    block = b"".join(recs)
    return (block * (n // len(recs) + 1))[:len(recs[0]) * n]


def scalar_bytes(scalars):
    return b"".join(O.to_le(s) for s in scalars)


def collapse(records, scalars):
    """(distinct records in order of first use, the sum of the scalars of each mod r): the same product over far fewer points. A
    record and its negative are two records; infinity records are dropped (they add nothing)."""
    sums = {}
    for rec, s in zip(records, scalars):
        if any(rec):
            sums[rec] = (sums.get(rec, 0) + s) % R
    return list(sums), list(sums.values())


def collapse_cycled(recs, scalars):
    """collapse(cycle(recs, n), scalars) for long inputs"""
    k = len(recs)
    assert len(set(recs)) == k and all(any(r) for r in recs)
    return list(recs), [sum(scalars[j::k]) % R for j in range(k)]


def oracle_msm(records, scalars, g2=False):
    if not records:
        return G2_INF if g2 else G1_INF
    return (O.g2_msm if g2 else O.g1_msm)(b"".join(records), scalar_bytes(scalars), len(records))


def oracle_mul(rec, k, g2=False):
    """k * P through the oracle's product over one point (k any integer: reduced mod r)"""
    return oracle_msm([rec], [k % R], g2)


# ------------------------------------------------------------------------------------------- exceptional additions
def exceptional_cases(points, filler, seed=None):
    """points and one-digit scalars whose first buckets hold, in this order and each inside the first segment:
         bucket of 1:  P, P            the doubling branch
         bucket of 2:  P, -P, Q        infinity in the middle of a run, then the first point again
         bucket of 3:  infinity, R     a run that begins with a point-at-infinity record
         bucket of 4:  infinity x 2    a run that never leaves infinity: the bucket is written as infinity
       then eight scalars that are zero (no entry at all), then `filler` scalars of 5 .. 7: three long buckets cut many times.
       (either group: the infinity record has the size of the points)"""
    P, Q, Rr, S = points[3], points[4], points[5], points[6]
    inf = bytes(len(P))
    recs = [P, P, P, neg(P), Q, inf, Rr, inf, inf] + [S] * 8
    vals = [1, 1, 2, 2, 2, 3, 3, 4, 4] + [0] * 8
    rng = random.Random(filler if seed is None else seed)
    recs += cycle(points, filler, start=10)
    vals += [rng.randrange(5, 8) for _ in range(filler)]
    return recs, vals


EXCEPTIONAL_SLICES = ((0, 2), (2, 5), (5, 7), (7, 9), (9, 17))       # each case of exceptional_cases alone


def exceptional_expected(recs, vals, g2=False):
    """what each case alone is built to give: 2P, 2Q, 3R, infinity, infinity"""
    inf = bytes(len(recs[0]))
    return [oracle_mul(recs[0], 2, g2), oracle_mul(recs[4], 2, g2), oracle_mul(recs[6], 3, g2), inf, inf]


def group_case(points, filler):
    """three members over the same one-digit scalars: at the indices 0 .. 2 (one bucket, inside the first segment) member 0 holds
    P, P, S (a doubling), member 1 P, -P, Q (through infinity), member 2 infinity records; then the indices 3 .. 5 of a second
    bucket with the cases moved on by one member; then `filler` entries of 5 .. 7 with other points in every member"""
    P, Q, S = points[3], points[4], points[5]
    inf = bytes(len(P))
    a, b, c = [P, P, S], [P, neg(P), Q], [inf, inf, inf]
    members = [a + c + cycle(points, filler, 10), b + a + cycle(points, filler, 20), c + b + cycle(points, filler, 30)]
    rng = random.Random(filler)
    vals = [1, 1, 1, 2, 2, 2] + [rng.randrange(5, 8) for _ in range(filler)]
    return members, vals


def equal_pieces_case(P, k, v=3):
    """one bucket of 32 k copies of P (scalar v each): k equal pieces 32 P, every addition of the tail doubles. Expected (32 k v) P"""
    n = SEG * k
    return [P] * n, [v] * n, n * v


def cancelling_case(P, k, v=3):
    """the same bucket with segments that alternate between 32 copies of P and 32 of -P: neighbouring pieces cancel. Expected
    infinity for even k, (32 v) P for odd k"""
    m = neg(P)
    recs = [P if (i // SEG) % 2 == 0 else m for i in range(SEG * k)]
    return recs, [v] * (SEG * k), (SEG * v if k % 2 else 0)


def cancel_then_point_case(P, Q, v=3):
    """32 P, 32 -P, 32 Q in one bucket: the fix-up passes through infinity and goes on. Expected (32 v) Q"""
    return [P] * SEG + [neg(P)] * SEG + [Q] * SEG, [v] * (3 * SEG), SEG * v


def reduction_cases(P, Q):
    """one-digit scalars that steer the running sum of bucket_chunk_reduce_kernel (buckets from the top of a chunk down; chunks of
    8 or more buckets, so the buckets 8 .. 15 share a chunk whose weight offset is not zero). name -> (records, scalars):
         returns     P in bucket 10, -P in bucket 9: `run` meets its negative and returns to infinity          (= P)
         doubles     P in the buckets 10 and 9: `run` meets its equal                                          (= 21 P)
         empty_sum   P in bucket 12, -P in bucket 10 and Q in bucket 20: a chunk whose buckets sum to infinity (its offset
                     multiplies infinity) below a chunk that is not empty                                      (= 2 P + 21 Q)
         acc_cancel  -P in bucket 11, P in bucket 10 twice: acc = -P meets run = P                             (= 10 P)"""
    m = neg(P)
    return {
        "returns": ([P, m], [11, 10]),
        "doubles": ([P, P], [11, 10]),
        "empty_sum": ([P, m, Q], [13, 11, 21]),
        "acc_cancel": ([m, P, P], [12, 11, 11]),
    }


REDUCTION_EXPECTED = {"returns": (1, 0), "doubles": (21, 0), "empty_sum": (2, 21), "acc_cancel": (10, 0)}     # multiples of P, Q
