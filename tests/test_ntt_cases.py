"""The builders of tests/ntt_cases.py against the CPU oracle, on the host: every closed form equals the oracle's transform (a radix-2
transform of another family than a closed form: the two are independent), three outputs per vector also equal the O(n) sum of the
definition, the unreduced twins are what they claim, and the two-record H polynomial equals the oracle's. The device tests
(test_gpu_ntt_shapes.py) take their expected values from here, so a mistake in a closed form shows up in this file first."""
import pytest

import ntt_cases as NC
import oracle as O

R = NC.R
SIZES = [1, 3, 6, 11]


def test_constants_are_the_oracles():
    assert NC.R == O.R_MOD and NC.MONT == O.MONT_R % O.R_MOD
    for logn in (1, 2, 11, 20, 28):
        assert NC.omega(logn) * NC.MONT % R == O.root_of_unity(logn)           # (the oracle's root is in Montgomery form)
    assert all(v >= R for v in NC.UNREDUCED) and all(v < 1 << 256 for v in NC.UNREDUCED) and all(v < R for v in NC.EDGES)
    assert len(NC.FAMILIES) == 7 and NC.C_VALUES == (1, R - 1, (1 << 256) % R)


def _spots(logn):
    n = 1 << logn
    return sorted({0, n // 2, n - 1, (5 * n) // 7})[:3] if n > 2 else [0, 1]


@pytest.mark.parametrize("name", NC.FAMILIES)
@pytest.mark.parametrize("logn", SIZES)
def test_family_equals_oracle_and_definition(logn, name):
    cases = NC.family(logn, name)
    assert cases
    for case in cases:
        data = case.data
        assert len(data) == 32 << logn and all(v < R for v in NC.to_ints(data))
        for inverse in (False, True):
            out = O.ntt(data, logn, inverse=inverse)
            assert case.holds(out, inverse), (case, inverse)
            exp = case.expected(inverse)
            assert (exp is None) == (name == "geometric")
            if logn <= 6 or case is cases[0]:                                  # (the sum is O(n) per output)
                for k in _spots(logn):
                    assert NC.definition_sum(data, logn, k, inverse) == O.from_le(out[32 * k:32 * k + 32]), (case, inverse, k)
    NC.forget_tables()


@pytest.mark.parametrize("logn", SIZES)
def test_family_places_and_counts(logn):
    """deltas and frequencies at 0, 1, n / 2, n - 1, and above 2^10 at the border of the first pass's tile"""
    n = 1 << logn
    assert set(NC.delta_places(logn)) >= {0, 1, n // 2, n - 1}
    assert set(NC.frequencies(logn)) >= {0, 1, n // 2, n - 1}
    if logn > 10:
        assert set(NC.delta_places(logn)) >= {1023, 1024, n - 1024} and 1024 in NC.frequencies(logn)
    assert len(NC.all_cases(logn)) == 1 + 3 + 3 * len(NC.delta_places(logn)) + 3 * len(NC.frequencies(logn)) + 3 + 3 + 1


def test_product_form_rejects_a_wrong_word():
    """the geometric check bites: one word off by one, one word plus r (not canonical), and a sampled check at that place"""
    logn = 6
    case = NC.family(logn, "geometric")[1]
    out = O.ntt(case.data, logn)
    assert case.holds(out, False) and case.holds(out, False, places=[0, 17, 63])
    for bad in ((O.from_le(out[32 * 17:32 * 18]) + 1) % R, O.from_le(out[32 * 17:32 * 18]) + R):
        wrong = out[:32 * 17] + O.to_le(bad) + out[32 * 18:]
        assert not case.holds(wrong, False) and not case.holds(wrong, False, places=[17])
        assert case.holds(wrong, False, places=[16, 18])
    assert not case.holds(out, True)


def test_geometric_at_2_19():
    """the size of the three-pass transform (10 + 5 + 4): input from Python integers, the product form over the whole vector"""
    logn = 19
    case = NC.family(logn, "geometric")[2]
    data = case.data
    for inverse in (False, True):
        out = O.ntt(data, logn, inverse=inverse)
        assert case.holds(out, inverse)
        for k in ((0, 1 << 18, (1 << 19) - 1) if not inverse else (12345,)):
            assert NC.definition_sum(data, logn, k, inverse) == O.from_le(out[32 * k:32 * k + 32])
    assert set(NC.sample_places(20)) >= set(range(0, 1 << 20, 64)) and len(NC.sample_places(20)) > (1 << 14) + 4000


@pytest.mark.parametrize("logn", SIZES)
def test_unreduced_twins(logn):
    """a twin holds the same residues, every word of it is r .. 4r above the reduced word, all four multiples occur (two at n = 2,
    the other two with another shift), and the oracle transforms it to the same bytes"""
    for t, case in enumerate(NC.all_cases(logn)):
        data = case.data
        tw = NC.twin(data, shift=t)
        a, b = NC.to_ints(data), NC.to_ints(tw)
        assert all(y < 1 << 256 and y >= R and (y - x) % R == 0 and R <= y - x <= 4 * R for x, y in zip(a, b))
        assert NC.reduce_words(tw) == data
        seen = {(y - x) // R for x, y in zip(a, b)} | {(y - x) // R for x, y in zip(a, NC.to_ints(NC.twin(data, shift=t + 2)))}
        assert seen == {1, 2, 3, 4}
        for inverse in (False, True):
            assert O.ntt(tw, logn, inverse=inverse) == O.ntt(data, logn, inverse=inverse), (case, inverse)
    NC.forget_tables()


@pytest.mark.parametrize("logn", [0, 1, 4, 10, 11, 12])
def test_spliced_random_vectors(logn):
    n = 1 << logn
    data, reduced = NC.spliced_random(logn)
    assert len(data) == len(reduced) == 32 * n and NC.reduce_words(data) == reduced
    vals = NC.to_ints(data)
    places = NC.splice_places(logn)
    assert {0, n - 1} <= set(places) and (logn <= 10 or {1023, 1024} <= set(places))
    if logn >= 10:
        assert any(v >= R for v in vals) and {0, R - 1} <= set(vals)
        assert sum(1 for p in places if vals[p] >= R or vals[p] in NC.EDGES) == len(places)
    for inverse in (False, True):
        assert O.ntt(data, logn, inverse=inverse) == O.ntt(reduced, logn, inverse=inverse)


def test_add_multiples_carries():
    words = [0, 1, (1 << 64) - 1, (1 << 128) - 1, (1 << 192) - 1, R - 1, (1 << 256) - 4 * R - 1]
    for k in range(5):
        assert NC.to_ints(NC.add_multiples(NC.to_words(words), [k] * len(words))) == [w + k * R for w in words]
    with pytest.raises(AssertionError):
        NC.add_multiples(NC.to_words([(1 << 256) - 4 * R]), [4])


@pytest.mark.parametrize("logn,ra,rb", [(3, 2, 2), (3, 1, 6), (11, 5, 5), (11, 0, 2047), (19, 77, 77), (20, (1 << 20) - 1, 12345)])
def test_hpoly_closed_form_equals_oracle(logn, ra, rb):
    coefs, ncoefs, w, nvars, exp = NC.hpoly_case(logn, ra, rb)
    assert len(coefs) == 44 * ncoefs
    got = O.hpoly(coefs, ncoefs, w, nvars, 1 << logn)
    assert got == exp
    assert any(exp[:32]) and all(v < R for v in NC.to_ints(exp[:32 * 64]))
    if logn <= 3:                    # the same h from the oracle's single steps: ifft, twist, fft of the two delta vectors
        n = 1 << logn
        a = NC.HPOLY_ALPHA * NC.HPOLY_WITNESS[2] % R
        b = NC.HPOLY_BETA * NC.HPOLY_WITNESS[3] % R
        w2n = NC.omega(logn + 1)

        def coset(v, row):
            x = NC.to_ints(O.ntt(NC._one_place(logn, row, v), logn, inverse=True))
            return NC.to_ints(O.ntt(NC.to_words(c * pow(w2n, i, R) % R for i, c in enumerate(x)), logn))
        ea, eb, ec = coset(a, ra), coset(b, rb), coset(a * b % R if ra == rb else 0, ra)
        assert NC.to_ints(exp) == [(x * y - z) % R for x, y, z in zip(ea, eb, ec)]
    NC.forget_tables()
