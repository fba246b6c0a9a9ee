"""Shared case builders of the phase-2 setup tests (test_setup_ptau_host.py on host threads, test_gpu_setup_ptau.py on the
device). Every comparison in those files is byte for byte. The references are: dev_setup's host path for the trapdoor
(tau, alpha, beta, gamma = 1, delta), which test_setup_host.py pins against Python integers; and, for the two tooling calls, the
CPU oracle's scalar multiplication of a sum computed with Python integers (every test point is k * G for a known k).
Every builder is deterministic and cached, so the two files share one copy, which nobody changes."""
import functools
import random

import r1cs_cases as RC
import setup_cases as SC
from ultragroth_amd import synth

R = SC.R
HALF = (R - 1) // 2
# the issue's list; the two random values have a magnitude of full length (253 bits after the fold at r / 2)
COEFS = (1, R - 1, 2, R - 2, (1 << 16) - 1, 1 << 16, 1 << 253, R - (1 << 253), HALF, HALF + 1,
         0x1d2a4c6e8f0b3d5a79c1e3f507294b6d8fa1c3e507192b4d6f8193a5c7e90b2d, R - 0x1f3b5d7e9a1c3e5f70825a4c6e8091b3d5f7192b3d4f6a8c0e2143658799abcd)
assert all(0 < c < R for c in COEFS) and COEFS[10].bit_length() == 253 and (R - COEFS[11]).bit_length() == 253
COLUMN_COUNTS = (1, 63, 64, 65, 257)
N_POINTS = 24
INF_AT = 5                                      # the base at infinity
FIXED_DELTA = 0x2b1c0d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5a4b3c2d1e0f9a8b7c6d5e4f3a2b1c % R


def trapdoor(delta=1):
    return dict(SC.trapdoor_dict(), gamma="1", delta_final=str(delta))


@functools.lru_cache(maxsize=None)
def ptau(power, prepared=True, device=-1):
    """the synthesized .ptau of the fixture's (tau, alpha, beta); device: where its points are made (the bytes are the same)"""
    t = SC.trapdoor_dict()
    return synth.ptau_file(power, int(t["tau"]), int(t["alpha"]), int(t["beta"]), prepared=prepared, device=device)


@functools.lru_cache(maxsize=None)
def dev_setup_key(r1cs, delta, log_domain):
    """(zkey, vkey) of dev_setup's host path for (tau, alpha, beta, gamma = 1, delta)"""
    import ultragroth_amd as ug
    return ug.dev_setup(r1cs, trapdoor(delta), "groth16", log_domain=log_domain, device=-1)[:2]


def with_sections(data, replace=None, drop=()):
    """the binfile with some sections' payloads replaced ({id: bytes}) or left out"""
    replace = replace or {}
    secs = [(i, replace.get(i, p)) for i, p in RC.sections(data) if i not in drop]
    return RC.binfile(data[:4], 1, secs)


# ------------------------------------------------------------------------------------------- points_combine
@functools.lru_cache(maxsize=None)
def point_scalars():
    rng = random.Random(0xC0B1)
    k = [rng.randrange(1, R) for _ in range(N_POINTS)]
    k[INF_AT] = 0
    k[1] = 1
    return tuple(k)


@functools.lru_cache(maxsize=None)
def points(g2):
    return tuple(SC.oracle_muls(point_scalars(), g2))


def _all_classes(rng):
    """one term per coefficient of the list: every length class in one column; the base at infinity among them"""
    terms = [(rng.randrange(N_POINTS), c) for c in COEFS]
    terms.append((INF_AT, COEFS[rng.randrange(len(COEFS))]))
    return terms


@functools.lru_cache(maxsize=None)
def combine_case(n_cols):
    """(col_ptr, index, coefs) of n_cols columns. Columns 0, 1, 62 .. 65, 126, 127 and 256 -- the first, a middle and the last
    lane of a wave whether a lane takes one column or two -- hold every coefficient of the list; 128 .. 255 hold unit terms only
    (a whole wave of them for either group); 2 .. 125 each hold a term of full length, which makes more than a whole wave of
    full-length products; also: a column whose terms cancel, an empty one, one on the base at infinity alone."""
    rng = random.Random(0xC01 + n_cols)
    cols = []
    for c in range(n_cols):
        if c in (0, 1, 62, 63, 64, 65, 126, 127, 256):
            terms = _all_classes(rng)
        elif 128 <= c < 256:
            terms = [(rng.randrange(N_POINTS), rng.choice((1, R - 1))) for _ in range(1 + c % 3)]
        else:
            full = rng.randrange(1 << 252, HALF)
            terms = [(rng.randrange(N_POINTS), rng.choice((full, R - full)))]
            terms += [(rng.randrange(N_POINTS), rng.choice(COEFS)) for _ in range(c % 4)]
        cols.append(terms)
    special = {3: [(2, 7), (2, R - 7), (4, 1), (4, R - 1)],              # cancels to the neutral element
               4: [],                                                    # empty
               5: [(INF_AT, 1), (INF_AT, COEFS[10])],                    # infinity alone, as a unit and as a long term
               6: [(7, 1), (7, 1), (7, R - 2)]}                          # a repeated base whose terms cancel
    for c, terms in special.items():
        if c < n_cols and n_cols > 8:
            cols[c] = terms
    col_ptr, index, coefs = [0], [], []
    for terms in cols:
        index += [i for i, _ in terms]
        coefs += [co for _, co in terms]
        col_ptr.append(len(index))
    return tuple(col_ptr), tuple(index), tuple(coefs)


@functools.lru_cache(maxsize=None)
def host_case():
    """the host test's columns: one per coefficient alone, then the specials and the mixed columns of combine_case(65)"""
    col_ptr, index, coefs = combine_case(65)
    singles = [(3 + i % 4, c) for i, c in enumerate(COEFS)]
    index = [i for i, _ in singles] + list(index)
    coefs = [c for _, c in singles] + list(coefs)
    col_ptr = list(range(len(singles))) + [len(singles) + p for p in col_ptr]
    return tuple(col_ptr), tuple(index), tuple(coefs)


def combine_reference(case, g2):
    col_ptr, index, coefs = case
    k = point_scalars()
    sums = [sum(coefs[t] * k[index[t]] for t in range(col_ptr[c], col_ptr[c + 1])) % R for c in range(len(col_ptr) - 1)]
    return SC.oracle_muls(sums, g2)


# ------------------------------------------------------------------------------------------- points_scale
SEVENS = sum(7 << (4 * i) for i in range(63))   # every digit of the width-4 non-adjacent form is +7 ...
NINES = sum(9 << (4 * i) for i in range(63))    # ... and -7 with a carry into the next
SCALE_COUNTS = (1, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def scale_scalars(n):
    """1, 2, r - 1, the edge scalars of the window widths and the all-sevens pair; the 1 000-point case takes five of them"""
    if n >= 1000:
        return (2, R - 1, (1 << 253) - 1, SEVENS, NINES)
    return tuple(dict.fromkeys((1, 2, R - 1, SEVENS, NINES) + SC.edge_scalars()))


@functools.lru_cache(maxsize=None)
def scale_points(n):
    """(scalars k_i, records k_i * G): infinity in the first and the last lane of the first wave and at the very end"""
    rng = random.Random(0x5CA1E + n)
    k = [rng.randrange(1, R) for _ in range(n)]
    for i in (0, 63, n - 1):
        if i < n and n > 1:
            k[i] = 0
    return tuple(k), tuple(SC.oracle_muls(k, False))


@functools.lru_cache(maxsize=None)
def scale_reference(n, scalar):
    k, _ = scale_points(n)
    return SC.oracle_muls([scalar * x % R for x in k], False)
