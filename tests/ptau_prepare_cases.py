"""Shared case builders of the powers-of-tau preparation tests (test_ptau_prepare_host.py on host threads,
test_gpu_ptau_prepare.py on the device). Every comparison in those files is byte for byte. Every test point is k_j * G for a known
k_j, made with the CPU oracle's scalar multiplication; the expected output of a transform of size N = 2^log_n is the oracle's
multiple of (1 / N) sum_j omega^(-j k) k_j mod r, computed with Python integers. For whole files the reference is the test writer
synth.ptau_file, which makes sections 12 - 15 from Lagrange VALUES of the known tau, not by a transform of points.
Every builder is deterministic and cached, so the two files share one copy, which nobody changes."""
import functools
import random

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC

R = SC.R
# the input sets of a size; the last two give fewer than N points (the rest is infinity)
SETS = ("random", "tau", "equal", "alternating", "infinity", "single_first", "single_last", "single_middle", "given_all_but_one",
        "given_half_plus_one")
LARGE_SETS = ("random", "equal")                # above 2^7
EQUAL_C = 0x1c3f5a7e9b2d4f6081a3c5e7092b4d6f8fa1c3e507192b4d6f8193a5c7e90b2d % R
LAGRANGE_IDS = (12, 13, 14, 15)
RECORD = {2: 64, 3: 128, 4: 64, 5: 64, 12: 64, 13: 128, 14: 64, 15: 64}


@functools.lru_cache(maxsize=None)
def scalars(name, log_n):
    """the k_j that are given: N of them, or fewer for the two padded sets"""
    n = 1 << log_n
    rng = random.Random(0x1A77 + 64 * log_n)
    if name == "random":
        return tuple(rng.randrange(1, R) for _ in range(n))
    if name == "tau":
        tau = int(SC.trapdoor_dict()["tau"])
        return tuple(pow(tau, j, R) for j in range(n))
    if name == "equal":                          # every first-stage sum is a doubling, every difference infinity: P, inf, inf, ...
        return (EQUAL_C,) * n
    if name == "alternating":                    # every first-stage sum is infinity
        return tuple(EQUAL_C if j % 2 == 0 else R - EQUAL_C for j in range(n))
    if name == "infinity":
        return (0,) * n
    if name.startswith("single_"):
        at = {"single_first": 0, "single_last": n - 1, "single_middle": n // 2}[name]
        return tuple(EQUAL_C if j == at else 0 for j in range(n))
    given = {"given_all_but_one": n - 1, "given_half_plus_one": n // 2 + 1}[name]
    return tuple(rng.randrange(1, R) for _ in range(min(given, n)))


@functools.lru_cache(maxsize=None)
def transformed(name, log_n):
    """(1 / N) sum_j omega^(-j k) k_j mod r for k = 0 .. N - 1, omega = 5^((r - 1) / N)"""
    n = 1 << log_n
    k = scalars(name, log_n)
    w_inv = pow(pow(5, (R - 1) // n, R), -1, R)
    powers = [1]
    for _ in range(n - 1):
        powers.append(powers[-1] * w_inv % R)
    n_inv = pow(n, -1, R)
    live = [(j, v) for j, v in enumerate(k) if v]
    return tuple(n_inv * sum(v * powers[j * i % n] for j, v in live) % R for i in range(n))


@functools.lru_cache(maxsize=None)
def case(name, log_n, g2):
    """(the records that are given, the N expected records)"""
    return tuple(SC.oracle_muls(scalars(name, log_n), g2)), tuple(SC.oracle_muls(transformed(name, log_n), g2))


def sets_for(log_n):
    return SETS if log_n <= 7 else LARGE_SETS


# ------------------------------------------------------------------------------------------- files
def sections(data):
    return dict(RC.sections(data))


def other_point(g2):
    """a valid point that no synthesized file holds at the places the tests plant it"""
    return SC.oracle_mul(0x5eed0f0ca11ab1e, bool(g2))


def planted(ptau, sid, record):
    """the prepared file with one record of section sid replaced by another valid point"""
    size = RECORD[sid]
    p = bytearray(sections(ptau)[sid])
    new = other_point(sid in (3, 13))
    assert bytes(p[record * size:record * size + size]) != new
    p[record * size:record * size + size] = new
    return PC.with_sections(ptau, {sid: bytes(p)})


def plants(power):
    """(section, record) of the issue's three places: section 13 level 3, section 12's padded level, section 15's last record"""
    n = 1 << power
    return ((13, 7 + 5), (12, 2 * n - 1 + (77 % (2 * n))), (15, 2 * n - 2))


def header_fields(section1):
    import struct
    n8 = struct.unpack_from("<I", section1, 0)[0]
    power, ceremony = struct.unpack_from("<II", section1, 36)
    return {"n8": n8, "prime": section1[4:36], "power": power, "ceremony_power": ceremony, "rest": section1[44:]}
