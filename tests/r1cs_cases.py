"""Shared case builders of the .r1cs witness-check tests (test_r1cs_host.py on host threads, test_gpu_r1cs_check.py on the
device). The reference everywhere is Python integers, as check_r1cs of tests/golden/make_trapdoor_fixtures.py does it:
dot(A) * dot(B) % r == dot(C). Every builder is deterministic (its own random.Random) and its results are cached, so the two
files and their parametrised cases share one copy, which nobody changes."""
import functools
import importlib.util
import os
import random
import struct

from conftest import GOLDEN, ROOT
from ultragroth_amd import synth

R = synth.R_MOD
TERM_COUNTS = (0, 1, 3, 4, 5, 24, 25, 49, 100)      # the edges of matvec_row's groups of four and of its contraction every 24 terms
CONSTRAINT_COUNTS = (1, 63, 64, 65, 257, 1000)      # below, at and above a wave; more than one block; a ragged last block


def terms_of(lc):
    return list(lc.items()) if isinstance(lc, dict) else list(lc)


def dot(lc, w):
    return sum(c * w[s] for s, c in terms_of(lc)) % R


def reference(rows, w):
    """(failing constraints in order, (a, b, c) of the first failing one or None) by Python integers"""
    failing = [k for k, (a, b, c) in enumerate(rows) if dot(a, w) * dot(b, w) % R != dot(c, w)]
    if not failing:
        return failing, None
    a, b, c = rows[failing[0]]
    return failing, (dot(a, w), dot(b, w), dot(c, w))


def message(failing, m):
    return "witness: constraint %d does not hold (%d of %d fail)" % (failing[0], len(failing), m)


def wtns_file(values):
    secs = [(1, struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", len(values))),
            (2, b"".join(int(x).to_bytes(32, "little") for x in values))]
    return b"wtns" + struct.pack("<II", 2, len(secs)) + b"".join(struct.pack("<IQ", i, len(p)) + p for i, p in secs)


def wtns_values(data):
    """the values of section 2 of a .wtns / .uwtns"""
    pos, n = 12, struct.unpack_from("<I", data, 8)[0]
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", data, pos)
        pos += 12
        if sid == 2:
            return [int.from_bytes(data[pos + 32 * i:pos + 32 * i + 32], "little") for i in range(size // 32)]
        pos += size
    raise ValueError("no section 2")


def sections(data):
    """[(id, bytes)] of a binfile"""
    out, pos = [], 12
    for _ in range(struct.unpack_from("<I", data, 8)[0]):
        sid, size = struct.unpack_from("<IQ", data, pos)
        out.append((sid, data[pos + 12:pos + 12 + size]))
        pos += 12 + size
    return out


def binfile(magic, version, secs):
    return magic + struct.pack("<II", version, len(secs)) + b"".join(struct.pack("<IQ", i, len(p)) + p for i, p in secs)


POOL = 48          # free wires 1 .. POOL that the A and B combinations draw from; wire 0 is the constant 1


@functools.lru_cache(maxsize=None)
def irregular(m, seed=0x51C5):
    """A random circuit of m constraints, satisfied by construction, then broken at {0, m - 1, three random constraints}.
    Returns (n_wires, rows, good witness, bad witness, broken constraints in order)."""
    rng = random.Random(seed * 1000003 + m)
    special = [0, 1, R - 1, R + 5, (1 << 256) - 1]      # the last two count as their residues
    w = [1] + special + [rng.randrange(R) for _ in range(POOL - len(special))]

    def combination(n):
        out = []
        for _ in range(n):
            wire = out[rng.randrange(len(out))][0] if out and rng.random() < 0.15 else rng.randrange(0, POOL + 1)      # sometimes a repeat
            out.append((wire, rng.choice((1, R - 1, 2, R - 2, rng.randrange(R)))))
        return out

    rows = []
    for k in range(m):
        # (the first constraints take the term counts in order, so that every count is met on both sides whatever m >= 9 draws)
        na = TERM_COUNTS[k % len(TERM_COUNTS)] if k < len(TERM_COUNTS) else rng.choice(TERM_COUNTS)
        nb = TERM_COUNTS[(k // 2) % len(TERM_COUNTS)] if k < 2 * len(TERM_COUNTS) else rng.choice(TERM_COUNTS)
        a, b = combination(na), combination(nb)
        sign = rng.choice((1, R - 1))
        rows.append((a, b, {POOL + 1 + k: sign}))
        ab = dot(a, w) * dot(b, w) % R
        value = ab if sign == 1 else (R - ab) % R
        if rng.random() < 0.2:
            value += R                                   # a representative above r of the same residue
        w.append(value)
    assert reference(rows, w)[0] == []
    broken = sorted({0, m - 1} | {rng.randrange(m) for _ in range(3)})
    bad = list(w)
    for k in broken:
        bad[POOL + 1 + k] = (bad[POOL + 1 + k] + 1) % R
    assert reference(rows, bad)[0] == broken
    return len(w), rows, w, bad, broken


@functools.lru_cache(maxsize=None)
def wrap_circuit():
    """The wrap cases as the constraints of one circuit, all of which hold. Returns (n_wires, rows, witness)."""
    big_a, big_b = 1 << 200, 1 << 100
    w = [1, R - 1, 2 * R - 1, big_a, big_b, big_a * big_b % R, 12345]
    rows = [
        ({1: 1}, {1: 1}, {0: 1}),                        # a = b = r - 1, c = 1
        ([(6, 1), (6, R - 1)], {6: 1}, {}),              # an A combination {w: 1, w: r - 1} is 0
        ({}, {}, {}),                                    # all three combinations empty
        ({3: 1}, {4: 1}, {5: 1}),                        # a * b = c mod r where a * b != c as integers
        ({1: 1}, {0: 1}, {2: 1}),                        # (r - 1) * 1 against c = r - 1 given through the witness value 2 r - 1
    ]
    assert big_a * big_b != w[5] and reference(rows, w)[0] == []
    return len(w), rows, w


def wrap_broken():
    """[(witness, failing constraints)]: the wrap circuit with one value changed at a time"""
    n, rows, w = wrap_circuit()
    out = []
    for wire, value in ((2, 2 * R), (5, w[5] + 1), (1, R - 2)):
        bad = list(w)
        bad[wire] = value
        out.append((bad, reference(rows, bad)[0]))
        assert out[-1][1]
    return out


@functools.lru_cache(maxsize=None)
def trapdoor_module():
    spec = importlib.util.spec_from_file_location("make_trapdoor_fixtures", os.path.join(GOLDEN, "make_trapdoor_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def trapdoor():
    """the trapdoor circuit: (module, constraint rows -- without snarkjs' public rows --, .r1cs bytes)"""
    mod = trapdoor_module()
    rows, n_constraints = mod.build_r1cs()
    rows = rows[:n_constraints]
    return mod, rows, trapdoor_r1cs(rows)


def trapdoor_r1cs(rows):
    mod = trapdoor_module()
    return synth.r1cs_file(mod.N_VARS, 1, mod.N_PUBLIC - 1, rows)


def golden(name):
    return open(os.path.join(GOLDEN, "trapdoor", name), "rb").read()
