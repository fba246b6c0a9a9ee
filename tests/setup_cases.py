"""Shared case builders of the development-setup tests (test_setup_host.py on host threads, test_gpu_setup.py on the device).
Every comparison in those files is byte for byte. The references are: the committed trapdoor fixtures; the generator script's
own lagrange_at; the CPU oracle's scalar multiplications; and, for small circuits, python_key_sections below, which restates
the generator's setup() for any rows. Every builder is deterministic and cached, so the files share one copy."""
import functools
import json
import random
import struct

import oracle as O
import r1cs_cases as RC
from ultragroth_amd import synth

R = synth.R_MOD
MONT = 1 << 256
GEN_MUL_COUNTS = (1, 63, 64, 65, 257)          # below, at and above a wave; more than one workgroup with a ragged end
WINDOWS = (8, 11, 13, 16)                      # the host's width, the device defaults, the widest


def trapdoor_dict():
    return json.loads(RC.golden("trapdoor.json").decode())


@functools.lru_cache(maxsize=None)
def ultra_spec():
    """rand_indx and the round / final signal lists of the generator's UltraGroth instance (main() of the script)"""
    m = RC.trapdoor_module()
    round_signals = [m.X, m.Y] + [m.C0 + j for j in range(m.J)] + [m.F0 + i for i in range(m.L)]
    final_signals = [m.INV1 + j for j in range(m.J)] + [m.INV2 + i for i in range(m.L)] + [m.PROD + i for i in range(m.L)]
    return {"rand_indx": m.RHO, "round_signals": round_signals, "final_signals": final_signals}


def window_count(c):
    return (255 + c - 1) // c


@functools.lru_cache(maxsize=None)
def edge_scalars():
    """0, 1, 2, r - 1, r - 2, 2^253; all bits set (every raw window digit is the maximum whatever the width: the signed-digit
    carry runs from the bottom window to the top); per width c: one digit alone -- 1, exactly half (the largest positive digit)
    and half + 1 (the first that turns negative and carries) -- in a middle window, and the top window alone"""
    out = [0, 1, 2, R - 1, R - 2, 1 << 253, (1 << 253) - 1]
    for c in WINDOWS:
        mid = c * (window_count(c) // 2)
        out += [1 << mid, (1 << (c - 1)) << mid, ((1 << (c - 1)) + 1) << mid, ((1 << c) - 1) << mid]
        top = c * (window_count(c) - 1)
        out.append(1 << top)
        out.append(((R >> top) << top))            # the top window as full as a scalar below r allows, nothing below it
    assert all(0 <= s < R for s in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gen_mul_scalars(n):
    """n scalars: the edges first, then seeded random ones; zeros in the first, a middle and the last lane of the first wave
    (n >= 63) and as the whole third wave (n >= 192)"""
    rng = random.Random(0x5E7 + n)
    pool = list(edge_scalars()[1:])
    out = [pool[i] if i < len(pool) else rng.randrange(R) for i in range(n)]
    if n == 1:
        return (R - 1,)
    for i in (0, 31, 63):
        if i < n:
            out[i] = 0
    if n >= 192:
        out[128:192] = [0] * 64
    return tuple(out)


def _m(x):
    return (x * MONT % O.Q_MOD).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def _generators():
    m = RC.trapdoor_module()
    return m.G1_REC, m.G2_REC


@functools.lru_cache(maxsize=None)
def oracle_mul(scalar, g2):
    g1rec, g2rec = _generators()
    scalar %= R
    if not scalar:
        return bytes(128 if g2 else 64)
    return O.g2_mul(g2rec, scalar) if g2 else O.g1_mul(g1rec, scalar)


def oracle_muls(scalars, g2):
    return [oracle_mul(s, bool(g2)) for s in scalars]


def lagrange_reference(x, log_n, coset):
    """the generator's lagrange_at for another domain size (the module computes with its global N)"""
    n = 1 << log_n
    if coset:
        x = x * pow(pow(5, (R - 1) // (2 * n), R), -1, R) % R
    omega = pow(5, (R - 1) // n, R)
    zn = (pow(x, n, R) - 1) % R
    ninv = pow(n, -1, R)
    out, wk = [], 1
    for _ in range(n):
        out.append(zn * wk % R * ninv % R * pow((x - wk) % R, -1, R) % R)
        wk = wk * omega % R
    return out


# ------------------------------------------------------------------------------------------- circuits
@functools.lru_cache(maxsize=None)
def odd_circuit(m, n_pub_out, n_pub_in, seed=0xD5):
    """An irregular circuit in the style of r1cs_cases.irregular: its m random constraints (repeated wires inside a combination,
    coefficients r - 1, r - 2, random), then: a pair of terms summing to 0 beside a live term, a pair that is the whole
    combination, three empty combinations, a coefficient r - 1 alone; three wires at the end occur in no matrix.
    Returns (n_wires, rows, .r1cs bytes)."""
    n_wires, rows, _, _, _ = RC.irregular(m, seed)
    rows = list(rows) + [
        ([(5, 7), (9, 3), (5, R - 7)], {3: R - 1}, {}),
        ([(4, 1), (4, R - 1)], [(6, 2), (6, 2), (6, R - 3)], {0: R - 1}),
        ({}, {}, {}),
        ({2: R - 1}, {}, [(0, 5), (0, R - 5)]),
    ]
    n_wires += 3
    return n_wires, tuple(rows), synth.r1cs_file(n_wires, n_pub_out, n_pub_in, rows)


@functools.lru_cache(maxsize=None)
def long_column_circuit(m):
    """m constraints x_k * x_k = y_k + 1: every C names wire 0, so the column of wire 0 in C has m terms"""
    rows = [({1 + k: 1}, {1 + k: 1}, {0: 1, 1 + m + k: 1}) for k in range(m)]
    n_wires = 1 + 2 * m
    return n_wires, tuple(rows), synth.r1cs_file(n_wires, 0, 1, rows)


CHAIN, EXTRA = 4000, 6200


@functools.lru_cache(maxsize=None)
def sparse_b_circuit():
    """The end-to-end circuit: a squaring chain x_(i+1) = x_i * x_i of CHAIN steps whose last value is the public output, and
    EXTRA constraints e_j * 1 = f_j whose 2 * EXTRA wires appear on no B side. nVars = 16 402 >= 2^14 with a quarter of the B
    points real: the prover's sparse-B path. 10 200 constraints: the domain is 2^14.
    wires: 0 one | 1 out = x_CHAIN | 2 x_0 | 3 .. CHAIN + 1: x_1 .. x_(CHAIN-1) | e_j | f_j. Returns (.r1cs bytes, .wtns bytes, out)."""
    x = lambda i: 1 if i == CHAIN else 2 + i
    rows = [({x(i): 1}, {x(i): 1}, {x(i + 1): 1}) for i in range(CHAIN)]
    e0 = CHAIN + 2
    rows += [({e0 + j: 1}, {0: 1}, {e0 + EXTRA + j: 1}) for j in range(EXTRA)]
    n_wires = e0 + 2 * EXTRA
    w = [0] * n_wires
    w[0] = 1
    v = 3
    for i in range(CHAIN):
        w[x(i)] = v
        v = v * v % R
    w[1] = v
    rng = random.Random(0xE2E)
    for j in range(EXTRA):
        w[e0 + j] = w[e0 + EXTRA + j] = rng.randrange(R)
    assert n_wires >= 1 << 14 and len(rows) + 2 <= 1 << 14
    return synth.r1cs_file(n_wires, 1, 0, rows), RC.wtns_file(w), v


def zkey_header(zkey):
    """(nVars, nPublic, domainSize) of a zkey's section 2"""
    sec = dict(RC.sections(zkey))[2]
    return struct.unpack_from("<III", sec, 4 + 32 + 4 + 32)


def python_key_sections(rows, n_wires, n_public, log_n, t):
    """Sections 3 - 9 of the Groth16 key of `rows`, restating setup() and coef_section() of the generator script for any
    circuit, with Python integers and the oracle's scalar multiplications. Small circuits only."""
    n = 1 << log_n
    tau, alpha, beta, gamma, delta = (int(t[k]) for k in ("tau", "alpha", "beta", "gamma", "delta_final"))
    rows = [tuple(RC.terms_of(lc) for lc in row) for row in rows]
    rows += [([(s, 1)], [], []) for s in range(n_public + 1)]
    lag = lagrange_reference(tau, log_n, False)
    uvw = [[0] * n_wires for _ in range(3)]
    for k, row in enumerate(rows):
        for m in range(3):
            for s, co in row[m]:
                uvw[m][s] = (uvw[m][s] + co * lag[k]) % R
    u, v, w = uvw
    K = [(beta * u[s] + alpha * v[s] + w[s]) % R for s in range(n_wires)]
    lag_coset = lagrange_reference(tau, log_n, True)
    h_scale = (pow(tau, n, R) - 1) * pow((-2 * delta) % R, -1, R) % R
    g1 = lambda k: oracle_mul(k % R, False)
    recs = []
    for k, row in enumerate(rows):
        for m in range(2):
            merged = {}
            for s, co in row[m]:
                merged[s] = (merged.get(s, 0) + co) % R
            for s in sorted(merged):
                if merged[s]:
                    recs.append(struct.pack("<III", m, k, s) + (merged[s] * MONT * MONT % R).to_bytes(32, "little"))
    return {
        3: b"".join(g1(K[s] * pow(gamma, -1, R)) for s in range(n_public + 1)),
        4: struct.pack("<I", len(recs)) + b"".join(recs),
        5: b"".join(g1(u[s]) for s in range(n_wires)),
        6: b"".join(g1(v[s]) for s in range(n_wires)),
        7: b"".join(oracle_mul(v[s], True) for s in range(n_wires)),
        8: b"".join(g1(K[s] * pow(delta, -1, R)) for s in range(n_public + 1, n_wires)),
        9: b"".join(g1(lag_coset[k] * h_scale) for k in range(n)),
    }
