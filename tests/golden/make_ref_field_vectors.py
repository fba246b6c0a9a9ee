#!/usr/bin/env python3
"""Generator of tests/golden/ref_field_vectors.npz -- TEST TOOLING (own code, no reference source).

tests/test_oracle.py pins the oracle's field layer, the lookup-table row of compute_lookup and derive_challenge to what the
reference's own code computes. That code is only at hand where oracle/_ref/libref_field.so could be built (oracle/Makefile
`ref`: the reference's build/f{r,q}*.cpp + GMP); the tests must run without it. This script runs the tests' inputs through
oracle/_ref once and stores inputs and results, so the tests compare against the stored answers everywhere:

    {fr,fq}_vals                      the operands a (b = vals[(7 i + 3) % n]), 32-byte little-endian each
    {fr,fq}_{mul,add,sub}             ref_<field>_<op>(a, b)
    {fr,fq}_{neg,to_mont,from_mont}   ref_<field>_<op>(a)
    {fr,fq}_inv                       ref_<field>_inv(a) for the first 40 operands (zero where a = 0: not compared)
    {fr,fq}_unreduced, _unreduced_to_mont   operands >= the modulus and ref_<field>_to_mont of them
    lookup_i, lookup_f, lookup_rand   compute_lookup's row inputs (rand in Montgomery form) ...
    lookup_inv, lookup_prod           ... and the row the reference's RawFr calls give
    challenge_k, challenge            index k of a record of the fixture zkey's section 5 and ref derive_challenge of it

Run from the repository root, with oracle/_ref built:  python tests/golden/make_ref_field_vectors.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_field_vectors.npz")


def rows(ints):
    return np.array([list(O.to_le(x)) for x in ints], dtype=np.uint8).reshape(-1, 32)


def field_vectors(which, mod, name):
    """the operands of test_field_against_python_and_reference, in its order"""
    rng = random.Random(which)
    R = 1 << 256
    vals = [0, 1, 2, mod - 1, mod - 2, R % mod, (R * R) % mod] + [rng.randrange(mod) for _ in range(200)]
    pairs = [(a, vals[(7 * i + 3) % len(vals)]) for i, a in enumerate(vals)]
    unreduced = [mod, mod + 5, (1 << 256) - 1, (1 << 255) + 12345]
    out = {name + "_vals": rows(vals)}
    for op in ("mul", "add", "sub"):
        out["%s_%s" % (name, op)] = rows(O.ref_op(name, op, a, b) for a, b in pairs)
    for op in ("neg", "to_mont", "from_mont"):
        out["%s_%s" % (name, op)] = rows(O.ref_op(name, op, a) for a in vals)
    out[name + "_inv"] = rows(O.ref_op(name, "inv", a) if a else 0 for a in vals[:40])
    out[name + "_unreduced"] = rows(unreduced)
    out[name + "_unreduced_to_mont"] = rows(O.ref_op(name, "to_mont", a) for a in unreduced)
    return out


def lookup_vectors():
    """the rows of test_lookup_row_against_the_reference_overloads, in its order, then its i + rand = 0 case"""
    rng = random.Random(77)
    R = 1 << 256
    ins = []
    for _ in range(60):
        rand = rng.randrange(O.R_MOD)
        i = rng.choice([0, 1, 2, 255, 65535, rng.randrange(1 << 20)])
        f = rng.choice([0, 1, 7, (1 << 31) - 1, 1 << 31, (1 << 31) + 5, (1 << 32) - 1, rng.randrange(1 << 32)])
        ins.append((i, f, rand * R % O.R_MOD))
    ins.append((5, 9, (O.R_MOD - 5) * R % O.R_MOD))
    got = [O.ref_lookup_row(i, f, rm) for i, f, rm in ins]
    return {"lookup_i": np.array([i for i, _, _ in ins], dtype=np.uint32),
            "lookup_f": np.array([f for _, f, _ in ins], dtype=np.uint32),
            "lookup_rand": rows(rm for _, _, rm in ins),
            "lookup_inv": rows(g[0] for g in got), "lookup_prod": rows(g[1] for g in got)}


def challenge_vectors():
    """the records of test_derive_challenge_against_the_reference_code: section 5 of the fixture zkey, k = 0, 7, ... < 400"""
    zkey = open(os.path.join(ROOT, "tests", "golden", "circuit_final.zkey"), "rb").read()
    off, sz = O.section(zkey, "zkey", 5)
    a = zkey[off:off + sz]
    ks = [k for k in range(0, 400, 7) if a[64 * k:64 * k + 64] != bytes(64)]
    return {"challenge_k": np.array(ks, dtype=np.uint32),
            "challenge": rows(O.ref_derive_challenge(a[64 * k:64 * k + 64]) for k in ks)}


def main():
    if O.ref is None or not hasattr(O.ref, "ref_lookup_row"):
        raise SystemExit("oracle/_ref/libref_field.so is not built (oracle/Makefile `ref`): nothing to take the answers from")
    vec = {}
    vec.update(field_vectors(O.FR, O.R_MOD, "fr"))
    vec.update(field_vectors(O.FQ, O.Q_MOD, "fq"))
    vec.update(lookup_vectors())
    vec.update(challenge_vectors())
    np.savez(OUT, **vec)
    print("wrote", OUT, sum(v.nbytes for v in vec.values()), "bytes of vectors")


if __name__ == "__main__":
    main()
