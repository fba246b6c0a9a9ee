#!/usr/bin/env python3
"""Times the witness check against a circuit's .r1cs (ultragroth_amd/csrc/r1cs.hip) on the device.

    python tools/witness_check_bench.py [--logs 16,20] [--seed 1] [--reps 5] [--device 0]
    python tools/witness_check_bench.py --provers 20,22 [--parent-tree DIR] [--rounds 3] [--steps 8]

The circuit is synthetic and satisfied by construction, made from the seed alone:
    m = 2^log constraints; a pool of m / 4 free wires (wire 0 = 1, the others uniform field elements);
    row k: A and B each draw n terms, n uniform in 1 .. 8 (mean 4.5), wires uniform over the pool, coefficients uniform over a
    table of 16 field elements (the first four are 1, r - 1, 2, r - 2); C is one dedicated wire per constraint with coefficient 1,
    set to (A.w)(B.w) mod r. nWires = m / 4 + m.
Per size it prints one JSON line: ug_r1cs_create (host wall, parse + upload + conversion), the check kernel alone (device_ms of
ug_r1cs_check, median and min .. max of --reps calls after one warm-up), the whole ug_r1cs_check call (host wall), and
ug_witness_check end to end from the two file buffers (context, create, witness upload, check, destroy).
The bytes the kernel must read are terms * 36 (signal id + coefficient) + gathers * 32 (one witness element per term); the status
bytes it may write are not counted (m * 0). achieved_GBps = those bytes over the kernel's median time.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

# (UG_BENCH_TREE: the checkout whose package and library a --provers child loads -- the parent commit's for the "parent" variant)
sys.path.insert(0, os.environ.get("UG_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug                      # noqa: E402
from ultragroth_amd import synth                 # noqa: E402

R = synth.R_MOD


def build(log_m, seed, m=None, pool=None, want_coefs=False):
    """(r1cs bytes, wtns bytes, witness values, terms per matrix[, zkey section-4 records with snarkjs' public rows for 1 public signal])"""
    m = (1 << log_m) if m is None else m
    pool = max(2, m // 4) if pool is None else pool
    rng = np.random.default_rng(seed)
    pr = random.Random(seed)
    coef = [1, R - 1, 2, R - 2] + [pr.randrange(R) for _ in range(12)]
    w = [1] + [pr.randrange(R) for _ in range(pool - 1)]
    n = rng.integers(1, 9, size=(m, 2))                          # terms of A and of B per row
    total = int(n.sum())
    wires = rng.integers(0, pool, size=total, dtype=np.uint32)
    cidx = rng.integers(0, 16, size=total, dtype=np.uint8)
    # the witness: one pass in Python integers
    wl, cl = wires.tolist(), cidx.tolist()
    cvals, p = [], 0
    for na, nb in n.tolist():
        a = sum(coef[cl[i]] * w[wl[i]] for i in range(p, p + na)) % R
        p += na
        b = sum(coef[cl[i]] * w[wl[i]] for i in range(p, p + nb)) % R
        p += nb
        cvals.append(a * b % R)
    # the file, section 2 laid out with numpy: per row [nA | A terms | nB | B terms | 1 | C term]
    per_row = 12 + 36 * (n.sum(axis=1) + 1)
    start = np.concatenate(([0], np.cumsum(per_row)))[:-1].astype(np.int64)
    buf = np.zeros(int(per_row.sum()), dtype=np.uint8)
    ctab = np.frombuffer(b"".join(c.to_bytes(32, "little") for c in coef), dtype=np.uint8).reshape(16, 32)

    def put_u32(pos, values):
        v = np.ascontiguousarray(values, dtype="<u4").view(np.uint8).reshape(-1, 4)
        buf[pos[:, None] + np.arange(4)] = v

    na, nb = n[:, 0].astype(np.int64), n[:, 1].astype(np.int64)
    pos_a, pos_b = start, start + 4 + 36 * na
    pos_c = pos_b + 4 + 36 * nb
    put_u32(pos_a, na); put_u32(pos_b, nb); put_u32(pos_c, np.ones(m))
    # term t of the flat lists belongs to row r(t), matrix A or B; its place inside the row
    counts = n.reshape(-1).astype(np.int64)                       # nA0, nB0, nA1, nB1, ...
    first = np.concatenate(([0], np.cumsum(counts)))[:-1]
    within = np.arange(total, dtype=np.int64) - np.repeat(first, counts)
    base = np.repeat(np.stack([pos_a + 4, pos_b + 4], axis=1).reshape(-1), counts)
    tpos = base + 36 * within
    put_u32(tpos, wires)
    buf[(tpos + 4)[:, None] + np.arange(32)] = ctab[cidx]
    put_u32(pos_c + 4, pool + np.arange(m))
    buf[pos_c + 8] = 1                                            # coefficient 1
    n_wires = pool + m
    import struct
    sec1 = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, 0, 0, n_wires - 1, n_wires, m)
    sec2 = buf.tobytes()
    r1cs = b"r1cs" + struct.pack("<II", 1, 2) + struct.pack("<IQ", 1, len(sec1)) + sec1 + struct.pack("<IQ", 2, len(sec2)) + sec2
    values = b"".join(x.to_bytes(32, "little") for x in w) + b"".join(x.to_bytes(32, "little") for x in cvals)
    wsec1 = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", n_wires)
    wtns = b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(wsec1)) + wsec1 + struct.pack("<IQ", 2, len(values)) + values
    out = (r1cs, wtns, values, (int(na.sum()), int(nb.sum()), m))
    if want_coefs:                                                # the same A and B as a zkey stores them: coef * 2^512 mod r
        rec = np.zeros(total + 2, dtype=synth.COEF_DTYPE)
        rec["m"][:total] = np.repeat(np.tile(np.array([0, 1], dtype=np.uint32), m), counts)
        rec["c"][:total] = np.repeat(np.repeat(np.arange(m, dtype=np.uint32), 2), counts)
        rec["s"][:total] = wires
        mont = np.frombuffer(b"".join(((c << 512) % R).to_bytes(32, "little") for c in coef), dtype="<u8").reshape(16, 4)
        rec["v"][:total] = mont[cidx]
        for srow in range(2):                                     # public rows: signal s at row m + s, A side only
            rec["m"][total + srow], rec["c"][total + srow], rec["s"][total + srow] = 0, m + srow, srow
            rec["v"][total + srow] = mont[0]
        out += (rec,)
    return out


def prover_child(variant, zkey_path, wtns_path, r1cs_path, steps):
    """one variant in a process of its own (the library is chosen by ULTRAGROTH_LIB before the import): JSON on stdout"""
    zkey, wtns = open(zkey_path, "rb").read(), open(wtns_path, "rb").read()
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        if variant == "attached":
            t = time.perf_counter()
            p.attach_r1cs(open(r1cs_path, "rb").read())
            attach_ms = (time.perf_counter() - t) * 1e3
        p.load_witness(wtns)
        for _ in range(2):
            p.prove_resident()
        one = []
        for _ in range(steps):
            t = time.perf_counter()
            p.prove_resident()
            one.append((time.perf_counter() - t) * 1e3)
        p.prove_batch([wtns] * 8)
        batch = []
        for _ in range(2):
            t = time.perf_counter()
            p.prove_batch([wtns] * 8)
            batch.append((time.perf_counter() - t) * 1e3 / 8)
    res = {"variant": variant, "prove_ms": {"median": round(float(np.median(one)), 3), "min": round(min(one), 3), "max": round(max(one), 3)},
           "batch8_ms_per_proof": [round(b, 3) for b in batch]}
    if variant == "attached":
        res["attach_ms"] = round(attach_ms, 1)
    print(json.dumps(res), flush=True)


def provers(log_domain, seed, parent_lib, rounds, steps, tmp):
    """parent commit (parent_lib: its checkout) | this build | this build with the .r1cs attached, alternated `rounds` times, each in a child process, on
    one circuit of domain 2^log_domain: 2^(log_domain - 1) constraints of the distribution above over 2^log_domain - 1 wires"""
    import subprocess
    m = 1 << (log_domain - 1)
    r1cs, wtns, values, terms, rec = build(log_domain - 1, seed, m=m, pool=m - 1, want_coefs=True)
    # (one public signal: wire 1 -- the file's header says so, the zkey's too)
    import struct
    r1cs = r1cs[:12 + 12 + 36 + 4] + struct.pack("<II", 1, 0) + r1cs[12 + 12 + 36 + 12:]
    dev = ug.Device(0)
    zkey, _, info = synth.build_circuit(dev, log_domain, coefs=rec)
    dev.close()
    paths = [os.path.join(tmp, "wcb_%d.%s" % (log_domain, e)) for e in ("zkey", "wtns", "r1cs")]
    for path, data in zip(paths, (zkey, wtns, r1cs)):
        with open(path, "wb") as f:
            f.write(data)
    del zkey
    print(json.dumps({"provers_log_domain": log_domain, "constraints": m, "terms": terms}), flush=True)
    try:
        for rnd in range(rounds):
            for variant in (["parent"] if parent_lib else []) + ["unattached", "attached"]:
                env = dict(os.environ)
                if variant == "parent":
                    env["UG_BENCH_TREE"] = parent_lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant] + paths + ["--steps", str(steps)],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("child %s failed (%d): %s" % (variant, r.returncode, r.stderr[-800:]))
                print(r.stdout.strip().splitlines()[-1], flush=True)
    finally:
        for path in paths:
            os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--build-only", action="store_true", help="make the circuit and check it on host threads (no GPU)")
    ap.add_argument("--provers", default="", help="log2 domains, e.g. 20,22: a Groth16 prover on this circuit, parent library | this build | "
                                                  "this build attached, alternated in child processes")
    ap.add_argument("--parent-tree", dest="parent_lib", default="", help="--provers: a checkout of the parent commit with its library built "
                                                                           "(its own package loads it; omit: two variants)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--child", nargs=4, metavar=("VARIANT", "ZKEY", "WTNS", "R1CS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        prover_child(*args.child, steps=args.steps)
        return
    if args.provers:
        for log_domain in [int(x) for x in args.provers.split(",")]:
            provers(log_domain, args.seed, args.parent_lib, args.rounds, args.steps, args.tmp)
        return
    for log_m in [int(x) for x in args.logs.split(",")]:
        t = time.perf_counter()
        r1cs, wtns, values, terms = build(log_m, args.seed)
        build_s = time.perf_counter() - t
        info = ug.r1cs_info(r1cs)
        assert tuple(info["terms"]) == terms
        if args.build_only:
            assert ug.witness_check(r1cs, wtns, device=-1) is None
            print(json.dumps({"log_constraints": log_m, "terms": terms, "build_s": round(build_s, 2), "host_check": "ok"}), flush=True)
            continue
        dev = ug.Device(args.device)
        t = time.perf_counter()
        cs = dev.r1cs(r1cs)
        create_ms = (time.perf_counter() - t) * 1e3
        v = dev.dvec(info["n_wires"], values)
        assert cs.check(v)["failed"] == 0                          # warm-up, and the circuit holds
        kern, call = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            rep = cs.check(v)
            call.append((time.perf_counter() - t) * 1e3)
            kern.append(rep["device_ms"])
        cs.close()
        del v
        ug.witness_check(r1cs, wtns, device=args.device)          # warm-up of the stand-alone path
        e2e = []
        for _ in range(max(2, args.reps // 2)):
            t = time.perf_counter()
            assert ug.witness_check(r1cs, wtns, device=args.device) is None
            e2e.append((time.perf_counter() - t) * 1e3)
        dev.close()
        total_terms = sum(terms)
        must_read = total_terms * 36 + total_terms * 32
        med = float(np.median(kern))
        print(json.dumps({
            "log_constraints": log_m, "n_wires": info["n_wires"], "terms": terms, "r1cs_MB": round(len(r1cs) / 1e6, 1), "build_s": round(build_s, 1),
            "create_ms": round(create_ms, 2),
            "kernel_ms": {"median": round(med, 4), "min": round(min(kern), 4), "max": round(max(kern), 4)},
            "check_call_ms": {"median": round(float(np.median(call)), 3), "min": round(min(call), 3), "max": round(max(call), 3)},
            "witness_check_e2e_ms": {"median": round(float(np.median(e2e)), 1), "min": round(min(e2e), 1), "max": round(max(e2e), 1)},
            "must_read_bytes": must_read, "achieved_GBps": round(must_read / (med * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
