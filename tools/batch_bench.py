#!/usr/bin/env python3
"""Single proofs against batched proofs (ug_groth16_prover_prove_batch) on one created prover, alternating in one process.

For every size: a seeded synthetic circuit (synth.build_circuit) and K = max(ks) different witnesses (synth.build_witness,
distinct seeds, uniform and circom-like alternating). Before timing, every batch output is checked once against the single
proof with the same blinding. Then `rounds` rounds; in each, every mode proves the same K witnesses, timed the same way: one
loop of calls over all K -- K prove() calls, or K / k prove_batch() calls of k witnesses. Prints one JSON line per size with
the per-proof milliseconds (median over the rounds) and the batch's speed-up.

    python tools/batch_bench.py --logs 16 18 20 22 24 --ks 1 4 8 --rounds 3

--ultra: the same for a created UltraGroth prover: synth.build_ultra_circuit with a lookup table of 2^lookup_log rows and K
distinct witnesses of it (synth.build_ultra_witnesses: other signals, chunks and frequencies), blinding rk, r, s per witness.

    python tools/batch_bench.py --ultra --lookup-log 16 --logs 16 20 22 --ks 8 --rounds 5

--profile single|batch: after the set-up and one warm-up call, only `--steps` calls of that mode (K witnesses each: K prove()
calls, or one prove_batch of K) and nothing else: the command for `rocprofv3 --kernel-trace --stats`, whose per-kernel totals
divided by steps + 1 are one step's split (the set-up kernels -- synthetic points, window tables -- have names of their own).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ULTRAGROTH_TEST_HOOKS", "1")


def rs(b):
    return hashlib.sha256(b"r%d" % b).digest()[:31] + hashlib.sha256(b"s%d" % b).digest()[:31]


def rkrs(b):
    return hashlib.sha256(b"rk%d" % b).digest()[:31] + rs(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 18, 20, 22, 24])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", choices=["single", "batch"], default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ultra", action="store_true", help="a created UltraGroth prover instead of a Groth16 one")
    ap.add_argument("--lookup-log", type=int, default=16, help="--ultra: log2 rows of the lookup table")
    args = ap.parse_args()
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    dev = ug.Device(0)
    kmax = max(args.ks)
    for log in args.logs:
        if args.ultra:
            zkey, _, _ = synth.build_ultra_circuit(dev, log, lookup_log=args.lookup_log)
            wtns = synth.build_ultra_witnesses(log, kmax, lookup_log=args.lookup_log, witness_seed=0xB000)
        else:
            zkey, _, _ = synth.build_circuit(dev, log, mix="U")
            wtns = [synth.build_witness(log, "UC"[b % 2], seed=0xB000 + 16 * b) for b in range(kmax)]
        blinding = rkrs if args.ultra else rs
        with (ug.UltraGrothProver if args.ultra else ug.Groth16Prover)(zkey) as p:
            p.tables_ready(wait=True)
            if args.profile:
                step = (lambda: [p.prove(w) for w in wtns]) if args.profile == "single" else (lambda: p.prove_batch(wtns))
                for _ in range(args.steps + 1):
                    step()
                print(json.dumps({"log_domain": log, "protocol": "ultragroth" if args.ultra else "groth16", "profile": args.profile, "calls": args.steps + 1, "witnesses": kmax}), flush=True)
                continue
            ug.set_test_blinding(b"".join(blinding(b) for b in range(kmax)))
            batch = p.prove_batch(wtns)
            ug.set_test_blinding(b"")
            for b, w in enumerate(wtns):
                ug.set_test_blinding(blinding(b))
                if p.prove(w) != batch[b]:
                    raise SystemExit("2^%d: batch proof %d differs from the single proof" % (log, b))
            ug.set_test_blinding(b"")
            p.prove(wtns[0]); p.prove_batch(wtns)                  # warm-up of both paths
            single, batched = [], {k: [] for k in args.ks}
            for _ in range(args.rounds):
                t = time.perf_counter()
                for w in wtns:
                    p.prove(w)
                single.append((time.perf_counter() - t) * 1e3 / kmax)
                for k in args.ks:
                    t = time.perf_counter()
                    for b0 in range(0, kmax - k + 1, k):
                        p.prove_batch(wtns[b0:b0 + k])
                    batched[k].append((time.perf_counter() - t) * 1e3 / (kmax // k * k))
            s_ms = statistics.median(single)
            out = {"log_domain": log, "protocol": "ultragroth" if args.ultra else "groth16", "mix": "U/C alternating", "rounds": args.rounds, "single_ms_per_proof": round(s_ms, 3),
                   "tables": [c for c, _, _, _ in p.table_plan()]}
            if args.ultra:
                out["lookup_log"] = args.lookup_log
            for k in args.ks:
                b_ms = statistics.median(batched[k])
                out["batch%d_ms_per_proof" % k] = round(b_ms, 3)
                out["batch%d_speedup" % k] = round(s_ms / b_ms, 3)
            out["rounds_ms"] = {"single": [round(x, 2) for x in single], **{"batch%d" % k: [round(x, 2) for x in batched[k]] for k in args.ks}}
            print(json.dumps(out), flush=True)
        del zkey
    dev.close()


if __name__ == "__main__":
    main()
