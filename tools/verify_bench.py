#!/usr/bin/env python3
"""Throughput of batch verification (include/verifier.h: ug_groth16_verify_batch) beside the single-proof verifier.

For N = 2^10, 2^14, 2^16 valid Groth16 proofs of tests/golden/trapdoor/groth16.{zkey,wtns}: proofs/s on the device, with
device = -1 (the same protocol on host threads), and of groth16_verify called from 16 host threads; at 2^14 also with one bad
proof and with 1 % bad proofs. A pool of --pool distinct proofs (prove_batch, fresh blinding) is repeated to fill N: every slot
still gets its own scalar, Miller loop and tree leaf, so the work is that of N distinct proofs. Prints a text report (the body of
profiles/verify_batch.txt) and writes it to --out.

    python tools/verify_bench.py --out out/verify_batch.txt [--sizes 10,14,16] [--host-sizes 10,14]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TD = os.path.join(ROOT, "tests", "golden", "trapdoor")


def read(name, mode="rb"):
    with open(os.path.join(TD, name), mode) as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--host-sizes", default="10,14,16", help="log2 sizes that also run with device = -1")
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--single-sample", type=int, default=512, help="proofs timed through groth16_verify on 16 threads")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ultragroth_amd as ug
    from ultragroth_amd._lib import VerifyBatchStats
    L = ug.load()
    vk = read("groth16_vkey.json", "r").encode()
    zkey, wtns = read("groth16.zkey"), read("groth16.wtns")
    pool = []
    with ug.Groth16Prover(zkey) as p:
        while len(pool) < a.pool:
            pool += p.prove_batch([wtns] * 16)
    pool = [(pr.encode(), pub.encode()) for pr, pub in pool[:a.pool]]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def run(n, device, bad=()):
        proofs = [pool[i % len(pool)][0] for i in range(n)]
        pubs = [pool[i % len(pool)][1] for i in range(n)]
        for i in bad:
            s = json.loads(pubs[i])
            s[0] = str(int(s[0]) + 1)
            pubs[i] = json.dumps(s).encode()
        pa, ia = (C.c_char_p * n)(*proofs), (C.c_char_p * n)(*pubs)
        verdicts, stats, err = (C.c_int * n)(), VerifyBatchStats(), C.create_string_buffer(256)
        t0 = time.perf_counter()
        rc = getattr(L, "ug_groth16_verify_batch")(device, n, pa, ia, vk, verdicts, C.byref(stats), err, 255)
        dt = time.perf_counter() - t0
        wrong = [i for i in range(n) if (verdicts[i] != 0) != (i in set(bad))]
        if rc == 2 or wrong:
            raise RuntimeError("verify_batch: rc %d, %s, %d wrong verdicts" % (rc, err.value.decode(), len(wrong)))
        ms = (C.c_double * 3)()
        L.ug_verify_batch_kernel_ms(ms)
        return dt, stats, list(ms)

    say("# batch verification, Groth16, tests/golden/trapdoor/groth16 (%d distinct proofs repeated to fill N)" % len(pool))
    run(64, a.device)                                                  # warm-up: code objects, the context
    host_sizes = {int(s) for s in a.host_sizes.split(",") if s}
    for lg in [int(s) for s in a.sizes.split(",")]:
        n = 1 << lg
        dt, st, ms = run(n, a.device)
        say("N=2^%d device      %9.0f proofs/s  wall %8.1f ms  device_ms %8.1f host_ms %8.1f  kernels: miller %.1f  f12 tree %.1f  g1 tree %.1f ms  batch_checks %d"
            % (lg, n / dt, dt * 1e3, st.device_ms, st.host_ms, ms[0], ms[1], ms[2], st.batch_checks))
        if lg in host_sizes:
            dt, st, _ = run(n, -1)
            say("N=2^%d device=-1   %9.0f proofs/s  wall %8.1f ms  (16 host threads)" % (lg, n / dt, dt * 1e3))
        if lg == 14:
            for label, bad in (("one bad", [n // 3]), ("1%% bad (%d)" % (n // 100), list(range(5, n, 100))[:n // 100])):
                dt, st, ms = run(n, a.device, bad)
                say("N=2^14 device, %-14s %9.0f proofs/s  wall %8.1f ms  batch_checks %d single_checks %d" % (label, n / dt, dt * 1e3, st.batch_checks, st.single_checks))
            dt, st, _ = run(n, -1, [n // 3])
            say("N=2^14 device=-1, one bad      %9.0f proofs/s  wall %8.1f ms  batch_checks %d single_checks %d" % (n / dt, dt * 1e3, st.batch_checks, st.single_checks))
    m = min(a.single_sample, len(pool))
    one = lambda i: L.groth16_verify(pool[i][0], pool[i][1], vk, None, 0)
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        res = list(ex.map(one, range(m)))
        dt = time.perf_counter() - t0
    assert not any(res)
    say("groth16_verify from 16 host threads: %9.0f proofs/s  (%d proofs, %.1f ms)" % (m / dt, m, dt * 1e3))
    for lg in [int(s) for s in a.sizes.split(",")]:
        n = 1 << lg
        nodes, t = n, n
        while nodes > 1:
            nodes = (nodes + 1) // 2
            t += nodes
        say("tree memory N=2^%d: %d nodes x (432 + 144) bytes = %.1f MB on the device and on the host" % (lg, t, t * 576 / 1e6))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
