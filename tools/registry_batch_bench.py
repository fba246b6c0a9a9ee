#!/usr/bin/env python3
"""Times what the registry's batched call and the one-launch witness check of a pass change (profiles/registry_batch.txt).

    python tools/registry_batch_bench.py --check 20,22 [--parent-lib PATH] [--width 8] [--reps 7]
    python tools/registry_batch_bench.py --provers g16:16,g16:20,ultra:16 [--parent-tree DIR] [--rounds 3] [--k 8]

--check: on the satisfied circuit of tools/witness_check_bench.py (2^log constraints), `width` copies of the witness side by side:
ONE r1cs_check_vectors_kernel launch (device_ms of ug_r1cs_check_vectors; UG_R1CS_VT = 4, 2 and 1 in turn) against `width` launches
of the single kernel (the sum of device_ms of ug_r1cs_check) -- of this build and, with --parent-lib, of the parent commit's library
loaded beside it, in alternating turns. Median and min .. max of --reps turns after one warm-up.
--provers: per circuit (g16 / ultra : log2 domain, synthetic, ultragroth_amd/synth.py) and round, one child process per build --
the parent commit's checkout (--parent-tree, its own package and library) and this one -- each: a single created-prover proof,
k Registry.prove singles, and on this build Registry.prove_batch of the k witnesses and the created prover's prove_batch beside it.
Milliseconds per proof, host wall, median of --steps calls after a warm-up call of each kind. One JSON line per child."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("UG_BENCH_TREE") or os.path.dirname(HERE))
sys.path.insert(1, HERE)
import ultragroth_amd as ug                      # noqa: E402
from ultragroth_amd import synth                 # noqa: E402


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


class ParentCheck:
    """the parent library's single check on its own context: ug_r1cs_create, the witness in a vector of its own, ug_r1cs_check"""

    def __init__(self, path, r1cs, values, n_wires):
        L = self.L = C.CDLL(os.path.abspath(path))
        vp, u64 = C.c_void_p, C.c_uint64
        L.ug_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
        L.ug_dvec_create.argtypes = [vp, u64, C.POINTER(vp)]
        L.ug_dvec_upload.argtypes = [vp, vp, u64]
        L.ug_r1cs_create.argtypes = [vp, vp, u64, C.POINTER(vp)]
        L.ug_r1cs_check.argtypes = [vp, vp, u64, vp, vp]
        self.ctx, self.vec, self.cs = vp(), vp(), vp()
        assert L.ug_ctx_create(C.byref(self.ctx), 0) == 0
        assert L.ug_dvec_create(self.ctx, n_wires, C.byref(self.vec)) == 0
        assert L.ug_dvec_upload(self.vec, values, n_wires) == 0
        assert L.ug_r1cs_create(self.ctx, r1cs, len(r1cs), C.byref(self.cs)) == 0

    def check_ms(self):
        rep = ug._R1csReport()
        assert self.L.ug_r1cs_check(self.cs, self.vec, 0, C.byref(rep), None) == 0 and rep.failed == 0
        return rep.device_ms


def check(log_m, width, reps, parent_lib):
    import witness_check_bench as W
    r1cs, _, values, terms = W.build(log_m, 1)
    n = ug.r1cs_info(r1cs)["n_wires"]
    dev = ug.Device(0)
    cs = dev.r1cs(r1cs)
    vec = dev.dvec(width * n, values * width)
    parent = ParentCheck(parent_lib, r1cs, values, n) if parent_lib else None
    turns = {"vectors_vt4": [], "vectors_vt2": [], "vectors_vt1": [], "singles_this": [], "singles_parent": []}
    for rep in range(reps + 1):
        row = {}
        for vt in (4, 2, 1):
            os.environ["UG_R1CS_VT"] = str(vt)
            got = cs.check_vectors(vec, width)
            assert all(g["failed"] == 0 for g in got)
            row["vectors_vt%d" % vt] = got[0]["device_ms"]
        os.environ.pop("UG_R1CS_VT")
        row["singles_this"] = sum(cs.check(vec, first=v * n)["device_ms"] for v in range(width))
        if parent:
            row["singles_parent"] = sum(parent.check_ms() for _ in range(width))
        if rep:                                                    # (turn 0 warms up)
            for key, ms in row.items():
                turns[key].append(ms)
    print(json.dumps({"check_log_constraints": log_m, "width": width, "terms": terms,
                      **{key: stats(ms) for key, ms in turns.items() if ms}}), flush=True)
    cs.close()
    dev.close()


def witnesses(kind, log, k):
    if kind == "ultra":
        return synth.build_ultra_witnesses(log, k)
    return [synth.build_witness(log, "UC"[b % 2], seed=0x7000 + 16 * b) for b in range(k)]


def child(kind, log, zkey_path, k, steps, batched):
    zkey = open(zkey_path, "rb").read()
    wtns = witnesses(kind, log, k)
    res = {"circuit": "%s:%d" % (kind, log), "tree": os.environ.get("UG_BENCH_TREE") or "this"}

    def timed(fn, per):
        fn()
        out = []
        for _ in range(steps):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3 / per)
        return stats(out)

    with (ug.UltraGrothProver if kind == "ultra" else ug.Groth16Prover)(zkey) as p:
        if kind != "ultra":
            p.tables_ready(wait=True)
        res["created_single_ms"] = timed(lambda: p.prove(wtns[0]), 1)
        if batched:
            res["created_batch_ms_per_proof"] = timed(lambda: p.prove_batch(wtns), k)
            res["created_batch_info"] = p.batch_info()
    with ug.Registry(0) as reg:
        reg.load("c", zkey)
        res["registry_singles_ms_per_proof"] = timed(lambda: [reg.prove("c", w) for w in wtns], k)
        if batched:
            res["registry_batch_ms_per_proof"] = timed(lambda: reg.prove_batch("c", wtns), k)
            res["registry_batch_info"] = reg.batch_info("c")
            res["registry_state"] = reg.info("c")[1]
    print(json.dumps(res), flush=True)


def provers(spec, parent_tree, rounds, k, steps, tmp):
    kind, log = spec.split(":")
    log = int(log)
    dev = ug.Device(0)
    zkey = (synth.build_ultra_circuit(dev, log) if kind == "ultra" else synth.build_circuit(dev, log))[0]
    dev.close()
    path = os.path.join(tmp, "rbb_%s_%d.zkey" % (kind, log))
    with open(path, "wb") as f:
        f.write(zkey)
    del zkey
    try:
        for _ in range(rounds):
            for tree in ([parent_tree] if parent_tree else []) + [""]:
                env = dict(os.environ)
                if tree:
                    env["UG_BENCH_TREE"] = tree
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(log), path, "--k", str(k), "--steps", str(steps)]
                                   + ([] if tree else ["--batched"]), env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError("child %s failed (%d): %s" % (tree or "this", r.returncode, r.stderr[-800:]))
                print(r.stdout.strip().splitlines()[-1], flush=True)
    finally:
        os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", default="", help="log2 constraint counts, e.g. 20,22")
    ap.add_argument("--parent-lib", default="", help="--check: the parent commit's libultragroth_hip.so, its single check in the same turns")
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--provers", default="", help="e.g. g16:16,g16:20,ultra:16")
    ap.add_argument("--parent-tree", default="", help="--provers: a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--batched", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=3, metavar=("KIND", "LOG", "ZKEY"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.child[2], a.k, a.steps, a.batched)
        return
    for log_m in [int(x) for x in a.check.split(",") if x]:
        check(log_m, a.width, a.reps, a.parent_lib)
    for spec in [x for x in a.provers.split(",") if x]:
        provers(spec, a.parent_tree, a.rounds, a.k, a.steps, a.tmp)


if __name__ == "__main__":
    main()
