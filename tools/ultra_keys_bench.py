#!/usr/bin/env python3
"""Measurements of the UltraGroth phase-2 setup (ug_ultra_setup_ptau_run, ug_points_scale_segments): what profiles/ultra_keys.txt
records.

    python tools/ultra_keys_bench.py setup <mix> <log> [<log> ...]    ug_ultra_setup_ptau_run and, on the same files in the same
                                                                     process, ug_setup_ptau_run: whole call and phases; then the
                                                                     two checks, ug_ultra_zkey_verify_run and ug_zkey_verify_run,
                                                                     on the keys just made; then the delta step's kernel alone
                                                                     (scale_segments_kernel over the key's three segments,
                                                                     stream events) beside scale_kernel
    python tools/ultra_keys_bench.py one <mix> <log> <out.json>      ONE run of both protocols' calls, setup_from_ptau then
                                                                     zkey_verify and ultra_setup_from_ptau then ultra_zkey_verify
                                                                     (validate 1), with the package and library of the checkout
                                                                     that ULTRAGROTH_TREE names (default: this one): times, the
                                                                     keys' SHA-256, the verdicts and the checks' peak device bytes
    python tools/ultra_keys_bench.py ab <mix> <log> <tree_a> <tree_b> [runs]
                                                                     the `one` run in fresh child processes, two built
                                                                     checkouts (a parent commit's and this one) alternating,
                                                                     `runs` (3) times each; says per protocol whether the key,
                                                                     the verdict and the peak device bytes agree across all runs

The circuit, the coefficient mixes and the .ptau are setup_ptau_bench's (the squaring chain; a .ptau of valid points that is
not a ceremony's). The spec: rand_indx = 1 (the chain's one public signal), the private wires alternating between the rounds."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ULTRAGROTH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402
from setup_ptau_bench import MIXES, fake_ptau, mixed_chain  # noqa: E402

R = synth.R_MOD
DELTAS = (pow(7, 77, R), pow(11, 55, R))


def _check(rc, err):
    if rc != 0:
        raise RuntimeError(err.value.decode())


def run_setup(L, opt, size_fn, run_fn, r1cs, ptau, device):
    """(whole-call ms, phase ms, zkey as a numpy array)"""
    err = C.create_string_buffer(512)
    zbytes, vmax, wrote, vlen = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(size_fn(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, C.byref(zbytes), C.byref(vmax), err, 511), err)
    zkey = np.empty(zbytes.value, dtype=np.uint8)
    vkey = C.create_string_buffer(vmax.value)
    raw = (C.c_double * len(ug.SETUP_PTAU_PHASES))()
    t0 = time.time()
    _check(run_fn(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, device, zkey.ctypes.data, zbytes.value, C.byref(wrote), vkey,
                  vmax.value, C.byref(vlen), raw, err, 511), err)
    return (time.time() - t0) * 1e3, list(raw), zkey[:wrote.value]


def groth16_options():
    opt = ug._SetupPtauOptions()
    opt.size, opt.validate, opt.contribute = C.sizeof(opt), 1, 1
    opt.delta = ug._le32(DELTAS[1], "delta")
    return opt


def ultra_options(log_n):
    """the options of the UltraGroth setup and the two lists they point into (keep them alive)"""
    private = np.arange(2, 1 << log_n, dtype=np.uint32)
    lists = (np.ascontiguousarray(private[1::2]), np.ascontiguousarray(private[0::2]))
    uopt = ug._UltraSetupPtauOptions()
    uopt.size, uopt.validate, uopt.contribute, uopt.rand_indx = C.sizeof(uopt), 1, 1, 1
    uopt.delta_round, uopt.delta_final = ug._le32(DELTAS[0], "d"), ug._le32(DELTAS[1], "d")
    uopt.round_signals = lists[0].ctypes.data_as(C.POINTER(C.c_uint32)); uopt.n_round = lists[0].size
    uopt.final_signals = lists[1].ctypes.data_as(C.POINTER(C.c_uint32)); uopt.n_final = lists[1].size
    return uopt, lists


def setup(mix, logs):
    dev = ug.Device(0)
    L = ug.load()
    print("mix %s, deltas given, validate 1; ms: whole call | %s" % (mix, " | ".join(ug.SETUP_PTAU_PHASES)))
    print("the checks: validate 2; ms: whole call | %s" % " | ".join(ug.ZKEY_VERIFY_PHASES))
    for log_n in logs:
        r1cs = mixed_chain(log_n, mix)
        ptau = fake_ptau(dev, log_n)
        uopt, lists = ultra_options(log_n)
        keys = {}
        for name, opt, fns in (("ultra_setup_from_ptau", uopt, (L.ug_ultra_setup_ptau_size, L.ug_ultra_setup_ptau_run)),
                               ("setup_from_ptau", groth16_options(), (L.ug_setup_ptau_size, L.ug_setup_ptau_run)),
                               ("ultra_setup_from_ptau", uopt, (L.ug_ultra_setup_ptau_size, L.ug_ultra_setup_ptau_run)),
                               ("setup_from_ptau", groth16_options(), (L.ug_setup_ptau_size, L.ug_setup_ptau_run))):
            whole, raw, zkey = run_setup(L, opt, fns[0], fns[1], r1cs, ptau, 0)
            print("2^%-2d %-22s %9.1f | %s   (zkey %.0f MiB)" % (log_n, name, whole, " | ".join("%9.1f" % v for v in raw), zkey.size / 2 ** 20), flush=True)
            keys[name] = zkey
        # the two checks on the keys just made, validate = 2; twice each, alternating
        spec = {"rand_indx": 1, "round_signals": lists[0], "final_signals": lists[1]}
        for turn in range(2):
            for name, call in (("ultra_zkey_verify", lambda t: ug.ultra_zkey_verify(r1cs, memoryview(ptau), memoryview(keys["ultra_setup_from_ptau"]), device=0, timings=t)),
                               ("ultra_zkey_verify+spec", lambda t: ug.ultra_zkey_verify(r1cs, memoryview(ptau), memoryview(keys["ultra_setup_from_ptau"]), ultra=spec, device=0, timings=t)),
                               ("zkey_verify", lambda t: ug.zkey_verify(r1cs, memoryview(ptau), memoryview(keys["setup_from_ptau"]), device=0, timings=t))):
                t = {}
                t0 = time.time()
                verdict = call(t)
                whole = (time.time() - t0) * 1e3
                print("2^%-2d %-22s %9.1f | %s | fold kernel %.3f ms, peak device memory %.0f MiB, verdict %s" % (
                    log_n, name, whole, " | ".join("%9.1f" % t[k] for k in ug.ZKEY_VERIFY_PHASES), t["fold_kernel"], t["peak_device_bytes"] / 2 ** 20,
                    "valid" if verdict is None else verdict[:2]), flush=True)
        keys.clear()
        # the delta step's kernels alone, over points of the key's counts
        n = 1 << log_n
        pts = np.empty(n * 64, dtype=np.uint8)
        synth.synth_points(dev, n, 0x77, out=memoryview(pts))
        err = C.create_string_buffer(512)
        scal = [d.to_bytes(32, "little") for d in DELTAS]
        segs = (ug._ScaleSegment * 3)()
        keep = [C.create_string_buffer(s, 32) for s in scal]
        for i, (sc, idx, count) in enumerate(((keep[0], lists[0], lists[0].size), (keep[1], lists[1], lists[1].size), (keep[1], None, n))):
            segs[i].scalar = C.cast(sc, C.c_void_p)
            if idx is not None:
                segs[i].index = idx.ctypes.data_as(C.POINTER(C.c_uint32))
            segs[i].count = count
        total = int(lists[0].size + lists[1].size + n)
        out = np.empty(total * 64, dtype=np.uint8)
        best = None
        for _ in range(3):
            ms = (C.c_double * 1)()
            _check(L.ug_points_scale_segments(0, 3, segs, pts.ctypes.data, n, out.ctypes.data, ms, err, 511), err)
            best = ms[0] if best is None else min(best, ms[0])
        print("2^%-2d scale_segments_kernel, %d + %d gathered + %d records, two scalars: %.2f ms, %.1f M points/s" % (
            log_n, lists[0].size, lists[1].size, n, best, total / best / 1e3), flush=True)
        one = None
        out1 = np.empty(n * 64, dtype=np.uint8)
        for _ in range(3):
            ms = (C.c_double * 1)()
            _check(L.ug_points_scale(0, scal[1], pts.ctypes.data, n, out1.ctypes.data, ms, err, 511), err)
            one = ms[0] if one is None else min(one, ms[0])
        print("2^%-2d scale_kernel, %d records, one scalar: %.2f ms, %.1f M points/s" % (log_n, n, one, n / one / 1e3), flush=True)
        del ptau, r1cs, pts, out, out1
    dev.close()


def one(mix, log_n, out_path):
    dev = ug.Device(0)
    L = ug.load()
    r1cs = mixed_chain(log_n, mix)
    ptau = fake_ptau(dev, log_n)
    uopt, lists = ultra_options(log_n)
    res = {"tree": os.path.dirname(os.path.dirname(os.path.abspath(ug.__file__)))}
    for name, opt, fns, check in (
            ("groth16", groth16_options(), (L.ug_setup_ptau_size, L.ug_setup_ptau_run),
             lambda key, t: ug.zkey_verify(r1cs, memoryview(ptau), memoryview(key), device=0, validate=1, timings=t)),
            ("ultra", uopt, (L.ug_ultra_setup_ptau_size, L.ug_ultra_setup_ptau_run),
             lambda key, t: ug.ultra_zkey_verify(r1cs, memoryview(ptau), memoryview(key), device=0, validate=1, timings=t))):
        whole, raw, zkey = run_setup(L, opt, fns[0], fns[1], r1cs, ptau, 0)
        timings = {}
        t0 = time.time()
        verdict = check(zkey, timings)
        verify_ms = (time.time() - t0) * 1e3
        res[name] = {"setup_ms": whole, "setup_phases": raw, "zkey_sha256": hashlib.sha256(zkey.tobytes()).hexdigest(),
                     "verify_ms": verify_ms, "verify_phases": [timings[k] for k in ug.ZKEY_VERIFY_PHASES],
                     "peak_device_bytes": int(timings["peak_device_bytes"]),
                     "verdict": None if verdict is None else [verdict[0], list(verdict[1]), verdict[2]]}
        del zkey
    with open(out_path, "w") as f:
        json.dump(res, f)
    dev.close()


SAME = ("zkey_sha256", "verdict", "peak_device_bytes")      # what both checkouts must agree on, per protocol


def ab(mix, log_n, lib_a, lib_b, runs):
    rows = {lib_a: [], lib_b: []}
    fd, path = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    for turn in range(runs):
        for lib in (lib_a, lib_b):
            env = dict(os.environ, ULTRAGROTH_TREE=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "one", mix, str(log_n), path], env=env, check=True, timeout=900)
            res = json.load(open(path))
            assert os.path.samefile(res["tree"], lib), res["tree"]
            rows[lib].append(res)
            for proto in ("groth16", "ultra"):
                r = res[proto]
                print("turn %d %-40s %-7s setup %9.1f ms  verify %9.1f ms  zkey %s  verdict %s  peak %d bytes" % (
                    turn, lib[-40:], proto, r["setup_ms"], r["verify_ms"], r["zkey_sha256"][:16], r["verdict"], r["peak_device_bytes"]), flush=True)
                print("        setup phases  %s" % " ".join("%.1f" % v for v in r["setup_phases"]))
                print("        verify phases %s" % " ".join("%.1f" % v for v in r["verify_phases"]), flush=True)
    for proto in ("groth16", "ultra"):
        for lib in (lib_a, lib_b):
            s = [r[proto]["setup_ms"] for r in rows[lib]]
            v = [r[proto]["verify_ms"] for r in rows[lib]]
            print("%-40s %-7s setup min %.1f max %.1f | verify min %.1f max %.1f" % (lib[-40:], proto, min(s), max(s), min(v), max(v)))
        for what in SAME:
            same = len({json.dumps(r[proto][what]) for lib in rows for r in rows[lib]}) == 1
            print("%-7s %s identical across both checkouts and all runs: %s" % (proto, what, same))
    os.unlink(path)


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 3 and a[0] == "setup" and a[1] in MIXES:
        setup(a[1], [int(x) for x in a[2:]])
    elif len(a) == 4 and a[0] == "one" and a[1] in MIXES:
        one(a[1], int(a[2]), a[3])
    elif len(a) in (5, 6) and a[0] == "ab" and a[1] in MIXES:
        ab(a[1], int(a[2]), a[3], a[4], int(a[5]) if len(a) == 6 else 3)
    else:
        sys.exit(__doc__)
