#!/usr/bin/env python3
"""Measurements of the key check (ug_zkey_verify_run) and of the only route to the same answer that existed before it: what
profiles/zkey_verify.txt records.

    python tools/zkey_verify_bench.py verify <log> [<log> ...]           the whole call on the device at validate = 2 and 1: per phase
                                                                        (host clocks), the fold kernel (stream events) with its
                                                                        bytes per second, the peak of device memory
    python tools/zkey_verify_bench.py host <log> [<log> ...]             the same on host threads (device = -1), validate = 2
    python tools/zkey_verify_bench.py baseline <library> <log> [...]     making the key again with the KNOWN delta through
                                                                        <library>'s ug_setup_ptau_run (the parent commit's build
                                                                        of libultragroth_hip.so) and comparing the bytes

The circuit and the .ptau are setup_ptau_bench's: the squaring chain with its coefficients redrawn from the "real" mix, and a
.ptau whose read slices hold the valid points (seed + i) * G of ug_synth_points. Such a .ptau is not a ceremony's and not even
consistent, but the key ug_setup_ptau_run makes from it satisfies every relation of the check, which are linear in the slices:
the check answers "valid" and does the work it does for a real key. The inputs are made with the library under test in
every mode; only the timed calls of `baseline` go to <library>."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402
from setup_ptau_bench import fake_ptau, mixed_chain  # noqa: E402

R = synth.R_MOD
DELTA = pow(7, 77, R)


def make_key(L, r1cs, ptau, device=0):
    """(the key as a numpy array, seconds of the size query, seconds of the run) through library L"""
    opt = ug._SetupPtauOptions()
    opt.size, opt.validate, opt.contribute = C.sizeof(opt), 1, 1
    opt.delta = ug._le32(DELTA, "delta")
    err = C.create_string_buffer(512)
    zbytes, vmax, wrote, vlen = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    t0 = time.time()
    if L.ug_setup_ptau_size(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, C.byref(zbytes), C.byref(vmax), err, 511) != 0:
        raise RuntimeError(err.value.decode())
    t1 = time.time()
    zkey = np.empty(zbytes.value, dtype=np.uint8)
    vkey = C.create_string_buffer(vmax.value)
    raw = (C.c_double * len(ug.SETUP_PTAU_PHASES))()
    if L.ug_setup_ptau_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, device, zkey.ctypes.data, zbytes.value, C.byref(wrote),
                           vkey, vmax.value, C.byref(vlen), raw, err, 511) != 0:
        raise RuntimeError(err.value.decode())
    return zkey[:wrote.value], t1 - t0, time.time() - t1


def inputs(dev, log_n):
    t0 = time.time()
    r1cs = mixed_chain(log_n, "real")
    ptau = fake_ptau(dev, log_n)
    zkey, _, _ = make_key(ug.load(), r1cs, ptau)
    print("2^%d: inputs made in %.1f s (r1cs %.0f MiB, ptau %.0f MiB, zkey %.0f MiB)" % (
        log_n, time.time() - t0, len(r1cs) / 2 ** 20, ptau.size / 2 ** 20, zkey.size / 2 ** 20), flush=True)
    return r1cs, ptau, zkey


def verify(logs, device):
    dev = ug.Device(0)
    L = ug.load()
    print("%s key check of the squaring chain, mix real; ms per phase (%s)" % ("device" if device >= 0 else "host-thread", " | ".join(ug.ZKEY_VERIFY_PHASES)))
    for log_n in logs:
        r1cs, ptau, zkey = inputs(dev, log_n)
        terms = sum(ug.r1cs_info(r1cs)["terms"])
        n = 1 << log_n
        fold_bytes = terms * (32 + 4 + 32) + 3 * 4 * n + 8 * 32 * n      # coefficient + wire id + the gathered weight per term; offsets; the eight vectors
        for validate in ((2, 1) if device >= 0 else (2,)):
            for turn in range(2):
                opt = ug._ZkeyVerifyOptions()
                opt.size, opt.validate = C.sizeof(opt), validate
                rep = ug._ZkeyVerifyReport()
                raw = (C.c_double * len(ug.ZKEY_VERIFY_PHASES))()
                err = C.create_string_buffer(512)
                t0 = time.time()
                rc = L.ug_zkey_verify_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, zkey.ctypes.data, zkey.size, device,
                                          C.byref(rep), raw, err, 511)
                wall = time.time() - t0
                if rc != 0:
                    raise RuntimeError("rc %d: %s" % (rc, err.value.decode()))
                print("2^%-2d validate %d run %d  %s  | ug_zkey_verify_run %.0f ms; fold kernel %.3f ms = %.0f GB/s over %.0f MiB; "
                      "peak device memory %.0f MiB; subgroup checked: %d" % (
                          log_n, validate, turn, " | ".join("%8.1f" % v for v in raw), wall * 1e3, rep.fold_kernel_ms,
                          fold_bytes / max(rep.fold_kernel_ms, 1e-9) / 1e6, fold_bytes / 2 ** 20, rep.peak_device_bytes / 2 ** 20,
                          rep.subgroup_checked), flush=True)
        del r1cs, ptau, zkey
    dev.close()


def baseline(path, logs):
    dev = ug.Device(0)
    P = C.CDLL(os.path.abspath(path))
    vp, u64 = C.c_void_p, C.c_uint64
    P.ug_setup_ptau_size.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, C.c_ulonglong]
    P.ug_setup_ptau_run.argtypes = [vp, vp, u64, vp, u64, C.c_int, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), C.POINTER(C.c_double), vp, C.c_ulonglong]
    print("baseline through %s: the key made again with the known delta (ug_setup_ptau_size + ug_setup_ptau_run, validate = 1), then compared byte for byte" % path)
    for log_n in logs:
        r1cs, ptau, zkey = inputs(dev, log_n)
        for turn in range(2):
            again, size_s, run_s = make_key(P, r1cs, ptau)
            t0 = time.time()
            same = again.size == zkey.size and np.array_equal(again, zkey)
            cmp_s = time.time() - t0
            print("2^%-2d run %d  size query %.0f ms + run %.0f ms + compare %.0f ms = %.0f ms; same key: %s" % (
                log_n, turn, size_s * 1e3, run_s * 1e3, cmp_s * 1e3, (size_s + run_s + cmp_s) * 1e3, same), flush=True)
            del again
        del r1cs, ptau, zkey
    dev.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what in ("verify", "host") and len(sys.argv) > 2:
        verify([int(a) for a in sys.argv[2:]], 0 if what == "verify" else -1)
    elif what == "baseline" and len(sys.argv) > 3:
        baseline(sys.argv[2], [int(a) for a in sys.argv[3:]])
    else:
        sys.exit(__doc__)
