#!/usr/bin/env python3
"""Measurements of the development setup (ug_setup_run, ug_generator_mul): what profiles/dev_setup.txt records.

    python tools/dev_setup_bench.py windows [log_n]            fixed-base A/B: every window width, G1 and G2, n = 2^log_n (20)
    python tools/dev_setup_bench.py setup <log> [<log> ...]    device setup of the squaring-chain circuit at 2^log, per phase
    python tools/dev_setup_bench.py host <log> [<log> ...]     the same on host threads (device = -1): the only comparator

The circuit is the squaring chain x_(i+1) = x_i * x_i with 2^log - 2 constraints (so that the rows and the two public rows fill
the domain), its last value the public output; the .r1cs bytes are laid out with numpy. Keys made here are TEST keys."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402

R = synth.R_MOD


def chain_r1cs(log_n):
    """wires: 0 one | 1 out | 2 x_0 | 3 .. : x_1 ..; row i: x_i * x_i = x_(i+1), the last into wire 1"""
    n = (1 << log_n) - 2
    rec = np.dtype([("na", "<u4"), ("wa", "<u4"), ("ca", "u1", 32), ("nb", "<u4"), ("wb", "<u4"), ("cb", "u1", 32),
                    ("nc", "<u4"), ("wc", "<u4"), ("cc", "u1", 32)])
    rows = np.zeros(n, dtype=rec)
    i = np.arange(n, dtype=np.uint32)
    for k in ("na", "nb", "nc"):
        rows[k] = 1
    rows["wa"] = rows["wb"] = i + 2
    rows["wc"] = i + 3
    rows["wc"][-1] = 1
    for k in ("ca", "cb", "cc"):
        rows[k][:, 0] = 1
    n_wires = n + 2
    import struct
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, 1, 0, n_wires - 2, n_wires, n)
    body = rows.tobytes()
    sec = lambda i, p: struct.pack("<IQ", i, len(p)) + p
    return b"r1cs" + struct.pack("<II", 1, 2) + sec(1, hdr) + sec(2, body)


def windows(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(0x5E7)
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x1f                                   # below 2^253 < r, otherwise full width
    data = s.tobytes()
    L = ug.load()
    print("fixed-base multiplication, n = 2^%d random scalars below 2^253; ms by stream events" % log_n)
    print("%-3s %-3s %8s %10s %10s %12s %12s" % ("grp", "c", "tables", "table MiB", "build ms", "mul ms", "M mul/s"))
    for g2 in (0, 1):
        rec = 128 if g2 else 64
        out = C.create_string_buffer(rec * n)
        ref = None
        for c in (8, 10, 11, 12, 13, 14, 15, 16):
            ms = (C.c_double * 2)()
            err = C.create_string_buffer(512)
            best = None
            for _ in range(3):
                if L.ug_generator_mul(0, g2, data, n, c, out, ms, err, 511) != 0:
                    raise RuntimeError(err.value.decode())
                if best is None or ms[1] < best[1]:
                    best = (ms[0], ms[1])
            head = out.raw[:rec * 1024]
            assert ref is None or head == ref, "widths disagree"
            ref = head
            tables = (255 + c - 1) // c
            print("%-3s %-3d %8d %10.1f %10.2f %12.2f %12.1f" % ("G2" if g2 else "G1", c, tables, tables * (1 << (c - 1)) * rec / 2 ** 20, best[0], best[1],
                                                                 n / best[1] / 1e3), flush=True)


def setup(logs, device):
    t = {k: str(pow(7, i + 1, R)) for i, k in enumerate(ug.TRAPDOOR_KEYS)}
    print("%s setup of the squaring chain; ms per phase (%s)" % ("device" if device >= 0 else "host-thread", " | ".join(ug.SETUP_PHASES)))
    for log_n in logs:
        t0 = time.time()
        r1cs = chain_r1cs(log_n)
        t0b = time.time()
        # (the C calls themselves, the key in one numpy buffer: ultragroth_amd.dev_setup copies it twice more)
        opt, keep = ug._setup_options(t, "groth16", 0, None)
        L = ug.load()
        err = C.create_string_buffer(512)
        zbytes, vmax, wrote, vlen = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        if L.ug_setup_size(C.byref(opt), r1cs, len(r1cs), C.byref(zbytes), C.byref(vmax), err, 511) != 0:
            raise RuntimeError(err.value.decode())
        t1 = time.time()
        zkey = np.empty(zbytes.value, dtype=np.uint8)
        vkey = C.create_string_buffer(vmax.value)
        raw = (C.c_double * len(ug.SETUP_PHASES))()
        if L.ug_setup_run(C.byref(opt), r1cs, len(r1cs), device, zkey.ctypes.data, zbytes.value, C.byref(wrote), vkey, vmax.value, C.byref(vlen), raw, err, 511) != 0:
            raise RuntimeError(err.value.decode())
        t2 = time.time()
        ms = dict(zip(ug.SETUP_PHASES, raw))
        print("2^%-2d  %s  | sum %.0f ms, ug_setup_run %.0f ms (size query before it %.0f ms, circuit laid out in %.1f s; zkey %.1f MiB)" % (
            log_n, " | ".join("%9.1f" % ms[k] for k in ug.SETUP_PHASES), sum(ms.values()), (t2 - t1) * 1e3, (t1 - t0b) * 1e3, t0b - t0,
            wrote.value / 2 ** 20), flush=True)
        del zkey, r1cs


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "windows":
        windows(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    elif what in ("setup", "host") and len(sys.argv) > 2:
        setup([int(a) for a in sys.argv[2:]], 0 if what == "setup" else -1)
    else:
        sys.exit(__doc__)
