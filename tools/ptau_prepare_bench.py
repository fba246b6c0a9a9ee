#!/usr/bin/env python3
"""Measurements of the powers-of-tau preparation (ug_ptau_prepare_run, ug_points_intt): what profiles/ptau_prepare.txt records.

    python tools/ptau_prepare_bench.py kernels <g1|g2> <log> [<log> ...]   one transform of 2^log points, ms by stream events (the
                                                                          1 / N products | the stages), and beside it, in the same
                                                                          process, points_combine of 3 * 2^(log-2) full-length
                                                                          terms: term_products_kernel's rate on this device
    python tools/ptau_prepare_bench.py file <path> <power>                 writes an UNPREPARED synthetic file of that power
    python tools/ptau_prepare_bench.py run <path> <out> [tool arguments]   the ptau_prepare tool on it, a child process: input and
                                                                          output mapped, phase times as the tool prints them

The file is NOT a ceremony's and not even consistent: sections 2 - 5 hold the valid curve points (seed + i) * G of
ug_synth_points. The sections made from it mean nothing; the work is the same: every point passes the check, every butterfly is
a full-length product and two real additions."""
import ctypes as C
import os
import struct
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402
from setup_ptau_bench import coefficients  # noqa: E402


def walks(log_n):
    """butterflies of a transform whose twiddle is not 1: stage s >= 1 has 2^(log_n-1) lanes, one in every 2^s without a walk"""
    half = 1 << (log_n - 1)
    return sum(half - (half >> s) for s in range(1, log_n))


def kernels(g2, logs):
    dev = ug.Device(0)
    L = ug.load()
    err = C.create_string_buffer(512)
    rec = 128 if g2 else 64
    name = "G2" if g2 else "G1"
    for log_n in [8] + logs:                     # (2^8 first: code objects loaded, nothing printed)
        n = 1 << log_n
        pts = np.empty(n * rec, dtype=np.uint8)
        synth.synth_points(dev, n, 0x99, g2=g2, out=memoryview(pts))
        out = np.empty(n * rec, dtype=np.uint8)
        best = None
        for _ in range(2):
            ms = (C.c_double * 2)()
            if L.ug_points_intt(0, int(g2), log_n, pts.ctypes.data, n, out.ctypes.data, ms, err, 511) != 0:
                raise RuntimeError(err.value.decode())
            if best is None or ms[1] < best[1]:
                best = (ms[0], ms[1])
        # the product kernel alone on the same points: 2^(log-2) columns of three full-length terms
        cols = max(n // 4, 1)
        col_ptr = (np.arange(cols + 1, dtype=np.uint64) * 3).astype(np.uint32)
        index = np.random.default_rng(1).integers(0, n, size=3 * cols, dtype=np.uint32)
        co = coefficients(3 * cols, "full", 7)
        cout = np.empty(cols * rec, dtype=np.uint8)
        prod = None
        for _ in range(2):
            ms = (C.c_double * 2)()
            if L.ug_points_combine(0, int(g2), col_ptr.ctypes.data, cols, index.ctypes.data, co.ctypes.data, pts.ctypes.data, n, cout.ctypes.data, ms, err, 511) != 0:
                raise RuntimeError(err.value.decode())
            prod = ms[0] if prod is None else min(prod, ms[0])
        if log_n == 8 and 8 not in logs:
            continue
        flies, w = (n // 2) * log_n, walks(log_n)
        print("%s 2^%-2d  1/N products %9.2f ms (%.1f M points/s, %d-bit scalar) | %2d stages %10.2f ms: %.2f M butterflies/s, %.2f M/s "
              "counting only the %d with a product | term_products_kernel, %d full-length terms: %9.2f ms, %.2f M products/s" % (
                  name, log_n, best[0], n / best[0] / 1e3, 254 - log_n, log_n, best[1], flies / best[1] / 1e3, w / best[1] / 1e3, w,
                  3 * cols, prod, 3 * cols / prod / 1e3), flush=True)
    dev.close()


def make_file(path, power):
    dev = ug.Device(0)
    n = 1 << power
    sizes = [(1, 44), (2, 64 * (2 * n - 1)), (3, 128 * n), (4, 64 * n), (5, 64 * n), (6, 128), (7, 4)]
    total = 12 + sum(12 + s for _, s in sizes)
    t0 = time.time()
    buf = np.memmap(path, dtype=np.uint8, mode="w+", shape=(total,))
    buf[:12] = np.frombuffer(b"ptau" + struct.pack("<II", 1, len(sizes)), dtype=np.uint8)
    at, where = 12, {}
    for sid, size in sizes:
        buf[at:at + 12] = np.frombuffer(struct.pack("<IQ", sid, size), dtype=np.uint8)
        where[sid] = at + 12
        at += 12 + size
    put = lambda sid, data: buf.__setitem__(slice(where[sid], where[sid] + len(data)), np.frombuffer(data, dtype=np.uint8))
    put(1, struct.pack("<I", 32) + synth.Q_MOD.to_bytes(32, "little") + struct.pack("<II", power, power))
    put(6, synth.g2_generator_record())
    for sid, g2, seed, count in ((2, False, 0x11, 2 * n - 1), (3, True, 0x22, n), (4, False, 0x33, n), (5, False, 0x44, n)):
        rec = 128 if g2 else 64
        piece = 1 << 22                          # (bounded pieces: the points are made in a host array, then copied into the map)
        for first in range(0, count, piece):
            m = min(piece, count - first)
            tmp = np.empty(m * rec, dtype=np.uint8)
            synth.synth_points(dev, m, seed + first, g2=g2, out=memoryview(tmp))
            buf[where[sid] + first * rec:where[sid] + (first + m) * rec] = tmp
    buf.flush()
    del buf
    dev.close()
    print("unprepared synthetic file of power %d: %.0f MiB, written in %.1f s" % (power, total / 2 ** 20, time.time() - t0), flush=True)


def run_tool(path, out, more):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultragroth_amd", "csrc", "ptau_prepare")
    t0 = time.time()
    r = subprocess.run([exe, path, out] + more, capture_output=True, text=True)
    print("ptau_prepare %s: exit %d, %.2f s wall (the process, with the mapping of both files and the device's start)" % (
        " ".join(more), r.returncode, time.time() - t0))
    print((r.stdout + r.stderr).strip(), flush=True)
    if r.returncode:
        sys.exit(1)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernels" and len(sys.argv) > 3 and sys.argv[2] in ("g1", "g2"):
        kernels(sys.argv[2] == "g2", [int(a) for a in sys.argv[3:]])
    elif what == "file" and len(sys.argv) == 4:
        make_file(sys.argv[2], int(sys.argv[3]))
    elif what == "run" and len(sys.argv) >= 4:
        run_tool(sys.argv[2], sys.argv[3], sys.argv[4:])
    else:
        sys.exit(__doc__)
