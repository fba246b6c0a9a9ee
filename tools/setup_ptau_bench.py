#!/usr/bin/env python3
"""Measurements of the phase-2 setup from a .ptau (ug_setup_ptau_run, ug_points_combine, ug_points_scale): what
profiles/setup_ptau.txt records.

    python tools/setup_ptau_bench.py kernels <log> [<log> ...]        the two kernels alone: combinations of 2^log columns with
                                                                     three terms each under four coefficient mixes, G1 and G2,
                                                                     and one scalar times 2^log points; ms by stream events
    python tools/setup_ptau_bench.py setup <mix> <log> [<log> ...]    the whole call on the device, per phase (host clocks)
    python tools/setup_ptau_bench.py host <mix> <log> [<log> ...]     the same on host threads (device = -1)

Mixes (the share of a term's coefficient classes): unit = 1 and r - 1 only; real = 90 % 1, 6 % r - 1, 3 % below 2^16, 1 % full
length (what a circom circuit looks like); fifth = 80 % unit, 20 % full length; full = every term at full length.
The circuit is dev_setup_bench's squaring chain with its coefficients redrawn from the mix (it is then no longer satisfiable:
a setup never looks at a witness). The .ptau is NOT a ceremony's and not even consistent: its read slices are filled with the
valid curve points (seed + i) * G of ug_synth_points, the levels nobody reads stay zero. The key is meaningless, the work is
the same: every point passes the check and every addition is a real one."""
import ctypes as C
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402
from dev_setup_bench import chain_r1cs  # noqa: E402

R = synth.R_MOD
MIXES = {"unit": (0.5, 0.5, 0.0, 0.0), "real": (0.90, 0.06, 0.03, 0.01), "fifth": (0.5, 0.3, 0.0, 0.2), "full": (0.0, 0.0, 0.0, 1.0)}


def coefficients(n, mix, seed):
    """n x 32 bytes: plain little-endian coefficients below r drawn from the mix (1 | r - 1 | below 2^16 | full length)"""
    rng = np.random.default_rng(seed)
    cls = rng.choice(4, size=n, p=MIXES[mix])
    out = np.zeros((n, 32), dtype=np.uint8)
    out[cls == 0, 0] = 1
    out[cls == 1] = np.frombuffer((R - 1).to_bytes(32, "little"), dtype=np.uint8)
    small = cls == 2
    out[small, :2] = rng.integers(2, 256, size=(int(small.sum()), 2), dtype=np.uint8)
    full = cls == 3
    out[full] = rng.integers(0, 256, size=(int(full.sum()), 32), dtype=np.uint8)
    out[full, 31] = (out[full, 31] & 0x0f) | 0x10          # 2^252 <= value < 2^253 < r: 251 - 253 bits after the fold at r / 2
    return out


def mixed_chain(log_n, mix):
    """the squaring chain's .r1cs with every coefficient redrawn"""
    data = bytearray(chain_r1cs(log_n))
    n = (1 << log_n) - 2
    body = len(data) - n * 120                               # a row: three times (u32 count = 1 | u32 wire | 32-byte coefficient)
    rows = np.frombuffer(data, dtype=np.uint8, count=n * 120, offset=body).reshape(n, 120)
    co = coefficients(3 * n, mix, 0xC0EF + log_n).reshape(n, 3, 32)
    for k in range(3):
        rows[:, 40 * k + 8:40 * k + 40] = co[:, k]
    return bytes(data)


def fake_ptau(dev, log_n):
    """a .ptau of power log_n whose read slices hold valid points (level log_n of sections 12 - 15, level log_n + 1 of 12)"""
    n = 1 << log_n
    sizes = [(1, 44), (2, 64), (3, 128), (4, 64), (5, 64), (6, 128), (7, 4), (12, 64 * (4 * n - 1)), (13, 128 * (2 * n - 1)),
             (14, 64 * (2 * n - 1)), (15, 64 * (2 * n - 1))]
    buf = np.zeros(12 + sum(12 + s for _, s in sizes), dtype=np.uint8)
    buf[:12] = np.frombuffer(b"ptau" + struct.pack("<II", 1, len(sizes)), dtype=np.uint8)
    at, where = 12, {}
    for sid, size in sizes:
        buf[at:at + 12] = np.frombuffer(struct.pack("<IQ", sid, size), dtype=np.uint8)
        where[sid] = at + 12
        at += 12 + size
    put = lambda sid, off, data: buf.__setitem__(slice(where[sid] + off, where[sid] + off + len(data)), np.frombuffer(data, dtype=np.uint8))
    put(1, 0, struct.pack("<I", 32) + synth.Q_MOD.to_bytes(32, "little") + struct.pack("<II", log_n, log_n))
    put(4, 0, synth.g1_generator_record()); put(5, 0, synth.g1_generator_record()); put(6, 0, synth.g2_generator_record())
    for sid, g2, seed, count, first in ((12, False, 0x11, 3 * n, n - 1), (13, True, 0x22, n, n - 1), (14, False, 0x33, n, n - 1), (15, False, 0x44, n, n - 1)):
        rec = 128 if g2 else 64
        synth.synth_points(dev, count, seed, g2=g2, out=memoryview(buf)[where[sid] + first * rec:where[sid] + (first + count) * rec])
    return buf


def setup(mix, logs, device):
    print("%s phase-2 setup of the squaring chain, mix %s, delta given; ms per phase (%s)" % (
        "device" if device >= 0 else "host-thread", mix, " | ".join(ug.SETUP_PTAU_PHASES)))
    dev = ug.Device(0)
    L = ug.load()
    for log_n in logs:
        t0 = time.time()
        r1cs = mixed_chain(log_n, mix)
        ptau = fake_ptau(dev, log_n)
        t1 = time.time()
        opt = ug._SetupPtauOptions()
        opt.size, opt.validate, opt.contribute = C.sizeof(opt), 1, 1
        opt.delta = ug._le32(pow(7, 77, R), "delta")
        err = C.create_string_buffer(512)
        zbytes, vmax, wrote, vlen = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        if L.ug_setup_ptau_size(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, C.byref(zbytes), C.byref(vmax), err, 511) != 0:
            raise RuntimeError(err.value.decode())
        t2 = time.time()
        zkey = np.empty(zbytes.value, dtype=np.uint8)
        vkey = C.create_string_buffer(vmax.value)
        raw = (C.c_double * len(ug.SETUP_PTAU_PHASES))()
        if L.ug_setup_ptau_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, device, zkey.ctypes.data, zbytes.value, C.byref(wrote),
                               vkey, vmax.value, C.byref(vlen), raw, err, 511) != 0:
            raise RuntimeError(err.value.decode())
        t3 = time.time()
        print("2^%-2d  %s  | ug_setup_ptau_run %.0f ms (size query %.0f ms, inputs made in %.1f s; ptau %.0f MiB, zkey %.0f MiB)" % (
            log_n, " | ".join("%9.1f" % v for v in raw), (t3 - t2) * 1e3, (t2 - t1) * 1e3, t1 - t0, ptau.size / 2 ** 20, wrote.value / 2 ** 20), flush=True)
        del zkey, ptau, r1cs
    dev.close()


def kernels(logs):
    dev = ug.Device(0)
    L = ug.load()
    err = C.create_string_buffer(512)
    print("combinations of 2^log columns, three terms each over 2^log points; ms by stream events (products | sums); M terms/s over both")
    for log_n in logs:
        n = 1 << log_n
        col_ptr = (np.arange(n + 1, dtype=np.uint64) * 3).astype(np.uint32)
        index = np.random.default_rng(1).integers(0, n, size=3 * n, dtype=np.uint32)
        for g2 in (0, 1):
            rec = 128 if g2 else 64
            pts = np.empty(n * rec, dtype=np.uint8)
            synth.synth_points(dev, n, 0x99, g2=bool(g2), out=memoryview(pts))
            out = np.empty(n * rec, dtype=np.uint8)
            for mix in ("unit", "real", "fifth", "full"):
                co = coefficients(3 * n, mix, 7)
                best = None
                for _ in range(2):
                    ms = (C.c_double * 2)()
                    if L.ug_points_combine(0, g2, col_ptr.ctypes.data, n, index.ctypes.data, co.ctypes.data, pts.ctypes.data, n, out.ctypes.data, ms, err, 511) != 0:
                        raise RuntimeError(err.value.decode())
                    if best is None or ms[0] + ms[1] < sum(best):
                        best = (ms[0], ms[1])
                print("2^%-2d %s %-5s %10.2f | %10.2f   %10.1f" % (log_n, "G2" if g2 else "G1", mix, best[0], best[1], 3 * n / sum(best) / 1e3), flush=True)
        pts = np.empty(n * 64, dtype=np.uint8)
        synth.synth_points(dev, n, 0x77, out=memoryview(pts))
        out = np.empty(n * 64, dtype=np.uint8)
        scalar = pow(7, 77, R).to_bytes(32, "little")
        best = None
        for _ in range(2):
            ms = (C.c_double * 1)()
            if L.ug_points_scale(0, scalar, pts.ctypes.data, n, out.ctypes.data, ms, err, 511) != 0:
                raise RuntimeError(err.value.decode())
            best = ms[0] if best is None else min(best, ms[0])
        print("2^%-2d one scalar (254 bits) times 2^%d G1 points: %.2f ms, %.1f M points/s" % (log_n, log_n, best, n / best / 1e3), flush=True)
    dev.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernels" and len(sys.argv) > 2:
        kernels([int(a) for a in sys.argv[2:]])
    elif what in ("setup", "host") and len(sys.argv) > 3 and sys.argv[2] in MIXES:
        setup(sys.argv[2], [int(a) for a in sys.argv[3:]], 0 if what == "setup" else -1)
    else:
        sys.exit(__doc__)
