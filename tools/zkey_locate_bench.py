#!/usr/bin/env python3
"""Measurements of locating the wrong records of a key (ug_zkey_locate_run): what profiles/zkey_locate.txt records.

    python tools/zkey_locate_bench.py <parent library> <log> [<log> ...]

<parent library>: the parent commit's build of libultragroth_hip.so, which has ug_zkey_verify_run and no route to the names.
Per size, in one process, every pair of calls alternated ROUNDS times:
  (a) a key with ONE wrong record in section 8: ug_zkey_locate_run of this build beside the parent's ug_zkey_verify_run
  (b) a key whose H section is of another delta: the same pair
  (c) a valid key: ug_zkey_verify_run of this build beside the parent's (the path is untouched: the difference must lie within the
      spread of the parent's own runs)
and the rates of the two new kernels from the located report's stream-event times: pairs/s of ratio_block_sums_kernel over a
section's records, lanes/s of ratio_judge_kernel over the block sums and the resolved records together.
The circuit, the .ptau and the key are zkey_verify_bench's (the squaring chain, mix "real", synthetic slices)."""
import ctypes as C
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ultragroth_amd as ug  # noqa: E402
from ultragroth_amd import synth  # noqa: E402
from setup_ptau_bench import fake_ptau, mixed_chain  # noqa: E402

R = synth.R_MOD
DELTA, OTHER_DELTA = pow(7, 77, R), pow(11, 55, R)
ROUNDS = 3


def make_key(r1cs, ptau, delta):
    opt = ug._SetupPtauOptions()
    opt.size, opt.validate, opt.contribute = C.sizeof(opt), 1, 1
    opt.delta = ug._le32(delta, "delta")
    L = ug.load()
    err = C.create_string_buffer(512)
    zbytes, vmax, wrote, vlen = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    if L.ug_setup_ptau_size(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, C.byref(zbytes), C.byref(vmax), err, 511) != 0:
        raise RuntimeError(err.value.decode())
    zkey = np.empty(zbytes.value, dtype=np.uint8)
    vkey = C.create_string_buffer(vmax.value)
    raw = (C.c_double * len(ug.SETUP_PTAU_PHASES))()
    if L.ug_setup_ptau_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, 0, zkey.ctypes.data, zbytes.value, C.byref(wrote),
                           vkey, vmax.value, C.byref(vlen), raw, err, 511) != 0:
        raise RuntimeError(err.value.decode())
    return zkey[:wrote.value]


def section(zkey, sid):
    """(offset, size) of a section's payload"""
    n = struct.unpack_from("<I", zkey, 8)[0]
    at = 12
    for _ in range(n):
        i, size = struct.unpack_from("<IQ", zkey, at)
        if i == sid:
            return at + 12, size
        at += 12 + size
    raise KeyError(sid)


def verify(L, r1cs, ptau, zkey):
    opt = ug._ZkeyVerifyOptions()
    opt.size, opt.validate = C.sizeof(opt), 2
    rep = ug._ZkeyVerifyReport()
    raw = (C.c_double * len(ug.ZKEY_VERIFY_PHASES))()
    err = C.create_string_buffer(512)
    t0 = time.time()
    rc = L.ug_zkey_verify_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, zkey.ctypes.data, zkey.size, 0, C.byref(rep), raw, err, 511)
    return (time.time() - t0) * 1e3, rc, rep.failed_sections


def locate(L, r1cs, ptau, zkey, located):
    opt = ug._ZkeyLocateOptions()
    opt.size, opt.validate = C.sizeof(opt), 2
    rep = ug._ZkeyVerifyReport()
    raw = (C.c_double * len(ug.ZKEY_VERIFY_PHASES))()
    err = C.create_string_buffer(512)
    t0 = time.time()
    rc = L.ug_zkey_locate_run(C.byref(opt), r1cs, len(r1cs), ptau.ctypes.data, ptau.size, zkey.ctypes.data, zkey.size, 0, C.byref(rep),
                              C.byref(located), raw, err, 511)
    return (time.time() - t0) * 1e3, rc, rep.failed_sections


def spread(v):
    return "%.0f - %.0f ms" % (min(v), max(v))


def main(parent_path, logs):
    dev = ug.Device(0)
    L = ug.load()
    P = C.CDLL(os.path.abspath(parent_path))
    P.ug_zkey_verify_run.argtypes = L.ug_zkey_verify_run.argtypes
    assert not hasattr(P, "ug_zkey_locate_run"), "the parent library has no locate entry"
    print("locating on the squaring chain, mix real; this build against %s; %d alternated rounds per pair" % (parent_path, ROUNDS))
    for log_n in logs:
        t0 = time.time()
        r1cs = mixed_chain(log_n, "real")
        ptau = fake_ptau(dev, log_n)
        valid = make_key(r1cs, ptau, DELTA)
        other = make_key(r1cs, ptau, OTHER_DELTA)
        one = valid.copy()                                   # (a) record 17 of section 8 replaced by record 40211 (a valid point, not its own)
        at, size = section(one, 8)
        one[at + 64 * 17:at + 64 * 18] = valid[at + 64 * 40211:at + 64 * 40212]
        hkey = valid.copy()                                  # (b) H of another delta
        at, size = section(hkey, 9)
        hkey[at:at + size] = other[at:at + size]
        del other
        print("2^%d: inputs made in %.1f s (zkey %.0f MiB)" % (log_n, time.time() - t0, valid.size / 2 ** 20), flush=True)
        located = ug._ZkeyLocateReport()
        for name, key, want in (("(a) one wrong record in section 8", one, 1 << 8), ("(b) H of another delta", hkey, 1 << 9)):
            tl, tv = [], []
            for _ in range(ROUNDS):
                ms, rc, failed = verify(P, r1cs, ptau, key)
                assert rc == ug.UG_ZKEY_INVALID and failed == want
                tv.append(ms)
                ms, rc, failed = locate(L, r1cs, ptau, key, located)
                assert rc == ug.UG_ZKEY_INVALID and failed == want and located.n_sections == 1
                tl.append(ms)
            e = located.section[0]
            lanes = e.blocks + e.resolved_blocks * 256
            print("2^%-2d %s: parent's zkey_verify %s; zkey_locate %s; extra over the bare verdict %.0f ms (medians), of it after the verdict %.0f ms"
                  % (log_n, name, spread(tv), spread(tl), sorted(tl)[ROUNDS // 2] - sorted(tv)[ROUNDS // 2], located.locate_ms))
            print("      section %d: %d records, %d blocks, %d fail, %d resolved, exact %d, %d wrong, listed %s" % (
                e.section, e.records, e.blocks, e.bad_blocks, e.resolved_blocks, e.exact, e.bad_records, [e.index[i] for i in range(min(e.n_listed, 4))]))
            print("      ratio_block_sums_kernel %.2f ms = %.1f M pairs/s; ratio_judge_kernel %.1f ms over %d lanes = %.0f lanes/s" % (
                e.kernel_ms[0], e.records / e.kernel_ms[0] / 1e3, e.kernel_ms[1], lanes, lanes / e.kernel_ms[1] * 1e3), flush=True)
        tp, tn = [], []
        for _ in range(ROUNDS):
            ms, rc, _ = verify(P, r1cs, ptau, valid)
            assert rc == 0
            tp.append(ms)
            ms, rc, _ = verify(L, r1cs, ptau, valid)
            assert rc == 0
            tn.append(ms)
        print("2^%-2d (c) zkey_verify of a valid key: parent %s; this build %s" % (log_n, spread(tp), spread(tn)), flush=True)
        del r1cs, ptau, valid, one, hkey
    dev.close()


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], [int(a) for a in sys.argv[2:]])
