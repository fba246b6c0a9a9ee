#!/usr/bin/env python3
"""Throughput of batch verification (include/verifier.h: ug_groth16_verify_batch) beside the single-proof verifier.

For N = 2^10, 2^14, 2^16 valid Groth16 proofs of tests/golden/trapdoor/groth16.{zkey,wtns}: proofs/s on the device, with
device = -1 (the same protocol on host threads), and of groth16_verify called from 16 host threads; at 2^14 also with one bad
proof and with 1 % bad proofs. A pool of --pool distinct proofs (prove_batch, fresh blinding) is repeated to fill N: every slot
still gets its own scalar, Miller loop and tree leaf, so the work is that of N distinct proofs. Prints a text report (the body of
profiles/verify_batch.txt) and writes it to --out.

    python tools/verify_bench.py --out out/verify_batch.txt [--sizes 10,14,16] [--host-sizes 10,14]

--judge 1 runs the batches through ug_groth16_verify_batch_opt with the judge on (--search-width / --judge-min, default the
library's); --judge both runs every batch that holds bad proofs with the judge off and on in turn, --repeat times, so that the
two are compared within one session (profiles/verify_judge.txt). With --judge the batches "50 % bad" and "every pi_b off the
subgroup" are added at 2^14 and "1 % bad" at 2^16. --sweep W1,W2,..:M1,M2,.. repeats "one bad" and "1 % bad" at 2^14 for every
search_width W and judge_min M.

--records compares the JSON call with ug_groth16_verify_batch_records on the same valid batches (profiles/verify_records.txt).
--records --format evm|compressed|all compares the record layouts instead (profiles/verify_record_formats.txt): the same valid
batches, converted ONCE outside the timed call, through ug_groth16_verify_batch_records (plain) and ug_groth16_verify_batch_records_fmt,
--runs runs of each in turn, with the ingest step of each call (ug_verify_batch_phase_ms [2]: upload, ingest kernel, ladder, status
bytes). --parent-lib PATH loads another build of the library beside this one and runs its plain records call in the same turns.

--keys K1,K2,.. measures the calls under several keys (profiles/verify_keys.txt): K keys x 2^--per-key records as ONE call of
ug_groth16_verify_batch_records_keys beside K one-key records calls of this build and of --parent-lib, in alternating turns, every
size warmed up; valid, with one bad record, and with 1 % bad records under every key with the judge on (keys_report).
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


PHASES = ("key", "parse+curve", "subgroup", "scalars+prefix", "packing", "pass", "root+search", "judge+single")


def records_report(a, L, vk, pool, run, say):
    """--records: the same valid batches through ug_groth16_verify_batch (texts) and ug_groth16_verify_batch_records (the same proofs
    packed ONCE, outside the timed call), --runs runs of each in turn; then the host split of both calls at the largest size, and the
    batch whose every pi_b is off the subgroup through the JSON call, judge off and on."""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    import ultragroth_amd as ug
    n_pub = len(json.loads(pool[0][1]))
    packed = [(ug.proof_pack(pr), ug.inputs_pack(pub, n_pub)) for pr, pub in pool]

    def phases():
        ms = (C.c_double * 8)()
        L.ug_verify_batch_phase_ms(ms)
        return "  ".join("%s %.1f" % (name, v) for name, v in zip(PHASES, ms))

    def run_records(n):
        recs = b"".join(packed[i % len(packed)][0] for i in range(n))
        ins = b"".join(packed[i % len(packed)][1] for i in range(n))
        verdicts, err, ex = (C.c_int * n)(), C.create_string_buffer(256), VerifyBatchStatsEx()
        t0 = time.perf_counter()
        rc = L.ug_groth16_verify_batch_records(a.device, n, recs, ins, n_pub, vk, verdicts, None, C.byref(ex), err, 255)
        dt = time.perf_counter() - t0
        if rc != 0 or any(verdicts):
            raise RuntimeError("verify_batch_records: rc %d, %s" % (rc, err.value.decode()))
        ms = (C.c_double * 3)()
        L.ug_verify_batch_kernel_ms(ms)
        return dt, ex.base, list(ms)

    run_records(64)
    sizes = [int(s) for s in a.sizes.split(",")]
    for lg in sizes:
        n = 1 << lg
        for rep in range(a.runs):
            for name, fn in (("json   ", lambda: run(n, a.device)), ("records", lambda: run_records(n))):
                dt, st, ms = fn()
                say("N=2^%d %s run %d  %9.0f proofs/s  wall %8.1f ms  device_ms %8.1f host_ms %8.1f  kernels: miller %.1f  f12 tree %.1f  g1 tree %.1f ms"
                    % (lg, name, rep, n / dt, dt * 1e3, st.device_ms, st.host_ms, ms[0], ms[1], ms[2]))
                if lg == max(sizes) and rep == a.runs - 1:
                    say("N=2^%d %s split (ms): %s" % (lg, name, phases()))
    if a.offsub_size:
        n = 1 << a.offsub_size
        for rep in range(a.runs):
            for judge in (0, 1):
                dt, st, _ = run(n, a.device, judge=judge, off_subgroup=True)
                say("N=2^%d json, every pi_b off the subgroup, judge %s  wall %9.1f ms  device_ms %8.1f host_ms %9.1f  single_checks %d judged %d"
                    % (a.offsub_size, "on " if judge else "off", dt * 1e3, st.device_ms, st.host_ms, st.single_checks, st.judged))
                if rep == a.runs - 1:
                    say("    split (ms): %s" % phases())


FORMATS = {"plain": 0, "evm": 1, "compressed": 2}


def formats_report(a, L, vk, pool, say):
    """--records --format: see the module docstring"""
    from ultragroth_amd._lib import VerifyBatchStatsEx
    import ultragroth_amd as ug
    n_pub = len(json.loads(pool[0][1]))
    names = {"all": ["evm", "compressed"], "plain": []}.get(a.format, [a.format])     # plain alone: this build beside --parent-lib
    packed = {"plain": [(ug.proof_pack(pr), ug.inputs_pack(pub, n_pub)) for pr, pub in pool]}
    for name in names:
        f = FORMATS[name]
        packed[name] = [(ug.proof_record_convert(r, ug.RECORDS_PLAIN, f), ug.inputs_convert(b, ug.RECORDS_PLAIN, f)) for r, b in packed["plain"]]
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        vp = C.c_void_p
        parent.ug_groth16_verify_batch_records.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.c_char_p, vp, vp, vp, C.c_char_p, C.c_ulong]
        parent.ug_verify_batch_phase_ms.argtypes = [vp]
        parent.ug_verify_batch_phase_ms.restype = None
        parent.ug_verify_batch_kernel_ms.argtypes = [vp]
        parent.ug_verify_batch_kernel_ms.restype = None

    def run_one(lib, name, n):
        src = packed[name]
        recs = b"".join(src[i % len(src)][0] for i in range(n))
        ins = b"".join(src[i % len(src)][1] for i in range(n))
        verdicts, err, ex = (C.c_int * n)(), C.create_string_buffer(256), VerifyBatchStatsEx()
        t0 = time.perf_counter()
        if name == "plain":
            rc = lib.ug_groth16_verify_batch_records(a.device, n, recs, ins, n_pub, vk, verdicts, None, C.byref(ex), err, 255)
        else:
            rc = lib.ug_groth16_verify_batch_records_fmt(a.device, FORMATS[name], n, recs, ins, n_pub, vk, verdicts, None, C.byref(ex), err, 255)
        dt = time.perf_counter() - t0
        if rc != 0 or any(verdicts):
            raise RuntimeError("verify_batch_records (%s): rc %d, %s" % (name, rc, err.value.decode()))
        phase, ms = (C.c_double * 8)(), (C.c_double * 3)()
        lib.ug_verify_batch_phase_ms(phase)
        lib.ug_verify_batch_kernel_ms(ms)
        return dt, ex.base, list(phase), list(ms)

    turns = ([("parent plain", parent, "plain")] if parent else []) + [("plain", L, "plain")] + [(name, L, name) for name in names]
    for lg in [int(s) for s in a.sizes.split(",")]:
        n = 1 << lg
        for label, lib, name in turns:
            run_one(lib, name, n)                                                  # warm-up of every code path at this size, not timed
        for rep in range(a.runs):
            for label, lib, name in turns[rep % len(turns):] + turns[:rep % len(turns)]:       # a turn starts with another call each time
                dt, st, phase, ms = run_one(lib, name, n)
                say("N=2^%d %-12s run %d  %9.0f proofs/s  wall %8.1f ms  device_ms %8.1f host_ms %8.1f  ingest step %6.2f ms  miller kernel %.1f ms"
                    % (lg, label, rep, n / dt, dt * 1e3, st.device_ms, st.host_ms, phase[2], ms[0]))


def keys_report(a, L, vk, pool, say):
    """--keys K1,K2,..: K keys x 2^--per-key valid records each, as ONE call of ug_groth16_verify_batch_records_keys beside K calls of
    ug_groth16_verify_batch_records (of this build, and of --parent-lib), keys parsed inside the timed region in all of them. The K
    keys are K copies of the fixture's key text: the library does not compare keys, so every copy is parsed, checked and given its
    own segment, which is the work of K distinct keys; the caller's order interleaves the keys, so the keyed call regroups. Then the
    same with one bad record under one key, and with 1 % bad records under every key with the judge on."""
    from ultragroth_amd._lib import VerifyBatchOptions, VerifyBatchStatsEx, VerifyBatchStatsKeys
    import ultragroth_amd as ug
    n_pub = len(json.loads(pool[0][1]))
    packed = [(ug.proof_pack(pr), ug.inputs_pack(pub, n_pub)) for pr, pub in pool]
    per = 1 << a.per_key
    vp = C.c_void_p
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.ug_groth16_verify_batch_records.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.c_char_p, vp, vp, vp, C.c_char_p, C.c_ulong]
        parent.ug_verify_batch_kernel_ms.argtypes = [vp]
        parent.ug_verify_batch_kernel_ms.restype = None

    def spoiled(block):
        v = int.from_bytes(block[:32], "little") + 1
        return v.to_bytes(32, "little") + block[32:]

    def options(judge):
        return C.byref(VerifyBatchOptions(C.sizeof(VerifyBatchOptions), 1, -1, -1)) if judge else None

    def one_key_calls(lib, K, bad, judge):
        """K calls, one per key, of per records each; bad: positions (key, index within the key)"""
        calls = []
        for q in range(K):
            blocks = [packed[(q * per + i) % len(packed)][1] for i in range(per)]
            for kq, i in bad:
                if kq == q:
                    blocks[i] = spoiled(blocks[i])
            calls.append((b"".join(packed[(q * per + i) % len(packed)][0] for i in range(per)), b"".join(blocks)))
        verdicts, err, ex = (C.c_int * per)(), C.create_string_buffer(256), VerifyBatchStatsEx()
        checks = singles = judged = 0
        opt = options(judge)
        t0 = time.perf_counter()
        for q, (recs, ins) in enumerate(calls):
            rc = lib.ug_groth16_verify_batch_records(a.device, per, recs, ins, n_pub, vk, verdicts, opt, C.byref(ex), err, 255)
            wrong = [i for i in range(per) if (verdicts[i] != 0) != ((q, i) in bad)]
            if rc == 2 or wrong:
                raise RuntimeError("verify_batch_records: rc %d, %s, %d wrong verdicts" % (rc, err.value.decode(), len(wrong)))
            checks += ex.base.batch_checks; singles += ex.base.single_checks; judged += ex.judged
        dt = time.perf_counter() - t0
        return dt, "batch_checks %d single_checks %d judged %d" % (checks, singles, judged)

    def keyed_call(K, bad, judge):
        n = K * per
        recs, blocks, key_of = [], [], []
        for i in range(per):                                                       # the caller's order: the keys interleaved
            for q in range(K):
                recs.append(packed[(q * per + i) % len(packed)][0])
                blocks.append(spoiled(packed[(q * per + i) % len(packed)][1]) if (q, i) in bad else packed[(q * per + i) % len(packed)][1])
                key_of.append(q)
        recs, ins = b"".join(recs), b"".join(blocks)
        keys = (C.c_char_p * K)(*([vk] * K))
        ko, npub = (C.c_int * n)(*key_of), (C.c_int * K)(*([n_pub] * K))
        verdicts, err, st = (C.c_int * n)(), C.create_string_buffer(256), VerifyBatchStatsKeys()
        opt = options(judge)
        t0 = time.perf_counter()
        rc = L.ug_groth16_verify_batch_records_keys(a.device, 0, n, recs, ins, K, keys, ko, npub, verdicts, opt, C.byref(st), err, 255)
        dt = time.perf_counter() - t0
        wrong = [t for t in range(n) if (verdicts[t] != 0) != ((t % K, t // K) in bad)]
        if rc == 2 or wrong:
            raise RuntimeError("verify_batch_records_keys: rc %d, %s, %d wrong verdicts" % (rc, err.value.decode(), len(wrong)))
        phase, ms = (C.c_double * 8)(), (C.c_double * 3)()
        L.ug_verify_batch_phase_ms(phase)
        L.ug_verify_batch_kernel_ms(ms)
        b = st.ex.base
        text = "batch_checks %d (key level %d) single_checks %d judged %d judge_launches %d segments %d tree_launches %d  kernels: miller %.1f  f12 forest %.2f  g1 forest %.2f ms" \
            % (b.batch_checks, st.key_checks, b.single_checks, st.ex.judged, st.ex.judge_launches, st.segments, st.tree_launches, ms[0], ms[1], ms[2])
        return dt, text, "  ".join("%s %.1f" % (name, v) for name, v in zip(PHASES, phase))

    for K in [int(s) for s in a.keys.split(",")]:
        one_pct = {(q, i) for q in range(K) for i in range(5, per, 100)}
        for label, bad, judge in (("valid", set(), False), ("one bad record", {(K // 3, per // 3)}, False), ("1%% bad under every key (%d), judge on" % len(one_pct), one_pct, True)):
            turns = ([("parent, K one-key calls", lambda: one_key_calls(parent, K, bad, judge))] if parent else []) + \
                [("this build, K one-key calls", lambda: one_key_calls(L, K, bad, judge)), ("this build, ONE keyed call", lambda: keyed_call(K, bad, judge))]
            for _, fn in turns:
                fn()                                                               # warm-up of every path at this size, not timed
            for rep in range(a.runs):
                for name, fn in turns[rep % len(turns):] + turns[:rep % len(turns)]:
                    out = fn()
                    say("K=%d x 2^%d %s | %-28s run %d  wall %8.1f ms  %9.0f proofs/s  %s" % (K, a.per_key, label, name, rep, out[0] * 1e3, K * per / out[0], out[1]))
                    if len(out) > 2 and rep == a.runs - 1:
                        say("    split of the keyed call (ms): %s" % out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--host-sizes", default="10,14,16", help="log2 sizes that also run with device = -1")
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--single-sample", type=int, default=512, help="proofs timed through groth16_verify on 16 threads")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--judge", default="0", choices=["0", "1", "both"])
    ap.add_argument("--search-width", type=int, default=-1, help="below zero: the library's default")
    ap.add_argument("--judge-min", type=int, default=-1, help="below zero: the library's default")
    ap.add_argument("--repeat", type=int, default=1, help="runs of every batch with bad proofs")
    ap.add_argument("--sweep", default=None, help="search widths : judge minima, e.g. 0,2,4,8,16:16,64,256")
    ap.add_argument("--skip-valid", action="store_true", help="only the batches with bad proofs")
    ap.add_argument("--batches", default="none,one,1pct,50pct,offsub", help="with --skip-valid: which of these batches run")
    ap.add_argument("--records", action="store_true", help="the JSON call and the packed-records call side by side, --runs times each")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--format", default="plain", choices=["plain", "evm", "compressed", "all"], help="--records: the record layouts side by side")
    ap.add_argument("--parent-lib", default=None, help="--records --format: another build of the library, its plain records call in the same turns")
    ap.add_argument("--offsub-size", type=int, default=12, help="--records: log2 size of the batch whose every pi_b is off the subgroup (0: skip)")
    ap.add_argument("--keys", default=None, help="K1,K2,..: K keys x 2^--per-key records as one keyed call beside K one-key calls (--parent-lib: also the parent's)")
    ap.add_argument("--per-key", type=int, default=10, help="--keys: log2 of the records per key")
    a = ap.parse_args()
    import ultragroth_amd as ug
    from ultragroth_amd._lib import VerifyBatchOptions, VerifyBatchStats, VerifyBatchStatsEx
    from oracle import pairing as PR
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

    def off_subgroup_b():
        """a point of the twist with x = 1: on the curve, outside the subgroup of order r (its cofactor is ~2^254)"""
        q = PR.P
        a = PR.f2_add((1, 0), PR.f2_muls(PR.f2_inv(PR.XI), 3))
        a1 = PR.f2_pow(a, (q - 3) // 4)
        x0 = PR.f2_mul(a1, a)
        alpha = PR.f2_mul(a1, x0)
        y = PR.f2_mul((0, 1), x0) if alpha == (q - 1, 0) else PR.f2_mul(PR.f2_pow(PR.f2_add((1, 0), alpha), (q - 1) // 2), x0)
        assert PR.f2_mul(y, y) == a
        return [["1", "0"], [str(y[0]), str(y[1])], ["1", "0"]]

    def run(n, device, bad=(), judge=None, off_subgroup=False, width=None, jmin=None):
        """judge None: the plain entry point; 0 / 1: ug_groth16_verify_batch_opt. off_subgroup: every proof's pi_b replaced"""
        proofs = [pool[i % len(pool)][0] for i in range(n)]
        pubs = [pool[i % len(pool)][1] for i in range(n)]
        for i in bad:
            s = json.loads(pubs[i])
            s[0] = str(int(s[0]) + 1)
            pubs[i] = json.dumps(s).encode()
        if off_subgroup:
            b, moved = off_subgroup_b(), {}
            for i in range(n):
                if proofs[i] not in moved:
                    pr = json.loads(proofs[i])
                    pr["pi_b"] = b
                    moved[proofs[i]] = json.dumps(pr).encode()
                proofs[i] = moved[proofs[i]]
            bad = range(n)
        pa, ia = (C.c_char_p * n)(*proofs), (C.c_char_p * n)(*pubs)
        verdicts, err = (C.c_int * n)(), C.create_string_buffer(256)
        t0 = time.perf_counter()
        if judge is None:
            stats = VerifyBatchStats()
            rc = L.ug_groth16_verify_batch(device, n, pa, ia, vk, verdicts, C.byref(stats), err, 255)
        else:
            opt = VerifyBatchOptions(C.sizeof(VerifyBatchOptions), judge, a.search_width if width is None else width, a.judge_min if jmin is None else jmin)
            ex = VerifyBatchStatsEx()
            rc = L.ug_groth16_verify_batch_opt(device, n, pa, ia, vk, verdicts, C.byref(opt), C.byref(ex), err, 255)
            stats = ex.base
            stats.judged, stats.judge_ms = ex.judged, ex.judge_ms
        dt = time.perf_counter() - t0
        bad = set(bad)
        wrong = [i for i in range(n) if (verdicts[i] != 0) != (i in bad)]
        if rc == 2 or wrong:
            raise RuntimeError("verify_batch: rc %d, %s, %d wrong verdicts" % (rc, err.value.decode(), len(wrong)))
        ms = (C.c_double * 3)()
        L.ug_verify_batch_kernel_ms(ms)
        return dt, stats, list(ms)

    say("# batch verification, Groth16, tests/golden/trapdoor/groth16 (%d distinct proofs repeated to fill N)" % len(pool))
    run(64, a.device)                                                  # warm-up: code objects, the context
    if a.records or a.keys:
        if a.keys:
            keys_report(a, L, vk, pool, say)
        elif a.format != "plain" or a.parent_lib:
            formats_report(a, L, vk, pool, say)
        else:
            records_report(a, L, vk, pool, run, say)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    host_sizes = {int(s) for s in a.host_sizes.split(",") if s}
    modes = {"0": [None], "1": [1], "both": [0, 1]}[a.judge]

    def bad_lines(lg, label, **kw):
        n = 1 << lg
        for rep in range(a.repeat):
            for judge in modes:
                dt, st, _ = run(n, a.device, judge=judge, **kw)
                tail = "" if judge is None else "  judge %s judged %d judge_ms %.1f" % ("on " if judge else "off", st.judged, st.judge_ms)
                say("N=2^%d device, %-22s %9.0f proofs/s  wall %8.1f ms  batch_checks %d single_checks %d%s"
                    % (lg, label, n / dt, dt * 1e3, st.batch_checks, st.single_checks, tail))

    for lg in [int(s) for s in a.sizes.split(",")]:
        n = 1 << lg
        one_pct = list(range(5, n, 100))[:n // 100]
        if a.skip_valid:
            want = a.batches.split(",")
            if lg == 14 and "none" in want:
                bad_lines(lg, "no bad", bad=[])
            if lg == 14 and "one" in want:
                bad_lines(lg, "one bad", bad=[n // 3])
            if "1pct" in want:
                bad_lines(lg, "1%% bad (%d)" % len(one_pct), bad=one_pct)
            if lg == 14 and "50pct" in want:
                bad_lines(lg, "50%% bad (%d)" % (n // 2), bad=list(range(1, n, 2)))
            if lg == 14 and "offsub" in want:
                bad_lines(lg, "every pi_b off subgroup", off_subgroup=True)
            continue
        dt, st, ms = run(n, a.device)
        say("N=2^%d device      %9.0f proofs/s  wall %8.1f ms  device_ms %8.1f host_ms %8.1f  kernels: miller %.1f  f12 tree %.1f  g1 tree %.1f ms  batch_checks %d"
            % (lg, n / dt, dt * 1e3, st.device_ms, st.host_ms, ms[0], ms[1], ms[2], st.batch_checks))
        if lg in host_sizes:
            dt, st, _ = run(n, -1)
            say("N=2^%d device=-1   %9.0f proofs/s  wall %8.1f ms  (16 host threads)" % (lg, n / dt, dt * 1e3))
        if lg == 14:
            bad_lines(lg, "one bad", bad=[n // 3])
            bad_lines(lg, "1%% bad (%d)" % len(one_pct), bad=one_pct)
            if a.judge != "0":
                bad_lines(lg, "50%% bad (%d)" % (n // 2), bad=list(range(1, n, 2)))
                bad_lines(lg, "every pi_b off subgroup", off_subgroup=True)
            dt, st, _ = run(n, -1, [n // 3])
            say("N=2^14 device=-1, one bad      %9.0f proofs/s  wall %8.1f ms  batch_checks %d single_checks %d" % (n / dt, dt * 1e3, st.batch_checks, st.single_checks))
    if a.sweep:
        widths, minima = [[int(v) for v in part.split(",")] for part in a.sweep.split(":")]
        n = 1 << 14
        one_pct = list(range(5, n, 100))[:n // 100]
        say("# sweep at N=2^14, judge on: wall ms of 'one bad' and '1% bad' per (search_width, judge_min)")
        for w in widths:
            for m in minima:
                t1, s1, _ = run(n, a.device, [n // 3], judge=1, width=w, jmin=m)
                t2, s2, _ = run(n, a.device, one_pct, judge=1, width=w, jmin=m)
                say("search_width %2d judge_min %3d   one bad %8.1f ms (checks %d singles %d judged %d)   1%% bad %8.1f ms (checks %d singles %d judged %d judge_ms %.1f)"
                    % (w, m, t1 * 1e3, s1.batch_checks, s1.single_checks, s1.judged, t2 * 1e3, s2.batch_checks, s2.single_checks, s2.judged, s2.judge_ms))
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
