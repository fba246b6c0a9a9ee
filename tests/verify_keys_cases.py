"""Shared by tests/test_verify_keys_host.py and tests/test_gpu_verify_keys.py: the keys and proofs of the calls under several keys
(include/verifier.h: the _keys entry points), their raw calls, the check bound of a rejected pass of several segments, and the forest
hook with a forest restated from the one-key hook's tree. Every expected verdict is the SINGLE verifier's on the same strings under the
proof's own key (verify_batch_cases.single), never the batch code's."""
import ctypes as C
import functools
import json
import math
import os
import random

import oracle as O
import r1cs_cases as RC
import setup_cases as SC
import verify_batch_cases as VB
import verify_records_cases as VR
from conftest import GOLDEN
from oracle import pairing as PR
from ultragroth_amd import synth
from verify_batch_cases import VALID, INVALID, ERROR, SENTINEL

R = synth.R_MOD
Q = PR.P
PER_KEY = 20            # proofs made per key
F12_WORDS, XYZZ_WORDS = 108, 36


def _ug():
    import ultragroth_amd as ug
    return ug


def _read(path, mode="rb"):
    with open(path, mode) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def chain_circuit(steps=9, outs=(9, 5, 2)):
    """a squaring chain x_(i+1) = x_i^2 with len(outs) public outputs (the values x_9, x_5, x_2): nPublic 3, in the style of
    setup_cases.sparse_b_circuit. wires: 0 one | 1 .. 3 the outputs | then the other x_i. Returns (.r1cs bytes, witness maker)."""
    wire = {}
    for slot, i in enumerate(outs):
        wire[i] = 1 + slot
    nxt = 1 + len(outs)
    for i in range(steps + 1):
        if i not in wire:
            wire[i] = nxt
            nxt += 1
    rows = [({wire[i]: 1}, {wire[i]: 1}, {wire[i + 1]: 1}) for i in range(steps)]

    def witness(x0):
        w = [0] * nxt
        w[0] = 1
        v = x0 % R
        for i in range(steps + 1):
            w[wire[i]] = v
            v = v * v % R
        return RC.wtns_file(w)
    return synth.r1cs_file(nxt, len(outs), 0, rows), witness


def _other_trapdoor(shift):
    return {k: str((int(v) * 3 + shift) % R or 1) for k, v in SC.trapdoor_dict().items()}


@functools.lru_cache(maxsize=None)
def g16_keys():
    """three Groth16 keys with 1, 2 and 3 public inputs: the reference fixture, the trapdoor fixture, a dev_setup key of
    chain_circuit. Returns [(vk dict, proofs, pubs)], PER_KEY valid proofs each (the oracle's)."""
    out = []
    zkey, wtns = _read(os.path.join(GOLDEN, "circuit_final.zkey")), _read(os.path.join(GOLDEN, "witness.wtns"))
    pairs = [O.groth16_prove(zkey, wtns, 31 + 5 * i, 77 + 3 * i)[:2] for i in range(PER_KEY)]
    out.append((json.loads(_read(os.path.join(GOLDEN, "verification_key.json"), "r")), [p for p, _ in pairs], [s for _, s in pairs]))
    zkey, wtns = VB.load("groth16.zkey"), VB.load("groth16.wtns")
    pairs = [O.groth16_prove(zkey, wtns, 1000 + 7 * i, 5000 + 11 * i)[:2] for i in range(PER_KEY)]
    out.append((json.loads(VB.load("groth16_vkey.json", "r")), [p for p, _ in pairs], [s for _, s in pairs]))
    r1cs, witness = chain_circuit()
    zkey, vk, _ = _ug().dev_setup(r1cs, _other_trapdoor(11), "groth16", device=-1)
    pairs = [O.groth16_prove(zkey, witness(3 + i), 200 + i, 900 + 13 * i)[:2] for i in range(PER_KEY)]
    out.append((vk, [p for p, _ in pairs], [s for _, s in pairs]))
    counts = [len(vk["IC"]) - 1 for vk, _, _ in out]
    assert counts == [1, 2, 3], counts
    for vk, proofs, pubs in out:
        assert all(VB.single(False, p, s, vk) == VALID for p, s in zip(proofs, pubs))
    return out


@functools.lru_cache(maxsize=None)
def ultra_keys():
    """two UltraGroth keys of the trapdoor circuit: the fixture, and a dev_setup key under another trapdoor"""
    out = []
    _, _, r1cs = RC.trapdoor()
    uwtns = VB.load("ultra.uwtns")
    for which in range(2):
        if which == 0:
            zkey, vk = VB.load("ultra.zkey"), json.loads(VB.load("ultra_vkey.json", "r"))
        else:
            zkey, vk, _ = _ug().dev_setup(r1cs, _other_trapdoor(29), "ultragroth", log_domain=10, device=-1, ultra=SC.ultra_spec())
        pairs = [O.ultra_groth_prove(zkey, uwtns, 10 + i + 50 * which, 200 + i, 3000 + i)[:2] for i in range(12)]
        proofs, pubs = [p for p, _ in pairs], [s for _, s in pairs]
        assert all(VB.single(True, p, s, vk) == VALID for p, s in zip(proofs, pubs))
        out.append((vk, proofs, pubs))
    assert VB.single(True, out[0][1][0], out[0][2][0], out[1][0]) == INVALID      # the keys do differ
    return out


def interleave(sets, counts, seed=5):
    """counts[q] proofs of every key, shuffled: (proofs, pubs, key_of)"""
    items = [(q, i) for q, c in enumerate(counts) for i in range(c)]
    random.Random(seed).shuffle(items)
    return [sets[q][1][i] for q, i in items], [sets[q][2][i] for q, i in items], [q for q, _ in items]


def expected(ultra, proofs, pubs, vks, key_of):
    return [VB.single(ultra, p, s, vks[q]) for p, s, q in zip(proofs, pubs, key_of)]


# ---- raw calls ---------------------------------------------------------------------------------------------------------------
def _stats(stats):
    out = VR._stats(stats.ex)
    out.update({f: getattr(stats, f) for f in ("segments", "tree_launches", "key_checks")})
    return out


def _keys_args(vks, key_of, n):
    texts = [VB._enc(k) for k in vks]
    return len(texts), (C.c_char_p * max(len(texts), 1))(*texts), (C.c_int * max(n, 1))(*key_of) if key_of is not None else None


def keys_batch(ultra, proofs, pubs, vks, key_of, device=-1, opt=None, n_keys=None):
    """raw text call: (rc, message, verdicts, stats dict); opt: None or verify_records_cases.options(...)"""
    from ultragroth_amd._lib import VerifyBatchStatsKeys
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_keys if ultra else L.ug_groth16_verify_batch_keys
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[VB._enc(p) for p in pubs])
    nk, ka, ko = _keys_args(vks, key_of, n)
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStatsKeys(), C.create_string_buffer(512)
    rc = fn(device, n, pa, ia, nk if n_keys is None else n_keys, ka, ko, verdicts, C.byref(opt) if opt is not None else None, C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), _stats(stats)


def keys_records(ultra, recs, blocks, vks, key_of, device=-1, fmt=0, opt=None, n_pub=None):
    """raw records call over per-proof records and input blocks (already in the layout `fmt`); the input block is the ragged one"""
    from ultragroth_amd._lib import VerifyBatchStatsKeys
    L = VB.lib()
    fn = L.ug_ultra_groth_verify_batch_records_keys if ultra else L.ug_groth16_verify_batch_records_keys
    n = len(recs)
    nk, ka, ko = _keys_args(vks, key_of, n)
    if n_pub is None:
        n_pub = [len(vk["IC"]) - 1 for vk in vks]
    npa = (C.c_int * max(len(n_pub), 1))(*n_pub)
    verdicts = (C.c_int * max(n, 1))(*([SENTINEL] * max(n, 1)))
    stats, err = VerifyBatchStatsKeys(), C.create_string_buffer(512)
    rc = fn(device, fmt, n, b"".join(recs) or b"\0", b"".join(blocks) or b"\0", nk, ka, ko, npa, verdicts, C.byref(opt) if opt is not None else None,
            C.byref(stats), err, 511)
    return rc, err.value.decode(), list(verdicts[:n]), _stats(stats)


def check_bound(seg_sizes, bad_per_seg, stats):
    """A rejected pass of segments seg_sizes with bad_per_seg[s] bad proofs in segment s: the pass's one equation, two checks per
    failing segment and level of the tree over the S segments, then per failing segment two checks per bad proof and level while
    the failing node covers more than 16 proofs; the single verifier for at most 16 proofs per bad one."""
    S = len(seg_sizes)
    failing = sum(1 for b in bad_per_seg if b)
    key_levels = math.ceil(math.log2(S)) if S > 1 else 0
    inner = sum(2 * b * max(0, math.ceil(math.log2(n / 16))) for n, b in zip(seg_sizes, bad_per_seg) if b)
    assert stats["batch_checks"] <= 1 + 2 * failing * key_levels + inner, stats
    assert stats["single_checks"] <= 16 * sum(bad_per_seg), stats
    assert stats["key_checks"] <= 1 + 2 * failing * key_levels, stats


# ---- the forest hook -------------------------------------------------------------------------------------------------------
def forest_nodes(sizes):
    """nodes of the forest over segments of these sizes (include/verifier.h: ug_test_tree_forest)"""
    total, m = 0, list(sizes)
    while m:
        total += sum(m)
        m = [(x + 1) // 2 for x in m if x > 1]
    return total


@functools.lru_cache(maxsize=None)
def forest_leaves(n, k, seed):
    """leaves as the Miller kernel leaves them: n arbitrary canonical Fq12 values (12 coefficients below q, each 9 limbs of 29
    bits) and n x k XYZZ records (x, y, zz = zzz = 1, Montgomery radix 2^261) of multiples of the generator -- a random multiple,
    then steps of another one, so that no two are equal or opposite"""
    rng = random.Random(seed)
    mont = lambda x: x * (1 << 261) % Q
    limbs = lambda x: [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    f = []
    for _ in range(n * 12):
        f += limbs(rng.randrange(Q))
    g = []
    p, step = PR.g1_mul((1, 2), rng.randrange(1, R)), PR.g1_mul((1, 2), rng.randrange(1, 1 << 64))
    for _ in range(n * k):
        g += limbs(mont(p[0])) + limbs(mont(p[1])) + limbs(mont(1)) + limbs(mont(1))
        p = PR.g1_add(p, step)
    return (C.c_uint32 * len(f))(*f), (C.c_uint32 * len(g))(*g)


def forest(device, k, sizes, leaves_f, leaves_g):
    """ug_test_tree_forest: (f_tree bytes, g_tree bytes)"""
    nodes = forest_nodes(sizes)
    fo, go = (C.c_uint32 * (nodes * F12_WORDS))(), (C.c_uint32 * (nodes * k * XYZZ_WORDS))()
    sz = (C.c_int * len(sizes))(*sizes)
    assert VB.lib().ug_test_tree_forest(device, k, len(sizes), sz, leaves_f, leaves_g, fo, go) == 0
    return bytes(fo), bytes(go)


def forest_from_single_trees(k, sizes, leaves_f, leaves_g):
    """the same forest put together by this file from the ONE-segment hook call of every segment (one segment: the tree of a
    one-key pass): level l of the forest is level l of every segment that still has one, in segment order"""
    per_seg, at = [], 0
    lf, lg = bytes(leaves_f), bytes(leaves_g)
    for n in sizes:
        sf = (C.c_uint32 * (n * F12_WORDS)).from_buffer_copy(lf[at * F12_WORDS * 4:(at + n) * F12_WORDS * 4])
        sg = (C.c_uint32 * (n * k * XYZZ_WORDS)).from_buffer_copy(lg[at * k * XYZZ_WORDS * 4:(at + n) * k * XYZZ_WORDS * 4])
        per_seg.append(forest(-1, k, [n], sf, sg))
        at += n
    f_out, g_out, level, offs = b"", b"", list(sizes), [0] * len(sizes)
    while any(level):
        for s, m in enumerate(level):
            if not m:
                continue
            f_out += per_seg[s][0][offs[s] * F12_WORDS * 4:(offs[s] + m) * F12_WORDS * 4]
            g_out += per_seg[s][1][offs[s] * k * XYZZ_WORDS * 4:(offs[s] + m) * k * XYZZ_WORDS * 4]
            offs[s] += m
        level = [(m + 1) // 2 if m > 1 else 0 for m in level]
    return f_out, g_out
