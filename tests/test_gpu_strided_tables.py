"""Strided fixed-base window tables (include/ultragroth_hip.h: ug_bases_create_tables_strided_g1 and the calls beside it) and
the created provers' table plan under ULTRAGROTH_TABLES_BUDGET.

With stride s a set holds T = ceil(W/s) tables 2^(s c j) P_i; a digit of window w goes to bucket set w mod s and reads table
w / s. Sums are checked against the closed form of the generator walk (synth.synth_points: P_i = (seed + i) G, so
sum s_i P_i = (sum s_i (seed + i) mod r) G) and, for the created provers, whole proofs against the CPU oracle."""
import os

import pytest

import oracle as O
from conftest import fixed_rs

pytestmark = pytest.mark.gpu

GiB = 1 << 30
SEED_A, SEED_B, SEED_C, SEED_G2 = 0x1234_0001, 0x1234_0003, 0x1234_0005, 0x1234_0007


def _windows(c):
    return (255 + c - 1) // c


def _walk(g2, sc, n, seed):
    from ultragroth_amd import synth
    k = O.fr_dot_walk(sc, n, seed)
    return O.g2_mul(synth.g2_generator_record(), k) if g2 else O.g1_mul(synth.g1_generator_record(), k)


def _strides(c):
    w = _windows(c)
    return sorted({1, 2, 3, w - 1, w})


@pytest.fixture(scope="module")
def walk_points(device):
    from ultragroth_amd import synth
    n = 1 << 16
    return {"A": bytes(synth.synth_points(device, n, SEED_A)), "B": bytes(synth.synth_points(device, n, SEED_B)),
            "C": bytes(synth.synth_points(device, n, SEED_C)), "G2": bytes(synth.synth_points(device, n, SEED_G2, g2=True))}


@pytest.mark.parametrize("n", [(1 << 14) + 3, 1 << 16])
@pytest.mark.parametrize("c", [16, 20])
def test_strided_msm_g1_g2(device, walk_points, n, c):
    """every stride from 1 (the plain tables) to W (one table) gives the closed-form sum, G1 and G2, uniform and circom-like"""
    from ultragroth_amd import synth
    mixes = [(mix, synth.scalars(n, mix, 77 + n + c).tobytes()) for mix in ("U", "C")]
    for g2, pts, seed in ((False, walk_points["A"][:64 * n], SEED_A), (True, walk_points["G2"][:128 * n], SEED_G2)):
        for s in _strides(c):
            b = device.bases(pts, n, g2=g2, table_c=c, table_stride=s)
            assert device._L.ug_bases_table_window(b.h) == c and device._L.ug_bases_table_stride(b.h) == s
            for mix, sc in mixes:
                v = device.dvec(n, sc)
                got = device.msm(b, device.schedule(v, 0, n, table_c=c, table_stride=s), g2=g2)
                assert got == _walk(g2, sc, n, seed), (g2, s, mix)
            if not g2 and s == 2:                                       # a classic schedule reads table 0 only
                sc = mixes[0][1]
                assert device.msm(b, device.schedule(device.dvec(n, sc), 0, n)) == _walk(False, sc, n, seed)


def test_strided_msm_against_the_oracle_pippenger(device, zkey):
    """zkey points with points at infinity among them (B1 of the fixture), against the oracle's own MSM"""
    import random
    n = O.zkey_info(zkey)["nVars"]
    off, _ = O.section(zkey, "zkey", 6)
    pts = zkey[off:off + 64 * n]
    rng = random.Random(5)
    sc = b"".join(O.to_le(rng.choice([0, 1, 2, O.R_MOD - 1, rng.randrange(O.R_MOD)])) for _ in range(n))
    v = device.dvec(n, sc)
    for c, s in ((16, 2), (17, 3), (24, 5), (24, 11)):
        b = device.bases(pts, n, table_c=c, table_stride=s)
        assert device.msm(b, device.schedule(v, 0, n, table_c=c, table_stride=s)) == O.g1_msm(pts, sc, n), (c, s)


@pytest.mark.parametrize("c,s", [(16, 3), (20, 2), (20, 12)])
def test_strided_group_and_g2_share_one_schedule(device, walk_points, c, s):
    """the interleaved K = 3 group (C with an index shift) and a G2 set, all strided, over ONE strided schedule"""
    from ultragroth_amd import synth
    n, shift = (1 << 14) + 3, 5
    A, B, Cp, G2 = walk_points["A"][:64 * n], walk_points["B"][:64 * n], walk_points["C"][:64 * (n - shift)], walk_points["G2"][:128 * n]
    grp = device.bases_group([(A, n, 0), (B, n, 0), (Cp, n - shift, shift)], 0, n, table_c=c, table_stride=s)
    g2 = device.bases(G2, n, g2=True, table_c=c, table_stride=s)
    for mix in ("U", "C"):
        sc = synth.scalars(n, mix, 991 + s).tobytes()
        sch = device.schedule(device.dvec(n, sc), 0, n, table_c=c, table_stride=s)
        exp = [_walk(False, sc, n, SEED_A), _walk(False, sc, n, SEED_B), _walk(False, sc[32 * shift:], n - shift, SEED_C)]
        assert device.msm_group(grp, sch) == exp, mix
        assert device.msm(g2, sch, g2=True) == _walk(True, sc, n, SEED_G2), mix


def test_strided_deferred_build_in_pieces(device, walk_points):
    """ug_ctx_defer_tables: the set remembers width and stride, alloc + adopt give it room, steps build it in pieces"""
    import ctypes as C
    from ultragroth_amd import synth
    L = device._L
    n, c, s = 1 << 16, 20, 3
    sc = synth.scalars(n, "U", 4242).tobytes()
    v = device.dvec(n, sc)
    assert L.ug_ctx_defer_tables(device._h, 1) == 0
    try:
        for g2, pts, seed in ((False, walk_points["A"], SEED_A), (True, walk_points["G2"], SEED_G2)):
            h = C.c_void_p()
            fn = L.ug_bases_create_tables_strided_g2 if g2 else L.ug_bases_create_tables_strided_g1
            assert fn(device._h, pts, n, 0, c, s, C.byref(h)) == 0
            import ultragroth_amd as ug
            b = ug._Handle(h, L.ug_bases_destroy, device)
            assert L.ug_bases_table_window(h) == 0                       # deferred: plain points until adopted
            assert device.msm(b, device.schedule(v, 0, n), g2=g2) == _walk(g2, sc, n, seed)
            mem = C.c_void_p()
            assert L.ug_bases_tables_alloc(h, C.byref(mem)) == 0
            assert L.ug_bases_tables_adopt(h, mem) == 0
            assert L.ug_bases_table_window(h) == c and L.ug_bases_table_stride(h) == s
            left, steps = C.c_uint64(1), 0
            while left.value:
                assert L.ug_bases_tables_step(h, C.c_uint64(10000), C.byref(left)) == 0
                steps += 1
                if steps == 2:                                           # not finished: a table schedule is refused
                    assert L.ug_bases_tables_ready(h) == 0
                    sch = C.c_void_p()
                    assert L.ug_schedule_create(device._h, C.byref(sch)) == 0
                    assert L.ug_schedule_build_tables_strided(sch, v.h, 0, n, c, s) == 0
                    out = C.create_string_buffer(128)
                    fn2 = L.ug_msm_g2 if g2 else L.ug_msm_g1
                    assert fn2(device._h, h, sch, 0, out) != 0
                    L.ug_schedule_destroy(sch)
            assert steps >= 3 and L.ug_bases_tables_ready(h) == 1
            assert device.msm(b, device.schedule(v, 0, n, table_c=c, table_stride=s), g2=g2) == _walk(g2, sc, n, seed)
    finally:
        L.ug_ctx_defer_tables(device._h, 0)


def test_strided_rejections(device, walk_points):
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    n = 1 << 14
    sc = synth.scalars(n, "U", 3).tobytes()
    v = device.dvec(n, sc)
    b2 = device.bases(walk_points["A"][:64 * n], n, table_c=20, table_stride=2)
    with pytest.raises(ug.DeviceError, match="stride 3 but the bases hold tables of stride 2"):
        device.msm(b2, device.schedule(v, 0, n, table_c=20, table_stride=3))
    with pytest.raises(ug.DeviceError, match="width"):
        device.msm(b2, device.schedule(v, 0, n, table_c=21, table_stride=2))
    b1 = device.bases(walk_points["A"][:64 * n], n, table_c=20)
    with pytest.raises(ug.DeviceError, match="stride 2 but the bases hold tables of stride 1"):
        device.msm(b1, device.schedule(v, 0, n, table_c=20, table_stride=2))
    for bad in (0, -1, _windows(20) + 1):
        with pytest.raises(ug.DeviceError, match="stride"):
            device.schedule(v, 0, n, table_c=20, table_stride=bad)
        with pytest.raises(ug.DeviceError, match="stride"):
            device.bases(walk_points["A"][:64 * n], n, table_c=20, table_stride=bad)
    with pytest.raises(ug.DeviceError, match="bucket classes"):
        device.schedule(v, 0, n, table_c=16, table_stride=2, classes=(3, 0, 8, 0, 0, 0))
    # the plain calls are the stride-1 case
    assert device.msm(b1, device.schedule(v, 0, n, table_c=20, table_stride=1)) == device.msm(b1, device.schedule(v, 0, n, table_c=20))


# ---- created provers ---------------------------------------------------------------------------------------------
def _prove(p, wtns, rs):
    import ultragroth_amd as ug
    ug.set_test_blinding(rs)
    try:
        return p.prove(wtns)
    finally:
        ug.set_test_blinding(b"")


def _budget_env(monkeypatch, budget):
    monkeypatch.setenv("ULTRAGROTH_TABLES_BUDGET", "%.9f" % (budget / GiB))


def _full_bytes(full_plan):
    return [b for _, _, b, _ in full_plan]


_CIRCUITS = {}


def _circuit(device, log, b_zero):
    from ultragroth_amd import synth
    key = (log, b_zero)
    if key not in _CIRCUITS:
        zkey, wtns, info = synth.build_circuit(device, log, mix="C", b_zero=b_zero)
        r, s = fixed_rs()
        exp = O.groth16_prove(zkey, wtns, int.from_bytes(r, "little"), int.from_bytes(s, "little"))
        _CIRCUITS[key] = (zkey, wtns, (exp[0], exp[1]))
    return _CIRCUITS[key]


@pytest.mark.parametrize("log,b_zero", [(16, 0.0), (17, 0.0), (16, 0.5)])
@pytest.mark.parametrize("bg", ["1", "0"])
def test_created_groth16_prover_under_a_budget(device, monkeypatch, log, b_zero, bg):
    import ultragroth_amd as ug
    zkey, wtns, exp = _circuit(device, log, b_zero)
    r, s = fixed_rs()
    monkeypatch.setenv("ULTRAGROTH_TABLES_BG", bg)
    monkeypatch.delenv("ULTRAGROTH_TABLES_BUDGET", raising=False)
    with ug.Groth16Prover(zkey) as p:                       # no budget: the unchanged default, full tables at stride 1
        p.tables_ready(wait=True)
        full = p.table_plan()
        assert len(full) == (3 if b_zero else 2)
        assert all(c and st == 1 and ready for c, st, _, ready in full), full
        assert _prove(p, wtns, r + s) == exp
    fb = _full_bytes(full)
    for budget in (fb[1], min(fb) // 2):                     # about H's full tables; below any full group
        _budget_env(monkeypatch, budget)
        free0, _ = device.mem_info()
        with ug.Groth16Prover(zkey) as p:
            first = _prove(p, wtns, r + s)
            p.tables_ready(wait=True)
            plan = p.table_plan()
            assert all(ready for _, _, _, ready in plan)
            assert sum(b for _, _, b, _ in plan) <= budget
            assert any(c for c, _, _, _ in plan), plan
            assert plan != full and any((c, st) != (fc, fs) for (c, st, _, _), (fc, fs, _, _) in zip(plan, full))
            if budget < min(fb):
                assert any(c and st > 1 for c, st, _, _ in plan), plan
            free1, _ = device.mem_info()
            assert free0 - free1 <= budget + 2 * GiB + 64 * 8 * (1 << log)     # tables + points, vectors, workspaces
            assert first == exp
            assert _prove(p, wtns, r + s) == exp


def test_created_ultragroth_prover_with_strides(device, monkeypatch):
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    zkey, uwtns, info = synth.build_ultra_circuit(device, 17)
    rk, r, s = bytes(range(1, 32)), bytes(range(40, 71)), bytes(range(80, 111))
    exp = O.ultra_groth_prove(zkey, uwtns, int.from_bytes(rk, "little"), int.from_bytes(r, "little"), int.from_bytes(s, "little"))
    monkeypatch.delenv("ULTRAGROTH_TABLES_BUDGET", raising=False)
    with ug.UltraGrothProver(zkey) as p:
        full = p.table_plan()
    assert all(st == 1 for c, st, _, _ in full if c)
    budget = min(b for b in _full_bytes(full) if b) // 2        # below any full group: whatever the plan holds is strided
    _budget_env(monkeypatch, budget)
    with ug.UltraGrothProver(zkey) as p:
        plan = p.table_plan()
        assert sum(b for _, _, b, _ in plan) <= budget
        assert any(c and st > 1 for c, st, _, _ in plan), plan
        for _ in range(2):
            assert _prove(p, uwtns, rk + r + s) == exp


def test_budget_zero_is_tables_off(device, monkeypatch):
    import ultragroth_amd as ug
    zkey, wtns, exp = _circuit(device, 16, 0.0)
    r, s = fixed_rs()
    monkeypatch.setenv("ULTRAGROTH_TABLES_BUDGET", "0")
    with ug.Groth16Prover(zkey) as p:
        assert all(c == 0 and b == 0 and ready for c, _, b, ready in p.table_plan())
        assert _prove(p, wtns, r + s) == exp


HUGE_LOG = int(os.environ.get("UG_HUGE_LOG", "26"))


def test_2_26_on_one_device_plans_tables(device):
    """BASELINE configs[3]: full tables do not fit one device, the default plan still gives tables to at least one group"""
    import ultragroth_amd as ug
    from ultragroth_amd import synth
    from oracle import closed_form
    if HUGE_LOG == 0:
        pytest.skip("UG_HUGE_LOG=0")
    _, total = device.mem_info()
    if total < (200 << 30):
        pytest.skip("a 2^%d circuit needs a device of 200 GiB or more" % HUGE_LOG)
    zkey, wtns, info = synth.build_circuit(device, HUGE_LOG, mix="U")
    r, s = fixed_rs()
    exp = closed_form.groth16_expected(zkey, wtns, synth.SEEDS, synth.g1_generator_record(), synth.g2_generator_record(),
                                       int.from_bytes(r, "little"), int.from_bytes(s, "little"))
    with ug.Groth16Prover(zkey) as p:
        p.tables_ready(wait=True)
        plan = p.table_plan()
        assert any(c for c, _, _, _ in plan), plan
        assert _prove(p, wtns, r + s) == exp
