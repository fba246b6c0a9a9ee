"""Device memory of the inner layer (ultragroth_amd/csrc/dev_common.hpp: DevBuf, PinnedBuf): every handle kind gives back what
it took, and so does every call that refuses after it has allocated. The measure is Device.mem_info(), as in
test_gpu_r1cs_check.py and test_gpu_validate.py: the free bytes after a cycle equal the free bytes before it. A cycle runs once
before the first reading, so that what the runtime and the context keep after a first use (code objects, the MSM workspaces, the
plan of ug_fr_ntt) is there already.

All shapes are small: 2^10 points, a domain of 2^10, an .r1cs of 257 constraints. Window tables take the narrowest width the
library accepts (16). Sums are checked against the closed form of the generator walk (synth.synth_points: P_i = (seed + i) G)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import r1cs_cases as K
import ultragroth_amd as ug
from test_gpu_validate import bump_y, put
from ultragroth_amd import synth

pytestmark = pytest.mark.gpu

N = 1 << 10
TABLE_C = 16
SEEDS = {"A": 0x2468_0001, "B": 0x2468_0003, "C": 0x2468_0005, "G2": 0x2468_0007}
LOGN, NVARS = 10, 300


@pytest.fixture(scope="module")
def data(device):
    """points, scalars and the expected sums, computed once and never changed"""
    d = {k: bytes(synth.synth_points(device, N, s, g2=(k == "G2"))) for k, s in SEEDS.items()}
    sc = synth.scalars(N, "C", 0xD0D0).tobytes()
    d["sc"] = sc
    for k, s in SEEDS.items():
        walk = O.fr_dot_walk(sc, N, s)
        d["sum" + k] = O.g2_mul(synth.g2_generator_record(), walk) if k == "G2" else O.g1_mul(synth.g1_generator_record(), walk)
    # every second point of A: sum s_i (seed + 2 i) G = (2 sum s_i (seed + i) - seed sum s_i) G over the first N / 2 scalars
    half = N // 2
    dot, total = O.fr_dot_walk(sc, half, SEEDS["A"]), O.fr_dot_walk(sc, half, 1) - O.fr_dot_walk(sc, half, 0)
    d["sumEvery"] = O.g1_mul(synth.g1_generator_record(), (2 * dot - SEEDS["A"] * total) % O.R_MOD)
    domain = 1 << LOGN
    d["coefs"] = synth.coefficients(domain, NVARS, 0xC0EF).tobytes()
    d["wtns"] = synth.scalars(NVARS, "U", 0x77).tobytes()
    d["h"] = O.hpoly(d["coefs"], 4 * domain, d["wtns"], NVARS, domain)
    return d


def drop(*handles):
    for h in handles:
        h._destroy(h.h)
        h.h = None


def free_bytes(device):
    assert device._L.ug_ctx_sync(device._h) == 0          # (staging memory of queued set-up work goes when the stream is idle)
    return device.mem_info()[0]


def returns(device, cycle, times=3):
    cycle()
    before = free_bytes(device)
    for _ in range(times):
        cycle()
    assert free_bytes(device) == before


def refused(L, rc, text):
    assert rc != 0 and text in L.ug_last_error().decode(), L.ug_last_error()


def raw_bases(device, fn, *args):
    h = C.c_void_p()
    rc = getattr(device._L, fn)(device._h, *args, C.byref(h))
    assert rc == 0, device._L.ug_last_error()
    return ug._Handle(h, device._L.ug_bases_destroy, device)


def group_members(d, last=None):
    """A | B | C, C five scalars in; last: member 2's last record"""
    shift = 5
    c = d["C"][:64 * (N - shift)]
    if last is not None:
        c = put(c, N - shift - 1, last)
    return [(d["A"], N, 0), (d["B"], N, 0), (c, N - shift, shift)], shift


# ---- life cycles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_plain_bases(device, data, g2):
    key = "G2" if g2 else "A"

    def cycle():
        b = device.bases(data[key], N, g2=g2)
        v = device.dvec(N, data["sc"])
        s = device.schedule(v, 0, N)
        assert device.msm(b, s, g2=g2) == data["sum" + key]
        drop(s, v, b)

    returns(device, cycle)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_bases_with_tables(device, data, g2, stride):
    key = "G2" if g2 else "A"

    def cycle():
        b = raw_bases(device, "ug_bases_create_tables_strided_g2" if g2 else "ug_bases_create_tables_strided_g1", data[key], N, 0, TABLE_C, stride)
        v = device.dvec(N, data["sc"])
        s = device.schedule(v, 0, N, table_c=TABLE_C, table_stride=stride)
        assert device.msm(b, s, g2=g2) == data["sum" + key]
        drop(s, v, b)

    returns(device, cycle)


@pytest.mark.parametrize("table_c", [0, TABLE_C], ids=["plain", "tables"])
def test_group(device, data, table_c):
    members, shift = group_members(data)
    exp_c = O.g1_mul(synth.g1_generator_record(), O.fr_dot_walk(data["sc"][32 * shift:], N - shift, SEEDS["C"]))

    def cycle():
        g = device.bases_group(members, 0, N, table_c=table_c)
        v = device.dvec(N, data["sc"])
        s = device.schedule(v, 0, N, table_c=table_c)
        assert device.msm_group(g, s) == [data["sumA"], data["sumB"], exp_c]
        drop(s, v, g)

    returns(device, cycle)


def test_bases_create_every(device, data):
    def cycle():
        b = raw_bases(device, "ug_bases_create_every_g1", data["A"], N, 0, 2, 0)
        v = device.dvec(N // 2, data["sc"][:32 * (N // 2)])
        s = device.schedule(v, 0, N // 2)
        assert device.msm(b, s) == data["sumEvery"]
        drop(s, v, b)

    returns(device, cycle)


def test_precompute_then_drop_tables(device, data):
    L = device._L

    def cycle():
        b = device.bases(data["A"], N, table_c=TABLE_C)
        v = device.dvec(N, data["sc"])
        s = device.schedule(v, 0, N, table_c=TABLE_C)
        assert device.msm(b, s) == data["sumA"]
        assert L.ug_bases_drop_tables(b.h) == 0 and L.ug_bases_table_window(b.h) == 0
        s2 = device.schedule(v, 0, N)
        assert device.msm(b, s2) == data["sumA"]
        drop(s, s2, v, b)

    returns(device, cycle)


@pytest.mark.parametrize("called_off", [False, True], ids=["built", "called_off"])
def test_deferred_tables(device, data, called_off):
    """ug_ctx_defer_tables: tables_alloc / adopt / step to the end; or the build called off with drop_tables before the adoption,
    which then gives the room back"""
    L = device._L

    def cycle():
        assert L.ug_ctx_defer_tables(device._h, 1) == 0
        try:
            b = raw_bases(device, "ug_bases_create_tables_strided_g1", data["A"], N, 0, TABLE_C, 2)
        finally:
            L.ug_ctx_defer_tables(device._h, 0)
        mem = C.c_void_p()
        assert L.ug_bases_tables_alloc(b.h, C.byref(mem)) == 0 and mem.value
        v = device.dvec(N, data["sc"])
        if called_off:
            assert L.ug_bases_drop_tables(b.h) == 0
            assert L.ug_bases_tables_adopt(b.h, mem) == 0 and L.ug_bases_table_window(b.h) == 0
            s = device.schedule(v, 0, N)
        else:
            assert L.ug_bases_tables_adopt(b.h, mem) == 0 and L.ug_bases_table_window(b.h) == TABLE_C
            left = C.c_uint64(1)
            while left.value:
                assert L.ug_bases_tables_step(b.h, C.c_uint64(400), C.byref(left)) == 0
            assert L.ug_bases_tables_ready(b.h) == 1
            s = device.schedule(v, 0, N, table_c=TABLE_C, table_stride=2)
        assert device.msm(b, s) == data["sumA"]
        drop(s, v, b)

    returns(device, cycle)


def test_dvec_and_index(device, data):
    L = device._L
    sc = data["sc"]
    el = lambda i: sc[32 * i:32 * i + 32]
    idx = np.array([5, 0, 1023, 5, 77], dtype=np.uint32)

    def cycle():
        src, out = device.dvec(N, sc), device.dvec(8, bytes(32 * 8))
        assert L.ug_dvec_gather(out.h, src.h, idx.ctypes.data, len(idx)) == 0
        assert device.download(out, 0, 5) == b"".join(el(i) for i in idx)
        device.gather_index_at(out, 3, src, idx[:4])
        assert device.download(out, 3, 4) == b"".join(el(i) for i in idx[:4])
        where = np.array([7, 2], dtype=np.uint32)
        assert L.ug_dvec_scatter(out.h, where.ctypes.data, el(9) + el(10), 2) == 0
        got = device.download(out, 0, 8)
        assert got[32 * 7:] == el(9) and got[64:96] == el(10)
        drop(src, out)

    returns(device, cycle)


def test_schedule_trim(device, data):
    L = device._L

    def cycle():
        b = device.bases(data["A"], N)
        v = device.dvec(N, data["sc"])
        s = device.schedule(v, 0, N)
        assert L.ug_schedule_trim(s.h) == 0
        assert L.ug_schedule_build(s.h, v.h, 0, N) == 0          # a trimmed schedule builds again
        assert device.msm(b, s) == data["sumA"]
        assert L.ug_schedule_trim(s.h) == 0
        drop(s, v, b)

    returns(device, cycle)


def test_hpoly_reserve_vectors(device, data):
    domain = 1 << LOGN

    def cycle():
        hp = device.hpoly(data["coefs"], 4 * domain, domain, NVARS)
        w = device.dvec(NVARS, data["wtns"])
        for group in (1, 4, 2, 1):
            hp.reserve_vectors(group)
            h = hp.run(w)
            assert device.download(h, 0, domain) == data["h"]
            drop(h)
        drop(w, hp)

    returns(device, cycle)


@pytest.mark.parametrize("want_mask", [False, True], ids=["no_mask", "mask"])
def test_r1cs(device, want_mask):
    n, rows, good, bad, broken = K.irregular(257)
    file = synth.r1cs_file(n, 0, 0, rows)
    wtns = b"".join(int(x).to_bytes(32, "little") for x in bad)

    def cycle():
        cs = device.r1cs(file)
        w = device.dvec(n, wtns)
        got = cs.check(w, want_mask=want_mask)
        assert got["failed"] == len(broken) and got["first"] == broken[0]
        if want_mask:
            assert got["mask"] == bytes(1 if k in set(broken) else 0 for k in range(len(rows)))
        cs.close()
        drop(w)

    returns(device, cycle)


def test_one_shot_calls(device, data):
    """ug_fr_ntt, ug_field_op, ug_synth_points: their scratch buffers"""
    vec = synth.scalars(1 << LOGN, "U", 0x51).tobytes()
    a, b = data["sc"][:32 * 16], data["sc"][32 * 16:32 * 32]

    def cycle():
        assert device.ntt(device.ntt(vec, LOGN), LOGN, inverse=True) == vec
        assert device.field_op(ug.FR, ug.OP_MUL, a, b) == device.field_op(ug.FR, ug.OP_MUL, b, a)
        assert bytes(synth.synth_points(device, 33, SEEDS["A"])) == data["A"][:64 * 33]

    returns(device, cycle)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_point_checks(device, data, g2):
    key, rec = ("G2", 128) if g2 else ("A", 64)
    bad = put(data[key], N - 1, bump_y(data[key][-rec:]))

    def cycle():
        assert device.check_points(data[key], N, g2=g2, level=2) is None
        assert device.check_points(bad, N, g2=g2, level=2) == (N - 1, ug.UG_POINT_OFF_CURVE)
        assert device.points_check_mask(bad, N, g2=g2, level=2) == bytes(N - 1) + bytes([ug.UG_POINT_OFF_CURVE])

    returns(device, cycle)


def test_whole_context(device, data):
    """a context of its own, used and closed: the readings are the session context's"""
    domain = 1 << LOGN

    def cycle():
        d = ug.Device(0)
        try:
            b, b2 = d.bases(data["A"], N), d.bases(data["G2"], N, g2=True)
            g = d.bases_group(group_members(data)[0], 0, N)
            v = d.dvec(N, data["sc"])
            s = d.schedule(v, 0, N)
            assert d.msm(b, s) == data["sumA"]
            assert d.msm_witness(g, b2, s)[3] == data["sumG2"]
            hp = d.hpoly(data["coefs"], 4 * domain, domain, NVARS)
            w = d.dvec(NVARS, data["wtns"])
            h = hp.run(w)
            assert d.download(h, 0, domain) == data["h"]
            d.ntt(data["sc"][:32 * 16], 4)
            d.check_on_create(1)
            assert d._L.ug_ctx_trim(d._h) == 0
            assert d.msm(b, s) == data["sumA"]                   # the workspaces come back after a trim
            drop(h, w, hp, s, v, g, b2, b)
        finally:
            d.close()

    returns(device, cycle)


# ---- refusals behind an allocation ------------------------------------------------------------------------------------------------
def test_refused_hpoly_create(device, data):
    domain = 1 << LOGN
    rec = np.frombuffer(data["coefs"], dtype=synth.COEF_DTYPE).copy()
    rec["s"][-1] = NVARS                                          # one signal index past the witness
    bad = rec.tobytes()
    drop(device.hpoly(data["coefs"], 4 * domain, domain, NVARS))
    before = free_bytes(device)
    for _ in range(3):
        with pytest.raises(ug.DeviceError, match="coefficient record out of range"):
            device.hpoly(bad, 4 * domain, domain, NVARS)
    assert free_bytes(device) == before
    hp = device.hpoly(data["coefs"], 4 * domain, domain, NVARS)
    w = device.dvec(NVARS, data["wtns"])
    assert device.download(hp.run(w), 0, domain) == data["h"]


def test_refused_bad_points(device, data):
    """check_on_create(1): a plain set and a 3-member group whose last record (of the third member) is off the curve"""
    L = device._L
    bad = put(data["A"], N - 1, bump_y(data["A"][-64:]))
    last = N - 5 - 1                                              # (member 2 starts five scalars in: group_members)
    members, _ = group_members(data, last=bump_y(data["C"][64 * last:64 * (last + 1)]))
    drop(device.bases(data["A"], N), device.bases_group(group_members(data)[0], 0, N))
    before = free_bytes(device)
    device.check_on_create(1)
    try:
        for _ in range(3):
            with pytest.raises(ug.DeviceError, match="point %d: not on the curve" % (N - 1)):
                device.bases(bad, N)
            with pytest.raises(ug.DeviceError, match="member 2 point %d: not on the curve" % (N - 1)):
                device.bases_group(members, 0, N)
            with pytest.raises(ug.DeviceError, match="member 2 point %d: not on the curve" % (N - 1)):
                device.bases_group(members, 0, N, table_c=TABLE_C)
        b, g = device.bases(data["A"], N), device.bases_group(group_members(data)[0], 0, N)      # good sets still create
        s = device.schedule(device.dvec(N, data["sc"]), 0, N)
        assert device.msm(b, s) == data["sumA"] and device.msm_group(g, s)[1] == data["sumB"]
        drop(s, g, b)
    finally:
        device.check_on_create(0)
    assert free_bytes(device) == before
    assert L.ug_ctx_sync(device._h) == 0


def test_refused_reserve_vectors(device, data):
    domain = 1 << LOGN
    hp = device.hpoly(data["coefs"], 4 * domain, domain, NVARS)
    w = device.dvec(NVARS, data["wtns"])
    hp.reserve_vectors(2)
    before = free_bytes(device)
    for _ in range(3):
        ug.inject_fault(ug.FAULT_HPOLY_RESERVE)
        with pytest.raises(ug.DeviceError, match="injected fault"):
            hp.reserve_vectors(16)
    assert free_bytes(device) == before
    assert device.download(hp.run(w), 0, domain) == data["h"]      # the old workspaces are still in use
    hp.reserve_vectors(16)
    assert device.download(hp.run(w), 0, domain) == data["h"]
    hp.reserve_vectors(2)
    assert free_bytes(device) == before


def test_refused_schedule_build(device, data):
    b = device.bases(data["A"], N)
    v = device.dvec(N, data["sc"])
    drop(device.schedule(v, 0, N))
    before = free_bytes(device)
    for _ in range(3):
        ug.inject_fault(ug.FAULT_SCHEDULE_BUILD)
        with pytest.raises(ug.DeviceError, match="injected fault"):
            device.schedule(v, 0, N)
    assert free_bytes(device) == before
    s = device.schedule(v, 0, N)
    assert device.msm(b, s) == data["sumA"]


def test_refused_r1cs_create(device):
    """r1cs_cases.py has no refused file of its own: the one of test_gpu_r1cs_check.py is built here. The loader applies every rule
    of the layout before ug_r1cs_create touches the device, so what this guards is that order, not a free."""
    n, rows, good, bad, broken = K.irregular(257)
    wrong = rows[:-1] + [(rows[-1][0], rows[-1][1], {n: 1})]      # a wire out of range in the last constraint
    file = synth.r1cs_file(n, 0, 0, rows)
    device.r1cs(file).close()
    before = free_bytes(device)
    for _ in range(3):
        with pytest.raises(ug.DeviceError, match="constraint 256: wire %d out of range" % n):
            device.r1cs(synth.r1cs_file(n, 0, 0, wrong))
    assert free_bytes(device) == before
    cs = device.r1cs(file)
    assert cs.check(device.dvec(n, b"".join(int(x).to_bytes(32, "little") for x in good)))["failed"] == 0
    cs.close()


def test_refused_gather(device, data):
    L = device._L
    src, out = device.dvec(N, data["sc"]), device.dvec(4)
    idx = np.arange(8, dtype=np.uint32)
    assert L.ug_dvec_gather(out.h, src.h, idx.ctypes.data, 4) == 0
    before = free_bytes(device)
    for _ in range(3):
        refused(L, L.ug_dvec_gather(out.h, src.h, idx.ctypes.data, 8), "gather larger than the output vector")
    assert free_bytes(device) == before
    assert L.ug_dvec_gather(out.h, src.h, idx.ctypes.data, 4) == 0
    assert device.download(out, 0, 4) == data["sc"][:32 * 4]
