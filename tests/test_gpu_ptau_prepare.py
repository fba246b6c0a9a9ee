"""Preparing a powers-of-tau file for phase 2 on the device (ptau_prepare.hip): the inverse transform over points as kernels, through
ultragroth_amd.points_intt / ptau_prepare / ptau_check with device = 0. Every comparison is byte for byte: the CPU oracle's
multiples of the transformed integers for one transform; for whole files the test writer's file (sections 12 - 15 from Lagrange
VALUES of the known tau) and the host path (device = -1), which tests/test_ptau_prepare_host.py holds against the same."""
import pytest

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ptau_prepare_cases as PP

pytestmark = pytest.mark.gpu
FIXED_DELTA = PC.FIXED_DELTA
# A lane is a butterfly, so a transform of 2^n has 2^(n-1) lanes per stage; workgroups are 128 lanes for G1 and 64 for G2
# (setup_dev.hpp: S1::BLOCK, S2::BLOCK). 0: no kernel; 1: no twiddle; 2: the first real twiddle; 6, 7: half a wave and one wave;
# G1 8, 9: one workgroup and two; 10: four, strides that cross them. G2 7, 8: one workgroup and two; 9: four.
SIZES = [(False, n) for n in (0, 1, 2, 6, 7, 8, 9, 10)] + [(True, n) for n in (0, 1, 2, 6, 7, 8, 9)]


@pytest.mark.parametrize("g2,log_n", SIZES, ids=["%s-%d" % ("g2" if g else "g1", n) for g, n in SIZES])
def test_points_intt_against_the_integers(device, g2, log_n):
    """every input set of ptau_prepare_cases up to 2^7, the random and the equal-points sets above: random k_j, tau^j, all equal
    (doublings and infinities in the first stage), alternating signs (sums at infinity), all infinity, a single finite point in
    three places, fewer points than the size"""
    import ultragroth_amd as ug
    for name in PP.sets_for(log_n):
        given, want = PP.case(name, log_n, g2)
        got = ug.points_intt(list(given), log_n, g2=g2, device=0)
        assert got == list(want), (name, [i for i in range(len(want)) if got[i] != want[i]][:8])


@pytest.mark.parametrize("power", [6, 10])
def test_prepared_file_equals_the_writers_and_the_host_path(device, power):
    import ultragroth_amd as ug
    raw = PC.ptau(power, prepared=False)
    ms = {}
    dev = ug.ptau_prepare(raw, device=0, timings=ms)
    assert dev == PC.ptau(power)
    assert dev == ug.ptau_prepare(raw, device=-1)
    assert all(v >= 0 for v in ms.values())


def test_prepared_file_of_power_13(device):
    """the file whose points the device made: whole against the writer's, and sections 13, 14 and 15 whole against the host path,
    level by level (the host's transform of the first 2^p records of sections 3, 4 and 5, p = 0 .. 13)"""
    import ultragroth_amd as ug
    want = PC.ptau(13, device=0)
    raw = PC.with_sections(want, drop=PP.LAGRANGE_IDS)
    dev = ug.ptau_prepare(raw, device=0)
    assert dev == want
    secs = PP.sections(dev)
    for src, sid in ((3, 13), (4, 14), (5, 15)):
        size = PP.RECORD[sid]
        powers = [secs[src][size * i:size * i + size] for i in range(1 << 13)]
        host = b"".join(b"".join(ug.points_intt(powers[:1 << p], p, g2=(sid == 13), device=-1)) for p in range(14))
        assert len(host) == size * ((2 << 13) - 1)
        assert secs[sid] == host, sid


def test_power_cut_on_the_device(device):
    import ultragroth_amd as ug
    got = RC.sections(ug.ptau_prepare(PC.ptau(10, prepared=False), power=7, device=0))
    want = RC.sections(PC.ptau(7))
    assert [i for i, _ in got] == [i for i, _ in want]
    assert got[1:] == want[1:]
    a, b = PP.header_fields(got[0][1]), PP.header_fields(want[0][1])
    assert (a["power"], a["ceremony_power"], b["ceremony_power"]) == (7, 10, 7)
    assert all(a[k] == b[k] for k in ("n8", "prime", "rest"))


@pytest.mark.parametrize("power", [6, 10, 13])
def test_check_accepts_the_file_and_names_each_planted_record(device, power):
    import ultragroth_amd as ug
    good = PC.ptau(13, device=0) if power == 13 else PC.ptau(power)
    assert ug.ptau_check(good, device=0) is None
    for sid, record in PP.plants(power):
        hit = ug.ptau_check(PP.planted(good, sid, record), device=0)
        assert hit == (sid, record, "ptau: section %d point %d: does not match the powers" % (sid, record)), (sid, record, hit)


def test_unprepared_file_to_key(device):
    """ceremony output -> prepared file -> key, all on the device: the key of the prepared file is dev_setup's for the trapdoor"""
    import ultragroth_amd as ug
    _, _, r1cs = RC.trapdoor()
    prepared = ug.ptau_prepare(PC.ptau(11, prepared=False))
    zkey, vkey, _ = ug.setup_from_ptau(r1cs, prepared, delta=FIXED_DELTA, log_domain=10)
    assert (zkey, vkey) == PC.dev_setup_key(r1cs, FIXED_DELTA, 10)
