"""UltraGroth keys from a prepared powers-of-tau file on the device: the point combinations of setup_points.hip and the whole
delta step -- C1, C2 and H, gathered through the signal lists -- as ONE launch of scale_segments_kernel, through
ultragroth_amd.ultra_setup_from_ptau / points_scale_segments with device = 0. Every comparison is byte for byte: the host path
(device = -1) and dev_setup's host path for protocol 1337 and the trapdoor (tau, alpha, beta, gamma = 1, delta_round,
delta_final), which tests/test_ultra_keys_host.py holds; setup_ptau_cases.scale_reference for the tooling call."""
import json

import pytest

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC
import ultra_keys_cases as UC

pytestmark = pytest.mark.gpu
R = SC.R


@pytest.mark.parametrize("d_round,d_final", UC.DELTA_PAIRS, ids=["ones", "round", "both"])
def test_fixture_circuit_equals_the_host_path_and_dev_setup(device, d_round, d_final):
    import ultragroth_amd as ug
    r1cs, spec, power, log_domain = UC.fixture()
    arg = UC.delta_arg(d_round, d_final)
    zkey, vkey, ms = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta=arg, log_domain=log_domain, device=0)
    host = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta=arg, log_domain=log_domain, device=-1)
    assert (zkey, vkey) == host[:2]
    assert (zkey, vkey) == UC.dev_key(r1cs, spec, d_round, d_final, log_domain)
    assert ug.zkey_check(zkey, level=2) is None
    assert all(v >= 0 for v in ms.values())


@pytest.mark.parametrize("kind", ["alternating", "no-round", "no-final", "descending"])
def test_irregular_circuit_and_list_shapes(device, kind):
    import ultragroth_amd as ug
    r1cs, spec = UC.irregular(kind)
    for d_round, d_final in UC.DELTA_PAIRS:
        arg = UC.delta_arg(d_round, d_final)
        dev = ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta=arg, device=0, validate=2)
        assert dev[:2] == ug.ultra_setup_from_ptau(r1cs, PC.ptau(6), spec, delta=arg, device=-1, validate=2)[:2]
        assert dev[:2] == UC.dev_key(r1cs, spec, d_round, d_final)
    assert ug.zkey_check(dev[0], level=2) is None


def test_long_column_takes_the_split_path(device):
    """wire 0's column of C has 257 terms, the smallest that is cut into pieces; 171 round and 342 final signals: each of the
    three segments of the delta step spans more than one workgroup and ends inside one"""
    import ultragroth_amd as ug
    r1cs, spec = UC.long_column()
    assert len(spec["round_signals"]) == 171 and len(spec["final_signals"]) == 342
    ptau = PC.ptau(10, device=0)
    dev = ug.ultra_setup_from_ptau(r1cs, ptau, spec, delta=(UC.FIXED_DELTA, UC.OTHER_DELTA), device=0)
    assert dev[:2] == ug.ultra_setup_from_ptau(r1cs, ptau, spec, delta=(UC.FIXED_DELTA, UC.OTHER_DELTA), device=-1)[:2]
    assert dev[:2] == UC.dev_key(r1cs, spec, UC.FIXED_DELTA, UC.OTHER_DELTA)


@pytest.mark.parametrize("which", range(len(UC.SEGMENT_COUNTS)), ids=["%d-%d-%d" % c for c in UC.SEGMENT_COUNTS])
def test_points_scale_segments_against_the_oracle(device, which):
    import ultragroth_amd as ug
    segments, pts = UC.segment_case(which)
    timing = []
    got = ug.points_scale_segments(segments, pts, device=0, timing=timing)
    assert got == UC.segment_reference(which)
    assert got == ug.points_scale_segments(segments, pts, device=-1)
    assert len(timing) == 1 and timing[0] >= 0


def test_points_scale_segments_one_segment_is_points_scale(device):
    import ultragroth_amd as ug
    _, pts = PC.scale_points(65)
    assert ug.points_scale_segments([(PC.SEVENS, None, 65)], pts, device=0) == [ug.points_scale(PC.SEVENS, pts, device=0)]
    assert ug.points_scale_segments([(PC.SEVENS, None, 0), (2, [], 0)], pts, device=0) == [[], []]
    assert ug.points_scale_segments([], pts, device=0) == []


def test_end_to_end_drawn_key_proves_and_verifies(device):
    """the fixture circuit: ultra_setup_from_ptau with drawn deltas -> UltraGrothProver on ultra.uwtns -> ultra_groth_verify under
    the emitted key: accepted, and rejected with a tampered public input. A second draw changes delta_c1, delta_c2 and what they
    divide, and leaves sections 3 - 7 alone."""
    import ultragroth_amd as ug
    r1cs, spec, power, log_domain = UC.fixture()
    zkey, vkey, _ = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta="draw", log_domain=log_domain, device=0, validate=2)
    assert ug.zkey_check(zkey, level=2) is None
    assert ug.ultra_zkey_verify(r1cs, PC.ptau(power), zkey, ultra=spec, device=0) is None
    vk = json.dumps(vkey)
    with ug.UltraGrothProver(zkey) as p:
        proof, pub = p.prove(RC.golden("ultra.uwtns"))
    assert ug.ultra_groth_verify(proof, pub, vk)
    values = json.loads(pub)
    bad = json.dumps([str((int(values[0]) + 1) % R)] + values[1:])
    assert not ug.ultra_groth_verify(proof, bad, vk)
    assert not ug.ultra_groth_verify(proof, pub, RC.golden("ultra_vkey.json").decode())       # another key's deltas
    again = ug.ultra_setup_from_ptau(r1cs, PC.ptau(power), spec, delta="draw", log_domain=log_domain, device=0)[0]
    a, b = dict(RC.sections(zkey)), dict(RC.sections(again))
    for sid in (3, 4, 5, 6, 7, 10, 11):
        assert a[sid] == b[sid], "section %d" % sid
    assert a[2][:-384] == b[2][:-384] and a[2][-384:-192] != b[2][-384:-192] and a[2][-192:] != b[2][-192:]
    assert a[8] != b[8] and a[9] != b[9] and a[12] != b[12]
