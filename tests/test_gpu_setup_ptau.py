"""The phase-2 setup from a prepared powers-of-tau file on the device (setup_points.hip): the per-wire point combinations and the
one-scalar-times-many-points step as kernels, through ultragroth_amd.setup_from_ptau / points_combine / points_scale with
device = 0. Every comparison is byte for byte: the host path (device = -1) and dev_setup's host path for the trapdoor
(tau, alpha, beta, gamma = 1, delta), which tests/test_setup_ptau_host.py and tests/test_setup_host.py hold against Python
integers; the CPU oracle for the two tooling calls."""
import json

import pytest

import r1cs_cases as RC
import setup_cases as SC
import setup_ptau_cases as PC

pytestmark = pytest.mark.gpu
R = SC.R
FIXED_DELTA = PC.FIXED_DELTA


@pytest.mark.parametrize("delta", [1, FIXED_DELTA], ids=["delta-1", "delta-fixed"])
def test_fixture_circuit_equals_the_host_path_and_dev_setup(device, delta):
    import ultragroth_amd as ug
    _, _, r1cs = RC.trapdoor()
    arg = None if delta == 1 else delta
    zkey, vkey, ms = ug.setup_from_ptau(r1cs, PC.ptau(11), delta=arg, log_domain=10, device=0)
    host = ug.setup_from_ptau(r1cs, PC.ptau(11), delta=arg, log_domain=10, device=-1)
    assert (zkey, vkey) == host[:2]
    assert (zkey, vkey) == PC.dev_setup_key(r1cs, delta, 10)
    assert ug.zkey_check(zkey, level=2) is None
    assert all(v >= 0 for v in ms.values())


@pytest.mark.parametrize("m,n_pub_out,n_pub_in", [(12, 0, 0), (12, 1, 2), (300, 2, 0)], ids=["12-no-public", "12-three-public", "300"])
def test_irregular_circuit_equals_the_host_path(device, m, n_pub_out, n_pub_in):
    import ultragroth_amd as ug
    _, _, r1cs = SC.odd_circuit(m, n_pub_out, n_pub_in)
    ptau = PC.ptau(10 if m == 300 else 6)                     # (above the domain, 2^9 and 2^5: H is dev_setup's too)
    dev = ug.setup_from_ptau(r1cs, ptau, delta=FIXED_DELTA, device=0, validate=2)
    host = ug.setup_from_ptau(r1cs, ptau, delta=FIXED_DELTA, device=-1, validate=2)
    assert dev[:2] == host[:2]
    assert dev[:2] == PC.dev_setup_key(r1cs, FIXED_DELTA, 0)


@pytest.mark.parametrize("m", [257, 4200], ids=["one-piece", "two-pieces"])
def test_long_column_takes_the_split_path(device, m):
    """wire 0 is named by every row's C: m terms in one column of K (and as many in none of A, B1, B2). Above 256 terms a column is
    cut into pieces of 4 096 terms that workgroups sum: 257 is the smallest such column, 4 200 the smallest with two pieces."""
    import ultragroth_amd as ug
    _, _, r1cs = SC.long_column_circuit(m)
    ptau = PC.ptau(10 if m == 257 else 13, device=0)
    dev = ug.setup_from_ptau(r1cs, ptau, delta=FIXED_DELTA, device=0)
    assert dev[:2] == ug.setup_from_ptau(r1cs, ptau, delta=FIXED_DELTA, device=-1)[:2]
    want_zkey, want_vkey = PC.dev_setup_key(r1cs, FIXED_DELTA, 0)
    if m == 257:
        assert dev[:2] == (want_zkey, want_vkey)
    else:                                                    # power 13 is the domain: H comes from the padded level and differs
        got, want = dict(RC.sections(dev[0])), dict(RC.sections(want_zkey))
        assert dev[1] == want_vkey and all(got[sid] == want[sid] for sid in want if sid != 9) and got[9] != want[9]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("n_cols", PC.COLUMN_COUNTS)
def test_points_combine_against_the_oracle(device, n_cols, g2):
    """setup_ptau_cases.combine_case: every length class in the first, a middle and the last lane of a wave, a whole wave of unit
    terms, more than a whole wave of full-length products, columns that cancel, an empty one, a base at infinity"""
    import ultragroth_amd as ug
    case = PC.combine_case(n_cols)
    assert ug.points_combine(*case, PC.points(g2), g2=g2, device=0) == PC.combine_reference(case, g2)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_points_combine_long_columns(device, g2):
    """one column of 257 terms (one piece), one of 4 200 (two pieces, every class among them), a short one between them and an
    empty one at the end: the sums of the pieces, against the oracle"""
    import random
    import ultragroth_amd as ug
    rng = random.Random(0x10C + g2)
    pool = PC.COEFS + (1, 1, 1, R - 1, R - 1)
    cols = [[(rng.randrange(PC.N_POINTS), rng.choice(pool)) for _ in range(n)] for n in (257, 3, 4200, 0)]
    col_ptr, index, coefs = [0], [], []
    for terms in cols:
        index += [i for i, _ in terms]
        coefs += [c for _, c in terms]
        col_ptr.append(len(index))
    case = (col_ptr, index, coefs)
    assert ug.points_combine(*case, PC.points(g2), g2=g2, device=0) == PC.combine_reference(case, g2)


@pytest.mark.parametrize("n", PC.SCALE_COUNTS)
def test_points_scale_against_the_oracle(device, n):
    """1, 2, r - 1, the window edge scalars, every digit of the non-adjacent form at +7 and at -7; infinity in the first and the
    last lane of a wave and at the end"""
    import ultragroth_amd as ug
    _, pts = PC.scale_points(n)
    for s in PC.scale_scalars(n):
        assert ug.points_scale(s, pts, device=0) == PC.scale_reference(n, s), "scalar %d" % s
    assert ug.points_scale(0, pts, device=0) == [bytes(64)] * n


def test_a_planted_bad_point_is_found_only_where_it_is_read(device):
    import ultragroth_amd as ug
    _, _, r1cs = SC.odd_circuit(12, 0, 0)
    good = PC.ptau(6)
    sec12 = dict(RC.sections(good))[12]

    def planted(record):
        p = bytearray(sec12)
        p[record * 64] ^= 1
        return PC.with_sections(good, {12: bytes(p)})

    for record in (31 + 7, 63 + 9):                          # level 5; an odd record of level 6
        with pytest.raises(ug.SetupError) as e:
            ug.setup_from_ptau(r1cs, planted(record), device=0)
        assert str(e.value) == "ptau: section 12 point %d: not on the curve" % record
    key = ug.setup_from_ptau(r1cs, good, device=0)[0]
    for record in (15 + 2, 63 + 8, 127 + 5):                 # level 4, an even record of level 6, level 7
        assert ug.setup_from_ptau(r1cs, planted(record), device=0)[0] == key


def test_end_to_end_drawn_delta_proves_and_verifies(device):
    """fixture circuit and witness: key from the synthesized .ptau with a drawn delta -> Groth16Prover -> groth16_verify under
    the emitted key accepts, a tampered public input is rejected; a second draw changes delta1 and leaves A, B1, B2, IC alone"""
    import ultragroth_amd as ug
    _, _, r1cs = RC.trapdoor()
    wtns = RC.golden("groth16.wtns")
    zkey, vkey, _ = ug.setup_from_ptau(r1cs, PC.ptau(11), delta="draw", log_domain=10, device=0)
    assert ug.zkey_check(zkey, level=2) is None
    with ug.Groth16Prover(zkey) as p:
        proof, pub = p.prove(wtns)
    assert ug.groth16_verify(proof, pub, vkey)
    inputs = json.loads(pub)
    bad = json.dumps([str((int(inputs[0]) + 1) % R)] + inputs[1:])
    assert not ug.groth16_verify(proof, bad, vkey)
    again, vkey2, _ = ug.setup_from_ptau(r1cs, PC.ptau(11), delta="draw", log_domain=10, device=0)
    a, b = dict(RC.sections(zkey)), dict(RC.sections(again))
    for sid in (3, 5, 6, 7):
        assert a[sid] == b[sid], "section %d" % sid
    assert a[2][-192:-128] != b[2][-192:-128] and vkey["vk_delta_2"] != vkey2["vk_delta_2"]
