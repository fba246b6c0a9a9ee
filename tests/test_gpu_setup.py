"""The development setup on the device (setup.hip): Lagrange evaluation, the transposed sparse products and the fixed-base
generator multiplications as kernels, through ultragroth_amd.dev_setup / generator_mul / lagrange_at with device = 0. The keys
are TEST keys (the trapdoor is known). Every comparison is byte for byte: the committed trapdoor fixtures, the CPU oracle, the
generator script's Lagrange values, and the host path (device = -1), which tests/test_setup_host.py holds against Python integers."""
import json

import pytest

import r1cs_cases as RC
import setup_cases as SC

pytestmark = pytest.mark.gpu
R = SC.R


def test_groth16_key_equals_the_fixture(device):
    import ultragroth_amd as ug
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), "groth16", log_domain=10, device=0)
    assert zkey == RC.golden("groth16.zkey")
    assert vkey == json.loads(RC.golden("groth16_vkey.json"))


def test_ultragroth_key_equals_the_fixture(device):
    import ultragroth_amd as ug
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), "ultragroth", log_domain=10, device=0, ultra=SC.ultra_spec())
    assert zkey == RC.golden("ultra.zkey")
    assert vkey == json.loads(RC.golden("ultra_vkey.json"))


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("n", SC.GEN_MUL_COUNTS)
def test_generator_mul_against_the_oracle(device, n, g2):
    """the default window widths; zeros in the first, middle and last lane of a wave and as a whole wave (setup_cases.gen_mul_scalars)"""
    import ultragroth_amd as ug
    scalars = SC.gen_mul_scalars(n)
    assert ug.generator_mul(scalars, g2=g2, device=0) == SC.oracle_muls(scalars, g2)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("window", [4, 8, 11, 13, 16])
def test_generator_mul_edge_scalars_at_every_width(device, window, g2):
    """all digits at the maximum (the carry runs to the top window), one digit alone at half and half + 1, the top window alone,
    r - 1: at the narrowest and widest widths and the ones the edge scalars were made for"""
    import ultragroth_amd as ug
    scalars = SC.edge_scalars()
    assert ug.generator_mul(scalars, g2=g2, device=0, window=window) == SC.oracle_muls(scalars, g2)


@pytest.mark.parametrize("log_n,coset", [(1, False), (1, True), (2, False), (2, True), (10, False), (10, True)])
def test_lagrange_at_against_the_generator(device, log_n, coset):
    """N = 2: a lane's eight values reach past the domain; N = 4; N = 2^10 against the generator script's own lagrange_at"""
    import ultragroth_amd as ug
    x = int(SC.trapdoor_dict()["tau"])
    got = ug.lagrange_at(x, log_n, coset=coset, device=0)
    assert got == SC.lagrange_reference(x, log_n, coset)
    if log_n == 10:
        shift = pow(5, (R - 1) >> 11, R) if coset else 1
        assert got == RC.trapdoor_module().lagrange_at(x, shift)


@pytest.mark.parametrize("m,n_pub_out,n_pub_in", [(12, 0, 0), (12, 1, 2), (300, 2, 0)], ids=["12-no-public", "12-three-public", "300"])
def test_irregular_circuit_equals_the_host_path(device, m, n_pub_out, n_pub_in):
    import ultragroth_amd as ug
    _, _, r1cs = SC.odd_circuit(m, n_pub_out, n_pub_in)
    t = SC.trapdoor_dict()
    dev = ug.dev_setup(r1cs, t, device=0)
    host = ug.dev_setup(r1cs, t, device=-1)
    assert dev[0] == host[0] and dev[1] == host[1]
    assert ug.zkey_check(dev[0], level=2) is None                   # the key validator accepts what the key maker makes


@pytest.mark.parametrize("m", [257, 4200], ids=["one-piece", "two-pieces"])
def test_long_column_takes_the_split_path(device, m):
    """wire 0 is named by every row's C: m terms in one column. Above 256 terms a column is cut into pieces of 4 096 terms that
    workgroups sum; 257 is the smallest such column (one piece), 4 200 the smallest size class with a second piece to combine."""
    import ultragroth_amd as ug
    _, _, r1cs = SC.long_column_circuit(m)
    assert ug.r1cs_info(r1cs)["terms"][2] == 2 * m
    t = SC.trapdoor_dict()
    assert ug.dev_setup(r1cs, t, device=0)[0] == ug.dev_setup(r1cs, t, device=-1)[0]


def test_ultragroth_irregular_equals_the_host_path(device):
    import ultragroth_amd as ug
    n_wires, _, r1cs = SC.odd_circuit(12, 1, 2)
    private = list(range(4, n_wires))
    spec = {"rand_indx": 3, "round_signals": private[1::2], "final_signals": private[0::2]}
    t = SC.trapdoor_dict()
    dev = ug.dev_setup(r1cs, t, "ultragroth", device=0, ultra=spec)
    host = ug.dev_setup(r1cs, t, "ultragroth", device=-1, ultra=spec)
    assert dev[0] == host[0] and dev[1] == host[1]


def test_end_to_end_sparse_b_proof_verifies(device):
    """2^14: the smallest size at which the prover keeps B1 / B2 compacted (sparse B). dev_setup -> Groth16Prover -> proof ->
    groth16_verify with the emitted key: accepted, and rejected with a tampered public input. The first proof of that path that
    satisfies a verifier equation."""
    import ultragroth_amd as ug
    r1cs, wtns, out = SC.sparse_b_circuit()
    assert ug.witness_check(r1cs, wtns) is None
    zkey, vkey, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), device=0)       # (a fixed trapdoor: a failure can be reproduced)
    n_vars, n_public, domain = SC.zkey_header(zkey)
    assert n_vars >= 1 << 14 and domain == 1 << 14 and n_public == 1
    assert ug.zkey_check(zkey, level=2) is None
    with ug.Groth16Prover(zkey) as p:
        assert len(p.table_plan()) == 3                             # the third schedule group only the sparse-B form has
        proof, pub = p.prove(wtns)
    assert json.loads(pub) == [str(out)]
    assert ug.groth16_verify(proof, pub, vkey)
    assert not ug.groth16_verify(proof, json.dumps([str((out + 1) % R)]), vkey)
