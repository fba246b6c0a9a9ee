"""The .r1cs reader and the witness check on host threads (ug_r1cs_parse_info, ug_witness_check with device = -1): no GPU.
The reference is Python integers (tests/r1cs_cases.py). The same irregular and wrap cases run on the device in
tests/test_gpu_r1cs_check.py."""
import struct

import pytest

import r1cs_cases as K
import ultragroth_amd as ug
from ultragroth_amd import synth

R = K.R


def host_check(r1cs, values):
    return ug.witness_check(r1cs, K.wtns_file(values), device=-1)


def assert_matches_python(r1cs, rows, values):
    failing, abc = K.reference(rows, values)
    got = host_check(r1cs, values)
    if not failing:
        assert got is None
        return
    assert got == (len(failing), failing[0], abc[0], abc[1], abc[2], K.message(failing, len(rows)))


def small():
    rows = [({1: 3, 2: R - 1}, {0: 1}, {3: 1}), ({}, {1: 1}, {}), ([(1, 2), (1, 5)], {2: 1, 3: 7, 0: 9}, {4: 1})]
    return rows


def test_writer_and_info_round_trip():
    data = synth.r1cs_file(7, 2, 1, small(), n_prv_in=3, n_labels=1234567890123)
    assert ug.r1cs_info(data) == {"n_wires": 7, "n_pub_out": 2, "n_pub_in": 1, "n_prv_in": 3, "n_constraints": 3,
                                  "n_labels": 1234567890123, "terms": (4, 5, 2)}


def test_sections_are_found_by_id_in_any_order():
    plain = synth.r1cs_file(7, 2, 1, small())
    shuffled = synth.r1cs_file(7, 2, 1, small(), section_order=(3, 2, 1), extra_sections=[(4, b"custom gates" * 5)])
    assert shuffled != plain and ug.r1cs_info(shuffled) == ug.r1cs_info(plain)
    w = [1, 5, 6, 9, 0, 0, 0]
    assert host_check(shuffled, w) == host_check(plain, w)


def _patched(sid, fn, rows=None, n_wires=7):
    secs = K.sections(synth.r1cs_file(n_wires, 2, 1, small() if rows is None else rows))
    return K.binfile(b"r1cs", 1, [(i, fn(p) if i == sid else p) for i, p in secs if not (i == sid and fn is None)])


def _term(wire, coef):
    return struct.pack("<I", wire) + coef.to_bytes(32, "little")


ERRORS = {
    "missing section 1": (lambda: _patched(1, None), "r1cs: section 1 (header) is missing"),
    "short section 1": (lambda: _patched(1, lambda p: p[:-1]), "r1cs: section 1 (header) is too short"),
    "missing section 2": (lambda: _patched(2, None), "r1cs: section 2 (constraints) is missing"),
    "short section 2": (lambda: _patched(2, lambda p: p[:-1]), "r1cs: constraint 2: record runs past the section"),
    "n8": (lambda: _patched(1, lambda p: struct.pack("<I", 31) + p[4:]), "r1cs: n8 is 31, not 32"),
    "prime": (lambda: _patched(1, lambda p: p[:4] + synth.Q_MOD.to_bytes(32, "little") + p[36:]), "r1cs: not over the BN254 scalar field"),
    "wire": (lambda: _patched(2, lambda p: p[:4] + struct.pack("<I", 7) + p[8:]), "r1cs: constraint 0: wire 7 out of range"),
    "coefficient": (lambda: synth.r1cs_file(7, 2, 1, small() + [({}, {}, {2: R})]),
                    "r1cs: constraint 3: coefficient not below the field modulus"),
    "record past the section": (lambda: _patched(2, lambda p: p + struct.pack("<I", 2) + _term(1, 1)),        # a 4th record ...
                                "r1cs: trailing bytes in section 2"),                                           # ... nConstraints says 3
    "count past the section": (lambda: _patched(2, lambda p: struct.pack("<I", 0x7fffffff) + p[4:]),
                               "r1cs: constraint 0: record runs past the section"),
    "trailing": (lambda: _patched(2, lambda p: p + b"\0"), "r1cs: trailing bytes in section 2"),
    "no wires": (lambda: synth.r1cs_file(0, 0, 0, []), "r1cs: nWires is 0"),
}
# (the last rule of the layout, more than 2^32 - 1 terms in one matrix, needs a file of 154 GB: it has no case here)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_layout_errors(name):
    make, text = ERRORS[name]
    data = make()
    with pytest.raises(ug.DeviceError) as e:
        ug.r1cs_info(data)
    assert str(e.value) == text
    with pytest.raises(ug.ProverError) as e:            # ProverError, not a fault tuple: the call left failed = 0
        ug.witness_check(data, K.wtns_file([1] * 7), device=-1)
    assert e.value.message == text and e.value.code == ug.PROVER_ERROR


def test_other_container_is_refused():
    with pytest.raises(ug.ProverError) as e:
        ug.witness_check(K.wtns_file([1]), K.wtns_file([1]), device=-1)
    assert "Invalid file type" in e.value.message


def test_witness_of_another_length():
    data = synth.r1cs_file(7, 2, 1, small())
    with pytest.raises(ug.ProverError) as e:
        ug.witness_check(data, K.wtns_file([1] * 6), device=-1)
    assert e.value.code == ug.PROVER_INVALID_WITNESS_LENGTH and e.value.message == "Invalid witness length. Circuit: 7, witness: 6"


def test_trapdoor_circuit_holds():
    mod, rows, data = K.trapdoor()
    info = ug.r1cs_info(data)
    assert info["n_constraints"] == 430 == len(rows) and info["n_wires"] == mod.N_VARS
    assert len(rows[-1][0]) == 364                       # the lookup identity's A row
    assert ug.witness_check(data, K.golden("groth16.wtns"), device=-1) is None


def test_trapdoor_circuit_with_inv1_0_changed():
    mod, rows, data = K.trapdoor()
    w = K.wtns_values(K.golden("groth16.wtns"))
    w[mod.INV1] = (w[mod.INV1] + 1) % R
    failing, _ = K.reference(rows, w)
    assert failing == [1, 429]                           # its own inverse constraint and the lookup identity
    assert_matches_python(data, rows, w)


@pytest.mark.parametrize("m", K.CONSTRAINT_COUNTS)
def test_irregular_circuits(m):
    n, rows, good, bad, broken = K.irregular(m)
    data = synth.r1cs_file(n, 0, 0, rows)
    assert host_check(data, good) is None
    got = host_check(data, bad)
    _, abc = K.reference(rows, bad)
    assert got == (len(broken), broken[0], abc[0], abc[1], abc[2], K.message(broken, m))


def test_wrap_cases():
    n, rows, w = K.wrap_circuit()
    data = synth.r1cs_file(n, 0, 0, rows)
    assert host_check(data, w) is None
    for bad, failing in K.wrap_broken():
        assert_matches_python(data, rows, bad)
