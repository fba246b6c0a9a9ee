"""The development setup on host threads (device = -1): include/ultragroth_hip.h ug_setup_*, ug_generator_mul, ug_lagrange_at
through ultragroth_amd.dev_setup / generator_mul / lagrange_at. The keys it makes are TEST keys (the trapdoor is known).
Every comparison is byte for byte: against the committed trapdoor fixtures, the CPU oracle and Python integers."""
import json
import os
import struct
import subprocess

import pytest

import oracle as O
from oracle import pairing
from conftest import ROOT
import sanitized_build
import r1cs_cases as RC
import setup_cases as SC

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
R = SC.R


def _ug():
    import ultragroth_amd as ug
    return ug


def test_groth16_key_equals_the_fixture():
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, used = ug.dev_setup(r1cs, SC.trapdoor_dict(), "groth16", log_domain=10, device=-1)
    assert zkey == RC.golden("groth16.zkey")
    assert vkey == json.loads(RC.golden("groth16_vkey.json"))
    assert used == SC.trapdoor_dict()


def test_ultragroth_key_equals_the_fixture():
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), "ultragroth", log_domain=10, device=-1, ultra=SC.ultra_spec())
    assert zkey == RC.golden("ultra.zkey")
    assert vkey == json.loads(RC.golden("ultra_vkey.json"))


def test_smallest_domain_key_proves_and_verifies():
    """log_domain = 0: 433 rows fit 2^9. The oracle's proof under that key satisfies the verifier equation (pure-Python pairing
    and the product's verifier), and one tampered coordinate does not."""
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    zkey, vkey, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), "groth16", device=-1)
    assert SC.zkey_header(zkey)[2] == 1 << 9
    assert len(zkey) == ug.dev_setup_size(r1cs, SC.trapdoor_dict(), "groth16")
    proof, pub = O.groth16_prove(zkey, RC.golden("groth16.wtns"), 12345, 67890)
    assert pairing.groth16_verify(vkey, pub, proof) and ug.groth16_verify(proof, pub, vkey)
    bad = json.loads(proof)
    bad["pi_a"][0] = str((int(bad["pi_a"][0]) + 1) % O.Q_MOD)
    assert not ug.groth16_verify(json.dumps(bad), pub, vkey)
    bad = json.loads(proof)
    bad["pi_c"][1] = json.loads(proof)["pi_a"][1]
    assert not pairing.groth16_verify(vkey, pub, json.dumps(bad)) and not ug.groth16_verify(json.dumps(bad), pub, vkey)


@pytest.mark.parametrize("protocol", ["groth16", "ultragroth"])
def test_size_query_equals_what_the_run_writes(protocol):
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    ultra = SC.ultra_spec() if protocol == "ultragroth" else None
    for log_domain in (0, 10, 11):
        zkey, _, _ = ug.dev_setup(r1cs, SC.trapdoor_dict(), protocol, log_domain=log_domain, device=-1, ultra=ultra)
        assert len(zkey) == ug.dev_setup_size(r1cs, SC.trapdoor_dict(), protocol, log_domain=log_domain, ultra=ultra)


def test_a_drawn_trapdoor_is_in_range_and_fresh():
    ug = _ug()
    n, rows, r1cs = SC.odd_circuit(12, 1, 1)
    seen = set()
    for _ in range(2):
        zkey, vkey, used = ug.dev_setup(r1cs, None, device=-1)
        assert set(used) == set(ug.TRAPDOOR_KEYS) and all(0 < int(v) < R for v in used.values())
        assert ug.dev_setup(r1cs, used, device=-1)[0] == zkey                 # the returned trapdoor reproduces the key
        seen.add(used["tau"])
    assert len(seen) == 2


def _refused(fn, text):
    ug = _ug()
    with pytest.raises(ug.SetupError) as e:
        fn()
    assert str(e.value).startswith(("setup: ", "r1cs: ")) and text in str(e.value), str(e.value)


def test_refusals():
    ug = _ug()
    _, _, r1cs = RC.trapdoor()
    t = SC.trapdoor_dict()
    run = lambda **kw: ug.dev_setup(r1cs, kw.pop("trapdoor", t), kw.pop("protocol", "groth16"), device=-1, **kw)
    omega10 = pow(5, (R - 1) >> 10, R)
    g = pow(5, (R - 1) >> 11, R)
    _refused(lambda: run(trapdoor=dict(t, tau=str(omega10 ** 3 % R)), log_domain=10), "setup: tau^(2N) = 1")       # tau in the domain
    _refused(lambda: run(trapdoor=dict(t, tau=str(g * omega10 % R)), log_domain=10), "setup: tau^(2N) = 1")        # tau / g in the domain
    _refused(lambda: run(trapdoor=dict(t, tau="1")), "setup: tau^(2N) = 1")
    for k in ("alpha", "beta", "gamma", "delta_final"):
        _refused(lambda: run(trapdoor=dict(t, **{k: "0"})), "setup: %s is 0 mod r" % k)
    _refused(lambda: run(trapdoor=dict(t, delta_round="0"), protocol="ultragroth", ultra=SC.ultra_spec()), "setup: delta_round is 0 mod r")
    for k in ug.TRAPDOOR_KEYS:
        if k != "delta_round":
            _refused(lambda: run(trapdoor=dict(t, **{k: str(R)})), "setup: %s is not below the field modulus" % k)
    _refused(lambda: run(trapdoor=dict(t, tau=str((1 << 256) - 1))), "setup: tau is not below the field modulus")
    _refused(lambda: run(log_domain=8), "setup: log_domain 8 is too small")
    _refused(lambda: run(log_domain=28), "setup: log_domain 28 is above")
    _refused(lambda: run(protocol="ultragroth"), "setup: protocol 1337 needs")
    spec = SC.ultra_spec()
    _refused(lambda: run(protocol="ultragroth", ultra=dict(spec, round_signals=spec["round_signals"][1:])), "do not partition")
    _refused(lambda: run(protocol="ultragroth", ultra=dict(spec, final_signals=spec["final_signals"][:-1] + [spec["round_signals"][0]])), "do not partition")
    _refused(lambda: run(protocol="ultragroth", ultra=dict(spec, final_signals=spec["final_signals"][:-1] + [1])), "do not partition")
    _refused(lambda: run(protocol="ultragroth", ultra=dict(spec, rand_indx=7)), "setup: rand_indx 7")
    _refused(lambda: ug.dev_setup(r1cs[:-5], t, device=-1), "setup: Section")                       # the container's own message
    _refused(lambda: ug.dev_setup(b"zkey" + r1cs[4:], t, device=-1), "setup: ")
    n_wires, rows, _ = SC.odd_circuit(12, 0, 0)
    _refused(lambda: ug.dev_setup(SC.synth.r1cs_file(n_wires - 3, 0, 0, rows[:1] + (({n_wires: 1}, {}, {}),)), t, device=-1), "r1cs: constraint 1: wire")
    # sizes that cannot be represented: a header that claims 2^27 constraints needs a domain above the prover's largest; the
    # options are checked before the constraints are walked, so the (short) section 2 is never reached
    small = SC.synth.r1cs_file(4, 1, 0, [({1: 1}, {2: 1}, {3: 1})])
    at = small.index(struct.pack("<IIIIQI", 4, 1, 0, 2, 4, 1)) + 24
    huge = small[:at] + struct.pack("<I", 1 << 27) + small[at + 4:]
    _refused(lambda: ug.dev_setup(huge, t, device=-1), "setup: sizes that cannot be represented")
    _refused(lambda: ug.dev_setup_size(huge, t), "setup: sizes that cannot be represented")
    _refused(lambda: ug.generator_mul([R], device=-1), "setup: scalar 0 is not below the field modulus")
    _refused(lambda: ug.generator_mul([1], device=-1, window=3), "setup: window 3")
    _refused(lambda: ug.lagrange_at(1, 4, device=-1), "setup: x lies in the evaluation domain")
    _refused(lambda: ug.lagrange_at(3, 0, device=-1), "setup: log_n 0")
    # the library is as usable as before: the same call that made the fixture still makes it
    assert run(log_domain=10)[0] == RC.golden("groth16.zkey")
    assert ug.groth16_verify(*O.groth16_prove(RC.golden("groth16.zkey"), RC.golden("groth16.wtns"), 1, 2), json.loads(RC.golden("groth16_vkey.json")))


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_generator_mul_on_host_threads(g2):
    ug = _ug()
    scalars = SC.edge_scalars() + SC.gen_mul_scalars(65)
    assert ug.generator_mul(scalars, g2=g2, device=-1) == SC.oracle_muls(scalars, g2)
    assert ug.generator_mul([], g2=g2, device=-1) == []


@pytest.mark.parametrize("log_n,coset", [(1, False), (1, True), (2, False), (2, True), (10, False), (10, True)])
def test_lagrange_at_on_host_threads(log_n, coset):
    ug = _ug()
    x = int(SC.trapdoor_dict()["tau"])
    assert ug.lagrange_at(x, log_n, coset=coset, device=-1) == SC.lagrange_reference(x, log_n, coset)
    if log_n == 10:                                # the generator's own function computes with N = 2^10
        mod = RC.trapdoor_module()
        shift = pow(5, (R - 1) >> 11, R) if coset else 1
        assert ug.lagrange_at(x, 10, coset=coset, device=-1) == mod.lagrange_at(x, shift)


@pytest.mark.parametrize("n_pub_out,n_pub_in", [(0, 0), (1, 2)], ids=["no-public", "three-public"])
def test_irregular_circuit_against_python_integers(n_pub_out, n_pub_in):
    """repeated wires (also a pair summing to 0), empty combinations, wires in no matrix, coefficients r - 1: every section of
    the key against the restated generator (Python integers, oracle multiplications)"""
    ug = _ug()
    n_wires, rows, r1cs = SC.odd_circuit(12, n_pub_out, n_pub_in)
    t = SC.trapdoor_dict()
    zkey, vkey, _ = ug.dev_setup(r1cs, t, device=-1)
    n_vars, n_public, domain = SC.zkey_header(zkey)
    assert (n_vars, n_public, domain) == (n_wires, n_pub_out + n_pub_in, 32)
    got = dict(RC.sections(zkey))
    want = SC.python_key_sections(rows, n_wires, n_public, 5, t)
    for sid in sorted(want):
        assert got[sid] == want[sid], "section %d" % sid
    assert got[5][-64 * 3:] == bytes(64 * 3) and got[7][-128 * 3:] == bytes(128 * 3)      # the wires in no matrix: infinity
    assert vkey["nPublic"] == n_public and len(vkey["IC"]) == n_public + 1
    n_records = struct.unpack_from("<I", got[4])[0]
    assert len(got[4]) == 4 + 44 * n_records


@pytest.fixture(scope="module")
def setup_main(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("setup_main")
    return sanitized_build.build(tmp, "setup_main", ["setup_main.cpp", "setup_host.cpp", "host_util.cpp"],
                                 flags=("-O1", "-pthread", "-Wno-unknown-pragmas")), tmp


def test_host_path_runs_clean_under_sanitizers(setup_main):
    """tests/native/setup_main.cpp: the host path alone (no HIP code linked), AddressSanitizer + UBSan, as a child process; it
    reproduces groth16.zkey from the fixture inputs"""
    exe, tmp = setup_main
    _, _, r1cs = RC.trapdoor()
    t = SC.trapdoor_dict()
    (tmp / "circuit.r1cs").write_bytes(r1cs)
    (tmp / "trapdoor.bin").write_bytes(b"".join(int(t[k]).to_bytes(32, "little") for k in ("tau", "alpha", "beta", "gamma", "delta_round", "delta_final")))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp / "circuit.r1cs"), str(tmp / "trapdoor.bin"), os.path.join(ROOT, "tests", "golden", "trapdoor", "groth16.zkey"), "10"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "setup_main ok", (r.stdout[-500:], r.stderr[-3000:])


def test_cli_says_test_key_and_writes_the_fixture(tmp_path):
    """dev_setup <r1cs> <zkey> <vkey> --trapdoor t.json --log-domain 10 on host threads; without --trapdoor one is written beside the key"""
    _, _, r1cs = RC.trapdoor()
    (tmp_path / "c.r1cs").write_bytes(r1cs)
    env = dict(os.environ, ULTRAGROTH_DEVICE="-1")
    exe = os.path.join(CSRC, "dev_setup")
    td = os.path.join(ROOT, "tests", "golden", "trapdoor", "trapdoor.json")
    r = subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "k.zkey"), str(tmp_path / "vk.json"), "--trapdoor", td, "--log-domain", "10"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "TEST key" in r.stderr
    assert (tmp_path / "k.zkey").read_bytes() == RC.golden("groth16.zkey")
    assert json.loads((tmp_path / "vk.json").read_text()) == json.loads(RC.golden("groth16_vkey.json"))
    (tmp_path / "u.json").write_text(json.dumps(SC.ultra_spec()))
    r = subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "u.zkey"), str(tmp_path / "uvk.json"), "--trapdoor", td, "--log-domain", "10",
                        "--ultra", str(tmp_path / "u.json")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "TEST key" in r.stderr, r.stderr
    assert (tmp_path / "u.zkey").read_bytes() == RC.golden("ultra.zkey")
    r = subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "d.zkey"), str(tmp_path / "dvk.json")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "TEST key" in r.stderr, r.stderr
    drawn = json.loads((tmp_path / "d.zkey.trapdoor.json").read_text())
    assert _ug().dev_setup(r1cs, drawn, device=-1)[0] == (tmp_path / "d.zkey").read_bytes()
    r = subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "e.zkey"), str(tmp_path / "evk.json"), "--log-domain", "3"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1 and "TEST key" in r.stderr and "Error: setup: log_domain 3 is too small" in r.stderr
    r = subprocess.run([exe, str(tmp_path / "c.r1cs"), str(tmp_path / "f.zkey"), str(tmp_path / "fvk.json"), "--log-domain", "ten"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1 and "--log-domain takes a number" in r.stderr and not (tmp_path / "f.zkey").exists()
