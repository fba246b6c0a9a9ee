"""The transform of csrc/ntt.hip (ntt_pass_kernel) through ug_fr_ntt and the H-polynomial block, against the CPU oracle and against
the closed forms of tests/ntt_cases.py (checked on the host by test_ntt_cases.py), bit for bit:

  every pass geometry     2^0 .. 2^21: one pass up to 2^10, 10 + k with every k = 1 .. 8 (odd k: a radix-2 step first), 10 + 5 + 4,
                          10 + 5 + 5 and 10 + 6 + 5 (a middle pass that is neither first nor last)
  structured inputs       vectors whose intermediate values are almost all zero residues -- carried as q, 2q, 3q by the lazily
                          reduced butterflies -- and their unreduced twins
  both twiddle forms      UG_NTT_SHOUP=0 (Montgomery twiddles, KQ = 2) in a process of its own
  the H-polynomial block  at three-pass sizes against the oracle and against the closed form of a two-record matrix

Expected values come from the oracle or from Python integers; the round trip is an extra check beside them."""
import hashlib
import os
import subprocess
import sys

import pytest

import ntt_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURED = [1, 3, 4, 9, 10, 11, 13, 15, 16, 18, 19, 20]
FULL_PRODUCT_FORM = 19               # the geometric family is checked at every place up to this size, at sample_places above


@pytest.fixture(scope="module", autouse=True)
def _tables():
    yield
    NC.forget_tables()


@pytest.mark.parametrize("logn", range(22))
def test_every_geometry(device, logn):
    data, reduced = NC.spliced_random(logn)
    fwd = device.ntt(data, logn)
    assert fwd == O.ntt(reduced, logn)
    assert device.ntt(data, logn, inverse=True) == O.ntt(reduced, logn, inverse=True)
    assert device.ntt(fwd, logn, inverse=True) == reduced                        # round trip


_C_IDS = {0: "", 1: "-1", NC.R - 1: "-r-1", NC.MONT: "-R"}
_EXPLICIT = [(case.name.split("(")[0], case.c) for case in NC.all_cases(1) if case.expected(False) is not None]
_EXPLICIT = list(dict.fromkeys(_EXPLICIT))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("name,c", _EXPLICIT, ids=[name + _C_IDS[c] for name, c in _EXPLICIT])
@pytest.mark.parametrize("logn", STRUCTURED)
def test_structured_inputs(device, logn, name, c, inverse):
    """every family with an explicit expected vector, one value of c per case: zero | constant | delta at 0, 1, n / 2, n - 1 and the
    borders of the first tile | single frequencies | alternating | all r - 1; the twin takes the same bytes"""
    cases = NC.family(logn, name, only_c=c)
    assert cases
    for t, case in enumerate(cases):
        data, exp = case.data, case.expected(inverse)
        assert device.ntt(data, logn, inverse=inverse) == exp, case
        assert device.ntt(NC.twin(data, shift=t), logn, inverse=inverse) == exp, (case, "twin")
    NC.forget_tables(keep_logn=logn)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("c", range(3), ids=["1", "r-1", "R"])
@pytest.mark.parametrize("logn", STRUCTURED)
def test_geometric_inputs(device, logn, c, inverse):
    """X_k (g omega^k - 1) == c (g^n - 1) with X_k canonical pins every output down; the twin must give the same bytes"""
    case, = NC.family(logn, "geometric", only_c=NC.C_VALUES[c])
    data = case.data
    out = device.ntt(data, logn, inverse=inverse)
    assert case.holds(out, inverse, places=None if logn <= FULL_PRODUCT_FORM else NC.sample_places(logn))
    if logn > FULL_PRODUCT_FORM:
        assert out == O.ntt(data, logn, inverse=inverse)
    assert device.ntt(NC.twin(data, shift=c), logn, inverse=inverse) == out


# ---- Montgomery twiddles ----------------------------------------------------------------------------------------------------------
CHILD_SIZES = [3, 10, 11, 16, 19]
_CHILD = """
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import ultragroth_amd as ug
import ntt_cases as NC
assert os.environ.get("UG_NTT_SHOUP") == "0"
d = ug.Device(0)
sha = lambda b: hashlib.sha256(b).hexdigest()
for logn in [int(x) for x in sys.argv[3].split(",")]:
    inputs = [("random", NC.spliced_random(logn)[0])] + [(c.name, c) for c in NC.all_cases(logn)]
    for name, src in inputs:
        data = src if isinstance(src, bytes) else src.data
        for inverse in (False, True):
            print("result", "ntt|%d|%d|%s" % (logn, inverse, name), sha(d.ntt(data, logn, inverse=inverse)), sep="\t")
    NC.forget_tables()
for name in sys.argv[4:]:
    coefs, w = open(os.path.join(sys.argv[2], name + ".coefs"), "rb").read(), open(os.path.join(sys.argv[2], name + ".wtns"), "rb").read()
    domain, nvars = [int(x) for x in open(os.path.join(sys.argv[2], name + ".shape")).read().split()]
    hp = d.hpoly(coefs, len(coefs) // 44, domain, nvars)
    print("result", "hpoly|" + name, sha(d.download(hp.run(d.dvec(nvars, w)), 0, domain)), sep="\t")
d.close()
"""


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_montgomery_twiddles(zkey, wtns, tmp_path):
    """UG_NTT_SHOUP=0 selects ntt_pass_kernel<false, ..> (48-byte Montgomery twiddles, products below 2q). The library reads the knob
    when a plan is made, so the whole list runs in ONE fresh process: the spliced random vector and every structured case at five
    sizes (one pass, two passes with k = 1 and k = 6, three passes), both directions, then the H-polynomial block of the fixture
    circuit and of two two-record matrices at 2^11. The child prints one sha256 per result; the expected hashes are the
    oracle's and the closed forms'. (The launch statistics of a context do not tell the two kernels apart, and ug_fr_ntt is not
    counted in them; a kernel trace of this child names ntt_pass_kernel<false, false> and no other instantiation.)"""
    expected = {}
    for logn in CHILD_SIZES:
        reduced = NC.spliced_random(logn)[1]
        cases = NC.all_cases(logn)
        for inverse in (False, True):
            expected["ntt|%d|%d|random" % (logn, inverse)] = _sha(O.ntt(reduced, logn, inverse=inverse))
            for case in cases:
                exp = case.expected(inverse)
                expected["ntt|%d|%d|%s" % (logn, inverse, case.name)] = _sha(exp if exp is not None else O.ntt(case.data, logn, inverse=inverse))
        NC.forget_tables()
    info = O.zkey_info(zkey)
    off, sz = O.section(zkey, "zkey", 4)
    woff, wsz = O.section(wtns, "wtns", 2)
    blocks = {"fixture": (zkey[off + 4:off + sz], wtns[woff:woff + wsz], info["domainSize"], info["nVars"], None)}
    for ra, rb in ((5, 5), (0, 2047)):
        coefs, _, w, nvars, exp = NC.hpoly_case(11, ra, rb)
        blocks["two_records_%d_%d" % (ra, rb)] = (coefs, w, 1 << 11, nvars, exp)
    for name, (coefs, w, domain, nvars, exp) in blocks.items():
        (tmp_path / (name + ".coefs")).write_bytes(coefs)
        (tmp_path / (name + ".wtns")).write_bytes(w)
        (tmp_path / (name + ".shape")).write_text("%d %d" % (domain, nvars))
        oracle = O.hpoly(coefs, len(coefs) // 44, w, nvars, domain)
        assert exp is None or exp == oracle
        expected["hpoly|" + name] = _sha(oracle)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path), ",".join(str(x) for x in CHILD_SIZES)] + list(blocks),
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, UG_NTT_SHOUP="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(ln.split("\t")[1:] for ln in r.stdout.splitlines() if ln.startswith("result\t"))
    assert set(got) == set(expected) and len(expected) == 2 * sum(1 + len(NC.all_cases(logn)) for logn in CHILD_SIZES) + 3
    assert [k for k in expected if got[k] != expected[k]] == []


# ---- the H-polynomial block at three-pass sizes ---------------------------------------------------------------------------------
NVARS = 5003


def _matrix(logn, nvars):
    """44-byte records of sparse A and B on about a quarter of the rows: the row pattern of test_gpu_hpoly_vectors.py -- empty rows,
    rows of 1, 4, 5 and 30 records (30 > 24: the contraction path), signals repeated within a row and across rows -- on 8 rows
    of every 256, one record on every fourth of the others; shuffled"""
    import numpy as np
    domain = 1 << logn
    counts = np.array([0, 1, 4, 5, 30, 2, 0, 9], dtype=np.int64)
    rows = np.arange(2 * domain, dtype=np.int64)
    m, c = rows // domain, rows % domain
    n = np.where(c % 256 < 8, counts[(c * 7 + m * 3 + 4) % 8], np.where(c % 4 == 1, 1, 0))
    n[[0, domain - 1, domain, 2 * domain - 1]] = (5, 30, 4, 1)          # the first and the last row of either matrix hold records
    total = int(n.sum())
    row_of = np.repeat(rows, n)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    rec = np.zeros(total, dtype=[("m", "<u4"), ("c", "<u4"), ("s", "<u4"), ("v", "V32")])
    rec["m"], rec["c"] = row_of // domain, row_of % domain
    rec["s"] = (row_of * 5 + (k % 7) * 3) % nvars
    vals = np.array([O.to_le((x * x * 0x9E3779B97F4A7C15 + 1) * pow(2, 512, O.R_MOD) % O.R_MOD) for x in range(1, 18)] +
                    [O.to_le((O.R_MOD - 1) * pow(2, 512, O.R_MOD) % O.R_MOD)], dtype="V32")
    rec["v"] = vals[(row_of + 3 * k) % len(vals)]
    np.random.Generator(np.random.PCG64(0xC0EF + logn)).shuffle(rec)
    return rec.tobytes(), total


@pytest.mark.parametrize("logn", [19, 20])
def test_hpoly_three_passes_matches_oracle(device, logn):
    """10 + 5 + 4 and 10 + 5 + 5: the scattering last pass (by_place at s0 = 15), the twist table in bit-reversed order, in2,
    fin_a / fin_b and the work buffers over three passes; a witness with values >= r (2^256 - 1 among them)"""
    from test_gpu_hpoly_vectors import _witness
    domain = 1 << logn
    coefs, ncoefs = _matrix(logn, NVARS)
    assert domain // 5 < ncoefs and 44 * ncoefs < 64 << 20
    w = _witness(1, NVARS)
    hp = device.hpoly(coefs, ncoefs, domain, NVARS)
    h = device.download(hp.run(device.dvec(NVARS, w)), 0, domain)
    if logn == 19:
        h_exp, abc = O.hpoly(coefs, ncoefs, w, NVARS, domain, want_abc=True)
        assert h == h_exp
        a, b, c = hp.debug_abc()
        n = 32 * domain
        assert a == abc[:n] and b == abc[n:2 * n] and c == abc[2 * n:]
    else:
        assert h == O.hpoly(coefs, ncoefs, w, NVARS, domain)
    assert h != bytes(32 * domain)


@pytest.mark.parametrize("rows", ["first_first", "last_middle", "middle_middle", "first_last", "last_last"])
@pytest.mark.parametrize("logn", [11, 19])
def test_hpoly_two_records_closed_form(device, logn, rows):
    n = 1 << logn
    place = {"first": 0, "middle": n // 2 + 5, "last": n - 1}
    ra, rb = (place[x] for x in rows.split("_"))
    coefs, ncoefs, w, nvars, exp = NC.hpoly_case(logn, ra, rb)
    hp = device.hpoly(coefs, ncoefs, n, nvars)
    assert device.download(hp.run(device.dvec(nvars, w)), 0, n) == exp
