"""The registry's batched call and witness check (include/prover.h: ug_registry_prove_batch, ug_registry_attach_r1cs*,
ug_registry_batch_info) and the batched pass of an attached created UltraGroth prover.

A batch must be the single proofs under the same blinding sequence, byte for byte, from the registry and from the created prover;
ug_*_batch_info shows that device passes were shared (passes < witnesses)."""
import hashlib
import os

import pytest

import r1cs_cases as K
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LOG = 13
COUNT = 17                               # above UG_BATCH_MAX: a call of 17 is two passes
TD = os.path.join(GOLDEN, "trapdoor")
_CIRCUITS = {}


def _blind(ultra, b):
    return tuple(hashlib.sha256(b"%s%d" % (t, b)).digest()[:31] for t in ((b"rk", b"r", b"s") if ultra else (b"r", b"s")))


def _with_blinding(ultra, first, count, fn):
    import ultragroth_amd as ug
    ug.set_test_blinding(b"".join(b"".join(_blind(ultra, first + i)) for i in range(count)))
    try:
        return fn()
    finally:
        ug.set_test_blinding(b"")


def _circuit(device, ultra):
    from ultragroth_amd import synth
    if ultra not in _CIRCUITS:
        if ultra:
            zkey = synth.build_ultra_circuit(device, LOG)[0]
            wtns = synth.build_ultra_witnesses(LOG, COUNT)
        else:
            zkey = synth.build_circuit(device, LOG, mix="U")[0]
            wtns = [synth.build_witness(LOG, "UC"[b % 2], seed=0x7000 + 16 * b) for b in range(COUNT)]
        _CIRCUITS[ultra] = (bytes(zkey), wtns)
    return _CIRCUITS[ultra]


@pytest.mark.parametrize("ultra", [False, True], ids=["groth16", "ultragroth"])
def test_registry_batch_equals_singles_and_the_created_prover(device, ultra):
    import ultragroth_amd as ug
    zkey, wtns = _circuit(device, ultra)
    with (ug.UltraGrothProver if ultra else ug.Groth16Prover)(zkey) as p:
        created = _with_blinding(ultra, 0, COUNT, lambda: p.prove_batch(wtns))
    with ug.Registry(0) as reg:
        reg.load("c", zkey)
        singles = [_with_blinding(ultra, b, 1, lambda: reg.prove("c", w)) for b, w in enumerate(wtns)]
        assert singles == created
        assert reg.batch_info("c") == (0, 0, 0)
        proofs = COUNT
        for k in (5, 3, 16, 17):
            passes0, witnesses0, _ = reg.batch_info("c")
            assert _with_blinding(ultra, 0, k, lambda: reg.prove_batch("c", wtns[:k])) == singles[:k], k
            passes, witnesses, width = reg.batch_info("c")
            assert witnesses - witnesses0 == k and passes - passes0 < k, (k, passes - passes0)
            assert 1 <= width <= min(k, ug.BATCH_MAX)            # (what ug_plan_proof_batch grants: window sets bound it at this size)
            proofs += k
            assert reg.info("c")[2] == proofs and reg.info()[2] == proofs
        assert reg.prove_batch("c", []) == []
        with pytest.raises(ug.ProverError, match="circuit not loaded: nope"):
            reg.prove_batch("nope", wtns[:2])
        with pytest.raises(ug.ProverError) as e:
            reg.prove_batch("c", wtns[:3], proof_size=100)
        assert e.value.code == ug.PROVER_ERROR_SHORT_BUFFER and all(sz >= (1400 if ultra else 810) for sz in e.value.proof_sizes)
        bad = list(wtns[:4])
        bad[2] = wtns[2][:len(wtns[2]) // 2]      # cut short: the single prove's code and message
        with pytest.raises(ug.ProverError) as single:
            reg.prove("c", bad[2])
        with pytest.raises(ug.ProverError) as e:
            reg.prove_batch("c", bad)
        assert e.value.code == single.value.code and e.value.message == "witness 2: " + single.value.message
        assert _with_blinding(ultra, 0, 2, lambda: reg.prove_batch("c", wtns[:2])) == singles[:2]


def _least_free_bytes(schedules, n_vars, domain, width):
    """the fewest free bytes for which ug_plan_proof_batch grants `width` witnesses of 16 asked for"""
    import ultragroth_amd as ug
    lo, hi = 0, 1 << 40
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if ug.plan_proof_batch(schedules, n_vars, domain, mid, 16) >= width:
            hi = mid
        else:
            lo = mid
    return hi


def test_registry_batch_under_a_budget(device, monkeypatch):
    """A budget whose room admits only a narrower pass than the card's: the same bytes, the budget kept; the batch buffers are
    work bytes, which the next circuit's load takes back. The budget comes from the planner's own memory model: the circuit, and
    room halfway between what a pass of two and the unconstrained pass need."""
    import ultragroth_amd as ug
    monkeypatch.setenv("ULTRAGROTH_TABLES", "0")                 # cores and workspaces alone, classic windows
    zkey, wtns = _circuit(device, False)
    k = 16
    n_vars, domain = (1 << LOG) - 1, 1 << LOG
    schedules = [(n_vars, 0, 1), (domain, 0, 1)]                 # the witness group and H
    with ug.Registry(0) as reg:
        reg.load("c", zkey)
        core = reg.info()[0]
        expected = _with_blinding(False, 0, k, lambda: reg.prove_batch("c", wtns[:k]))
        passes0, _, width0 = reg.batch_info("c")
        total = reg.info()[0]
    assert width0 == ug.plan_proof_batch(schedules, n_vars, domain, 1 << 40, k) > 2
    room = (_least_free_bytes(schedules, n_vars, domain, 2) + _least_free_bytes(schedules, n_vars, domain, width0)) // 2
    budget = core + room
    print("bytes: core %d, after passes of %d: %d; room %d" % (core, width0, total, room))
    with ug.Registry(0, budget) as reg:
        reg.load("c", zkey)
        assert reg.info("c")[0] == core
        assert _with_blinding(False, 0, k, lambda: reg.prove_batch("c", wtns[:k])) == expected
        passes, witnesses, width = reg.batch_info("c")
        held = reg.info("c")[0]
        print("budget %d: %d passes, last width %d, bytes %d" % (budget, passes, width, reg.info()[0]))
        assert witnesses == k and passes0 < passes < k and 1 <= width < width0
        assert reg.info()[0] <= budget
        assert held > core
        # more circuits of the same size, until they no longer fit beside the first one's workspaces: those go, batch buffers included
        names = ["d%d" % i for i in range((budget - reg.info()[0]) // core + 1)]
        assert (len(names) + 1) * core <= budget                  # (the cores alone fit: nobody is evicted as a whole)
        for name in names:
            reg.load(name, zkey)
            assert reg.info()[0] <= budget
        assert reg.info("c")[0] == core < held
        assert _with_blinding(False, 0, 3, lambda: reg.prove_batch(names[-1], wtns[:3])) == expected[:3]


FAIL_1 = "witness: constraint 1 does not hold (2 of 430 fail)"      # inv1_0 changed: its own inverse constraint and the lookup identity


def _twin_witnesses(k):
    """k witnesses of the trapdoor circuit's Groth16 twin, one per challenge value, and witness 0 with inv1_0 changed"""
    mod = K.trapdoor_module()
    w1, chunks, freq = mod.first_round_witness()
    good = [mod.complete_witness(w1, chunks, freq, mod.det("registry batch challenge %d" % b)) for b in range(k)]
    bad = list(good[0])
    bad[mod.INV1] = (bad[mod.INV1] + 1) % K.R
    return [K.wtns_file(w) for w in good], K.wtns_file(bad)


def _changed(rows, k, side, fn):
    rows = [tuple(dict(lc) for lc in row) for row in rows]
    fn(rows[k][side])
    return rows


@pytest.mark.parametrize("form", ["buffer", "file"])
def test_registry_attach(device, tmp_path, form):
    import ultragroth_amd as ug
    mod, rows, data = K.trapdoor()
    good, bad = _twin_witnesses(5)
    zkey_path = str(tmp_path / "twin.zkey")
    with open(zkey_path, "wb") as f:
        f.write(K.golden("groth16.zkey"))
    r1cs_path = str(tmp_path / "twin.r1cs")
    with open(r1cs_path, "wb") as f:
        f.write(data)
    attachment = data if form == "buffer" else r1cs_path

    def batch(reg, wtns):
        return _with_blinding(False, 0, len(wtns), lambda: reg.prove_batch("twin", wtns))

    with ug.Registry(0) as reg:
        reg.load_file(zkey_path)
        expected = batch(reg, good)
        assert batch(reg, [bad]) != expected[:1]                     # unattached, a bad witness proves
        unattached = reg.info("twin")[0]
        # a wrong .r1cs is refused and nothing is attached
        twin = K.trapdoor_r1cs(_changed(rows, 5, 0, lambda lc: lc.update({mod.RHO: 2})))
        with pytest.raises(ug.ProverError) as e:
            reg.attach_r1cs("twin", twin)
        assert e.value.message == "r1cs: not this circuit: matrix A row 5 differs from the zkey"
        batch(reg, [bad])
        with pytest.raises(ug.ProverError, match="circuit not loaded: nope"):
            reg.attach_r1cs("nope", data)
        reg.attach_r1cs("twin", attachment)
        print("resident bytes: %d unattached, %d attached" % (unattached, reg.info("twin")[0]))
        assert reg.info("twin")[0] >= unattached                     # (the matrices count as resident bytes: a few KB here, below the allocator's grain)
        # good batches prove, the same bytes; a bad witness at position b fails the call with its name and writes nothing
        assert batch(reg, good) == expected
        for b in (0, 3, 4):
            with pytest.raises(ug.ProverError) as e:
                batch(reg, good[:b] + [bad] + good[b + 1:])
            assert e.value.message == "witness %d: " % b + FAIL_1 and e.value.code == ug.PROVER_ERROR
        with pytest.raises(ug.ProverError) as e:
            reg.prove("twin", bad)
        assert e.value.message == FAIL_1
        assert batch(reg, good) == expected                          # the next call works
        passes, witnesses, _ = reg.batch_info("twin")
        assert passes < witnesses
        # evicted whole by a budget, reloaded from its file: the bad witness is still refused
    # evicted whole under a budget, reloaded from its file: the bad witness is still refused. The budget holds three and a half of
    # the larger synthetic circuits; they are loaded, then proven, until the least recently used circuit -- `twin` -- has to go.
    big, big_wtns = _circuit(device, False)
    others = []
    for i in range(6):
        others.append(str(tmp_path / ("other%d.zkey" % i)))
        with open(others[-1], "wb") as f:
            f.write(big)
    with ug.Registry(0) as reg:
        reg.load_file(others[0])
        core = reg.info()[0]

    def crowd_out(reg, use):
        for path in others:
            use(path)
            if reg.info("twin")[1] == ug.Registry.EVICTED:
                return
        raise AssertionError("six circuits of %d bytes fit a budget of three and a half" % core)

    with ug.Registry(0, core * 7 // 2) as reg:
        reg.load_file(zkey_path)
        reg.attach_r1cs("twin", attachment)
        crowd_out(reg, reg.load_file)
        with pytest.raises(ug.ProverError) as e:
            batch(reg, good[:2] + [bad])
        assert e.value.message == "witness 2: " + FAIL_1
        assert reg.info("twin")[1] != ug.Registry.EVICTED
        assert batch(reg, good) == expected
        if form == "file":                                           # evicted again, its .r1cs gone: the proof call fails, nothing is proven unchecked
            crowd_out(reg, lambda path: reg.prove(os.path.basename(path)[:-5], big_wtns[0]))
            os.rename(r1cs_path, r1cs_path + ".away")
            with pytest.raises(ug.ProverError, match="r1cs: cannot read"):
                batch(reg, [bad])
            with pytest.raises(ug.ProverError, match="r1cs: cannot read"):
                reg.prove("twin", bad)
            os.rename(r1cs_path + ".away", r1cs_path)
            with pytest.raises(ug.ProverError) as e:
                batch(reg, [bad])
            assert e.value.message == "witness 0: " + FAIL_1
        # detached, the bad witness proves again; loading a zkey under the name drops an attachment too
        reg.attach_r1cs("twin", None)
        batch(reg, [bad])
        reg.attach_r1cs("twin", attachment)
        reg.load_file(zkey_path)
        batch(reg, [bad])


def test_registry_refuses_the_environment_r1cs(device, tmp_path, monkeypatch):
    import ultragroth_amd as ug
    monkeypatch.setenv("ULTRAGROTH_R1CS", str(tmp_path / "any.r1cs"))
    with ug.Registry(0) as reg:
        with pytest.raises(ug.ProverError) as e:
            reg.load("twin", K.golden("groth16.zkey"))
        assert e.value.message == "witness check: not available on this kind of prover"


def test_created_ultragroth_prover_attached_keeps_its_batched_pass(device):
    import ultragroth_amd as ug
    mod, rows, data = K.trapdoor()
    zkey, uwtns = K.golden("ultra.zkey"), K.golden("ultra.uwtns")
    values = K.wtns_values(uwtns)
    values[mod.C0] += 1                                              # constraint 1 breaks, and only it (test_gpu_r1cs_check.py)
    bad = K.binfile(b"wtns", 2, [(i, b"".join(v.to_bytes(32, "little") for v in values) if i == 2 else s) for i, s in K.sections(uwtns)])
    four = [uwtns] * 4
    with ug.UltraGrothProver(zkey) as p:
        unattached = _with_blinding(True, 0, 4, lambda: p.prove_batch(four))
        singles = [_with_blinding(True, b, 1, lambda: p.prove(uwtns)) for b in range(4)]
        assert unattached == singles
        shared, witnesses, width = p.batch_info()
        assert witnesses == 4 and shared < 4 and width > 1           # (the width is the planner's: window sets bound it at this size)
        p.attach_r1cs(data)
        assert _with_blinding(True, 0, 4, lambda: p.prove_batch(four)) == unattached
        passes, witnesses, width = p.batch_info()
        assert witnesses == 8 and passes < witnesses and passes == 2 * shared      # (the parent: one pass per witness while attached)
        with pytest.raises(ug.ProverError) as e:
            p.prove_batch([uwtns, uwtns, bad, uwtns])
        assert e.value.message == "witness 2: witness: constraint 1 does not hold (1 of 430 fail)"
        with pytest.raises(ug.ProverError) as e:
            p.prove_batch([bad, uwtns, bad])
        assert e.value.message == "witness 0: witness: constraint 1 does not hold (1 of 430 fail)"
        assert _with_blinding(True, 0, 4, lambda: p.prove_batch(four)) == unattached
    with ug.Registry(0) as reg:                                      # the same through the registry
        reg.load("ultra", zkey)
        reg.attach_r1cs("ultra", data)
        assert _with_blinding(True, 0, 4, lambda: reg.prove_batch("ultra", four)) == unattached
        assert reg.batch_info("ultra") == (shared, 4, width)
        with pytest.raises(ug.ProverError) as e:
            reg.prove_batch("ultra", [uwtns, bad])
        assert e.value.message == "witness 1: witness: constraint 1 does not hold (1 of 430 fail)"
