"""ultragroth_amd -- MI355X-native drop-in for the prover hot path of rarimo/ultragroth.

Host-side mirror (Python) of the C interfaces in ``include/``:

* :class:`Groth16Prover`, :class:`UltraGrothProver`, :func:`groth16_prover` ... mirror the reference's
  ``extern "C"`` prover API (src/prover.h) -- same names, argument meaning and error behaviour,
  with the status codes raised as :class:`ProverError` carrying ``code`` and the reference's message.
* :class:`Device` exposes the inner ABI (``include/ultragroth_hip.h``): MSM, NTT, H polynomial and
  field ops, in the reference's byte formats.

All compute goes through ``libultragroth_hip.so`` (hand-written HIP for gfx950). There is no CPU
fallback: without the library or without a GPU every call raises.
"""
import ctypes as C

from . import _lib
from ._lib import build, load, LIB_PATH

PROVER_OK = 0
PROVER_ERROR = 1
PROVER_ERROR_SHORT_BUFFER = 2
PROVER_INVALID_WITNESS_LENGTH = 3

FR, FQ = 0, 1
OP_MUL, OP_ADD, OP_SUB, OP_SQR = 0, 1, 2, 3
GROTH16_PARTIALS_SIZE = 384


class ProverError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code
        self.message = message


class DeviceError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise DeviceError(load().ug_last_error().decode(errors="replace"))


def device_count():
    return load().ug_device_count()


def set_test_blinding(data):
    """Queue bytes for the prover's blinding draws (31 bytes each); b'' restores OS entropy."""
    data = bytes(data)
    if load().ug_test_set_blinding(data if data else None, len(data)) != PROVER_OK:
        raise ProverError(PROVER_ERROR, "test hooks are off: start the process with ULTRAGROTH_TEST_HOOKS=1")


FAULT_HPOLY_RUN, FAULT_SCHEDULE_BUILD, FAULT_HPOLY_RESERVE = 1, 2, 3


def inject_fault(site, after=1):
    """ug_test_inject_fault: the `after`-th next pass through fault point `site` fails (test processes only)"""
    if load().ug_test_inject_fault(site, after) != 0:
        raise ProverError(PROVER_ERROR, "test hooks are off: start the process with ULTRAGROTH_TEST_HOOKS=1")


def _buf(b):
    return (C.c_char * len(b)).from_buffer_copy(b) if not isinstance(b, C.Array) else b


# ---------------------------------------------------------------------------------------------------
# outer API mirror (src/prover.h)

def groth16_proof_size():
    v = C.c_ulonglong()
    load().groth16_proof_size(C.byref(v))
    return v.value


def ultra_groth_proof_size():
    v = C.c_ulonglong()
    load().ultra_groth_proof_size(C.byref(v))
    return v.value


def _public_size(fn, zkey):
    v = C.c_ulonglong()
    err = C.create_string_buffer(1024)
    rc = fn(zkey, len(zkey), C.byref(v), err, len(err) - 1)
    if rc != PROVER_OK:
        raise ProverError(rc, err.value.decode(errors="replace"))
    return v.value


def groth16_public_size_for_zkey_buf(zkey):
    return _public_size(load().groth16_public_size_for_zkey_buf, zkey)


def ultra_groth_public_size_for_zkey_buf(zkey):
    return _public_size(load().ultra_groth_public_size_for_zkey_buf, zkey)


# ---------------------------------------------------------------------------------------------------
# zkey validation (include/prover.h: ug_zkey_check; include/ultragroth_hip.h: ug_points_check)
UG_POINT_OK, UG_POINT_UNREDUCED, UG_POINT_OFF_CURVE, UG_POINT_OFF_SUBGROUP = 0, 1, 2, 3


class _PointFault(C.Structure):
    _fields_ = [("index", C.c_uint64), ("reason", C.c_int)]


class _ZkeyFault(C.Structure):
    _fields_ = [("section", C.c_int), ("index", C.c_ulonglong), ("reason", C.c_int)]


def zkey_check(zkey, level=2, device=0):
    """ug_zkey_check: None for a key whose every point passes, else (section, index, reason, message) -- section 2 is the header,
    reason one of UG_POINT_*. A key that cannot be parsed raises ProverError with the loaders' message."""
    fault = _ZkeyFault()
    err = C.create_string_buffer(1024)
    rc = load().ug_zkey_check(zkey, len(zkey), device, level, C.byref(fault), err, len(err) - 1)
    if rc == PROVER_OK:
        return None
    msg = err.value.decode(errors="replace")
    if fault.reason == UG_POINT_OK:
        raise ProverError(rc, msg)
    return fault.section, fault.index, fault.reason, msg


# ---------------------------------------------------------------------------------------------------
# witness check against the circuit's .r1cs (include/prover.h: ug_witness_check; include/ultragroth_hip.h: ug_r1cs_*)
class _WitnessFault(C.Structure):
    _fields_ = [("failed", C.c_ulonglong), ("first", C.c_ulonglong), ("a", C.c_ubyte * 32), ("b", C.c_ubyte * 32), ("c", C.c_ubyte * 32)]


class _R1csInfo(C.Structure):
    _fields_ = [("n_wires", C.c_uint32), ("n_pub_out", C.c_uint32), ("n_pub_in", C.c_uint32), ("n_prv_in", C.c_uint32),
                ("n_constraints", C.c_uint32), ("n_labels", C.c_uint64), ("terms", C.c_uint64 * 3)]

    def as_dict(self):
        return {"n_wires": self.n_wires, "n_pub_out": self.n_pub_out, "n_pub_in": self.n_pub_in, "n_prv_in": self.n_prv_in,
                "n_constraints": self.n_constraints, "n_labels": self.n_labels, "terms": tuple(self.terms)}


class _R1csReport(C.Structure):
    _fields_ = [("failed", C.c_uint64), ("first", C.c_uint64), ("a", C.c_ubyte * 32), ("b", C.c_ubyte * 32), ("c", C.c_ubyte * 32),
                ("device_ms", C.c_double)]


def _le(arr):
    return int.from_bytes(bytes(arr), "little")


def witness_check(r1cs, wtns, device=0):
    """ug_witness_check: None for a witness that satisfies every constraint of the .r1cs, else (failed, first, a, b, c, message) --
    the count of failing constraints, the lowest of them and its values A.w, B.w, C.w as integers mod r. device=-1 runs the check
    on host threads (no GPU). A file that does not parse raises ProverError with the loaders' message."""
    fault = _WitnessFault()
    err = C.create_string_buffer(1024)
    rc = load().ug_witness_check(r1cs, len(r1cs), wtns, len(wtns), device, C.byref(fault), err, len(err) - 1)
    if rc == PROVER_OK:
        return None
    msg = err.value.decode(errors="replace")
    if fault.failed == 0:
        raise ProverError(rc, msg)
    return fault.failed, fault.first, _le(fault.a), _le(fault.b), _le(fault.c), msg


def r1cs_info(r1cs):
    """ug_r1cs_parse_info (host only): the header fields and the term counts of A, B, C as a dict; DeviceError for a file that
    breaks a rule of the layout"""
    info = _R1csInfo()
    _check(load().ug_r1cs_parse_info(r1cs, len(r1cs), C.byref(info)))
    return info.as_dict()


# ---------------------------------------------------------------------------------------------------
# development setup (include/ultragroth_hip.h: ug_setup_*): a TEST key from an .r1cs and a known trapdoor
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TRAPDOOR_KEYS = ("tau", "alpha", "beta", "gamma", "delta_round", "delta_final")
SETUP_PHASES = ("parse", "lagrange", "products", "g1", "g2", "assembly")


class SetupError(RuntimeError):
    pass


class _SetupOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("protocol", C.c_uint32), ("log_domain", C.c_uint32), ("rand_indx", C.c_uint32)] + \
               [(k, C.c_ubyte * 32) for k in TRAPDOOR_KEYS] + \
               [("round_signals", C.POINTER(C.c_uint32)), ("n_round", C.c_uint64),
                ("final_signals", C.POINTER(C.c_uint32)), ("n_final", C.c_uint64)]


def _setup_call(fn, *args):
    err = C.create_string_buffer(1024)
    if fn(*args, err, len(err) - 1) != 0:
        raise SetupError(err.value.decode(errors="replace"))


def _le32(value, what):
    value = int(value)
    if not 0 <= value < 1 << 256:
        raise SetupError("setup: %s is not below the field modulus" % what)
    return (C.c_ubyte * 32)(*value.to_bytes(32, "little"))


def _setup_options(trapdoor, protocol, log_domain, ultra):
    """(options struct, the arrays it points into) of dev_setup's arguments; trapdoor None: drawn from OS entropy"""
    opt = _SetupOptions()
    opt.size = C.sizeof(_SetupOptions)
    if protocol in ("groth16", 1):
        opt.protocol = 1
    elif protocol in ("ultragroth", 1337):
        opt.protocol = 1337
    else:
        raise SetupError("setup: protocol %r is neither groth16 nor ultragroth" % (protocol,))
    opt.log_domain = log_domain
    if trapdoor is None:
        _setup_call(load().ug_setup_draw_trapdoor, C.byref(opt))
    else:
        for k in TRAPDOOR_KEYS:
            if k not in trapdoor and not (k == "delta_round" and opt.protocol == 1):
                raise SetupError("setup: the trapdoor has no %s" % k)
            setattr(opt, k, _le32(trapdoor.get(k, 0), k))
    keep = []
    if opt.protocol == 1337:
        if ultra is None:
            raise SetupError("setup: protocol 1337 needs rand_indx and the round and final signal lists")
        opt.rand_indx = int(ultra["rand_indx"])
        for name, count in (("round_signals", "n_round"), ("final_signals", "n_final")):
            arr = (C.c_uint32 * max(1, len(ultra[name])))(*ultra[name])
            keep.append(arr)
            setattr(opt, name, C.cast(arr, C.POINTER(C.c_uint32)))
            setattr(opt, count, len(ultra[name]))
    return opt, keep


def dev_setup(r1cs, trapdoor=None, protocol="groth16", log_domain=0, device=0, ultra=None, timings=None):
    """ug_setup_run: a development setup. Returns (zkey_bytes, vkey_dict, trapdoor_dict) for the circuit of the .r1cs bytes.

    THE RESULT IS A TEST KEY: whoever knows the trapdoor forges proofs for it. It is for benchmarks, integration tests and CI.

    trapdoor: a dict with TRAPDOOR_KEYS (integers or decimal strings, the form of tests/golden/trapdoor/trapdoor.json); None
    draws one from OS entropy. The dict returned holds the values used, as decimal strings. protocol: "groth16" (1) or
    "ultragroth" (1337); the latter takes ultra = {"rand_indx": n, "round_signals": [...], "final_signals": [...]}.
    log_domain 0 is the smallest domain that fits. device=-1 runs on host threads and gives the same bytes.
    timings: a dict that receives the milliseconds of SETUP_PHASES. Refusals raise SetupError ("setup: ..." / "r1cs: ...")."""
    import json
    L = load()
    opt, keep = _setup_options(trapdoor, protocol, log_domain, ultra)
    r1cs = bytes(r1cs)
    zbytes, vmax = C.c_uint64(), C.c_uint64()
    _setup_call(L.ug_setup_size, C.byref(opt), r1cs, len(r1cs), C.byref(zbytes), C.byref(vmax))
    zkey = C.create_string_buffer(zbytes.value)
    vkey = C.create_string_buffer(vmax.value)
    wrote, vlen = C.c_uint64(), C.c_uint64()
    ms = (C.c_double * len(SETUP_PHASES))()
    _setup_call(L.ug_setup_run, C.byref(opt), r1cs, len(r1cs), device, zkey, zbytes.value, C.byref(wrote), vkey, vmax.value, C.byref(vlen), ms)
    if timings is not None:
        timings.update(zip(SETUP_PHASES, ms))
    used = {k: str(_le(getattr(opt, k))) for k in TRAPDOOR_KEYS}
    return zkey.raw[:wrote.value], json.loads(vkey.raw[:vlen.value].decode()), used


def dev_setup_size(r1cs, trapdoor, protocol="groth16", log_domain=0, ultra=None):
    """ug_setup_size (host only): the exact length of the zkey dev_setup returns for these arguments"""
    opt, keep = _setup_options(trapdoor, protocol, log_domain, ultra)
    r1cs = bytes(r1cs)
    zbytes, vmax = C.c_uint64(), C.c_uint64()
    _setup_call(load().ug_setup_size, C.byref(opt), r1cs, len(r1cs), C.byref(zbytes), C.byref(vmax))
    return zbytes.value


def generator_mul(scalars, g2=False, device=0, window=0, timing=None):
    """ug_generator_mul (test tooling): [scalar * G] as zkey-format affine records (64 bytes for G1, 128 for G2; a scalar of 0
    gives the all-zero record) for integers below r. window: the signed-digit window width, 0 = the default. device=-1: host
    threads. timing: a list that receives (table build ms, multiplication ms)."""
    scalars = [int(s) for s in scalars]
    for s in scalars:
        if not 0 <= s < 1 << 256:
            raise SetupError("setup: a scalar is not below the field modulus")
    data = b"".join(s.to_bytes(32, "little") for s in scalars)
    rec = 128 if g2 else 64
    out = C.create_string_buffer(max(1, rec * len(scalars)))
    ms = (C.c_double * 2)()
    _setup_call(load().ug_generator_mul, device, 1 if g2 else 0, data, len(scalars), window, out, ms)
    if timing is not None:
        timing.append((ms[0], ms[1]))
    return [out.raw[rec * i:rec * i + rec] for i in range(len(scalars))]


def lagrange_at(x, log_n, coset=False, device=0):
    """ug_lagrange_at (test tooling): [L_k(x)] (coset: L_k(x / omega_2N)) of the size-2^log_n domain, as integers"""
    n = 1 << log_n if 0 <= log_n < 32 else 0
    out = C.create_string_buffer(max(1, 32 * n))
    _setup_call(load().ug_lagrange_at, device, log_n, int(x).to_bytes(32, "little"), 1 if coset else 0, out)
    return [int.from_bytes(out.raw[32 * k:32 * k + 32], "little") for k in range(n)]


# ---------------------------------------------------------------------------------------------------
# phase-2 setup from a prepared powers-of-tau file (include/ultragroth_hip.h: ug_setup_ptau_*): a Groth16 key from an .r1cs
# and a .ptau, optionally with one delta contribution. No trapdoor is known to this code.
SETUP_PTAU_PHASES = ("parse", "point_check", "g1", "g2", "delta", "assembly")


class _SetupPtauOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_domain", C.c_uint32), ("validate", C.c_uint32), ("contribute", C.c_uint32),
                ("delta", C.c_ubyte * 32)]


class _PtauInfo(C.Structure):
    _fields_ = [("power", C.c_uint32), ("ceremony_power", C.c_uint32), ("prepared", C.c_uint32), ("max_log_domain", C.c_uint32)]


class _Mapped:
    """bytes, a memoryview / mmap, or a path (mapped here, read-only) as (address, length) for a C call that only reads;
    nothing is copied. A context manager: the mapping closes with the block."""

    def __init__(self, src):
        import mmap
        import os
        import numpy as np
        self._close = []
        if isinstance(src, (str, os.PathLike)):
            f = open(src, "rb")
            self._close.append(f)
            if os.fstat(f.fileno()).st_size == 0:
                src = b""
            else:
                src = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                self._close.insert(0, src)
        self._keep = np.frombuffer(src, dtype=np.uint8)
        self.length = int(self._keep.size)
        self.address = C.c_void_p(self._keep.ctypes.data if self.length else 0)

    def close(self):
        self._keep = None                           # (an mmap cannot close while a view of it is alive)
        for c in self._close:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _joined(points, rec):
    """the records joined, every one of `rec` bytes"""
    data = b"".join(points)
    if len(data) != rec * len(points):
        raise SetupError("setup: a point record of another size")
    return data


def ptau_info(ptau):
    """ug_ptau_parse_info (host only): {"power", "ceremony_power", "prepared", "max_log_domain"} of a .ptau given as bytes, a
    memoryview / mmap or a path. The layout is restated in include/ultragroth_hip.h; no file of a real ceremony has been read yet."""
    info = _PtauInfo()
    with _Mapped(ptau) as m:
        _setup_call(load().ug_ptau_parse_info, m.address, m.length, C.byref(info))
    return {"power": info.power, "ceremony_power": info.ceremony_power, "prepared": bool(info.prepared), "max_log_domain": info.max_log_domain}


def setup_from_ptau(r1cs, ptau, delta=None, log_domain=0, device=0, validate=1, timings=None):
    """ug_setup_ptau_run: a Groth16 proving key and verification key from a circuit's .r1cs and a .ptau prepared for phase 2
    (what `snarkjs zkey new` does). Returns (zkey_bytes, vkey_dict, phase_ms_dict).

    ptau: bytes, a memoryview / mmap, or a path that is mapped here; only the slices the circuit's domain needs are read.
    delta: None writes delta = 1 -- ANYONE forges proofs for such a key until a contribution is applied; an integer below r applies
    that delta; "draw" draws one from OS entropy, applies and wipes it (a single-party phase 2 with no transcript: sound only if
    that delta is gone and the .ptau is honest; `snarkjs zkey verify` does not accept the key).
    validate: 0 none, 1 field range and curve of every point read, 2 the G2 subgroup as well. device=-1 runs on host threads and
    gives the same bytes. UltraGroth keys, transcripts, beacons and verifying the .ptau's ceremony are out of scope.
    Refusals raise SetupError ("ptau: ..." / "r1cs: ..." / "setup: ...")."""
    L = load()
    opt = _SetupPtauOptions()
    opt.size = C.sizeof(_SetupPtauOptions)
    opt.log_domain, opt.validate = log_domain, validate
    if delta is None:
        opt.contribute = 0
    elif isinstance(delta, str):
        if delta != "draw":
            raise SetupError("setup: delta is None, an integer or \"draw\"")
        opt.contribute = 2
    else:
        opt.contribute = 1
        opt.delta = _le32(delta, "delta")
    return _setup_ptau_call(L.ug_setup_ptau_size, L.ug_setup_ptau_run, opt, r1cs, ptau, device, timings)


def _setup_ptau_call(size_fn, run_fn, opt, r1cs, ptau, device, timings):
    """the size entry, buffers of that size, the run entry: (zkey_bytes, vkey_dict, phase_ms_dict)"""
    import json
    r1cs = bytes(r1cs)
    with _Mapped(ptau) as m:
        zbytes, vmax = C.c_uint64(), C.c_uint64()
        _setup_call(size_fn, C.byref(opt), r1cs, len(r1cs), m.address, m.length, C.byref(zbytes), C.byref(vmax))
        zkey = C.create_string_buffer(zbytes.value)
        vkey = C.create_string_buffer(vmax.value)
        wrote, vlen = C.c_uint64(), C.c_uint64()
        ms = (C.c_double * len(SETUP_PTAU_PHASES))()
        _setup_call(run_fn, C.byref(opt), r1cs, len(r1cs), m.address, m.length, device, zkey, zbytes.value, C.byref(wrote), vkey, vmax.value,
                    C.byref(vlen), ms)
    phase_ms = dict(zip(SETUP_PTAU_PHASES, ms))
    if timings is not None:
        timings.update(phase_ms)
    return zkey.raw[:wrote.value], json.loads(vkey.raw[:vlen.value].decode()), phase_ms


def points_combine(col_ptr, index, coefs, points, g2=False, device=0, timing=None):
    """ug_points_combine (test tooling): one zkey-format record per column, the sum over the column's terms of coefs[t] *
    points[index[t]]. col_ptr: n_cols + 1 ascending offsets from 0; coefs: integers below r; points: zkey-format records (64
    bytes for G1, 128 for G2; all-zero is infinity). device=-1: host threads. timing: a list that receives (product ms, sum ms)."""
    rec = 128 if g2 else 64
    n_cols = len(col_ptr) - 1
    for c in coefs:
        if not 0 <= int(c) < 1 << 256:
            raise SetupError("setup: a coefficient is not below the field modulus")
    cp = (C.c_uint32 * (n_cols + 1))(*col_ptr)
    ix = (C.c_uint32 * max(1, len(index)))(*index)
    co = b"".join(int(c).to_bytes(32, "little") for c in coefs)
    pts = _joined(points, rec)
    out = C.create_string_buffer(max(1, rec * n_cols))
    ms = (C.c_double * 2)()
    _setup_call(load().ug_points_combine, device, 1 if g2 else 0, cp, n_cols, ix, co, pts, len(points), out, ms)
    if timing is not None:
        timing.append((ms[0], ms[1]))
    return [out.raw[rec * i:rec * i + rec] for i in range(n_cols)]


def points_scale(scalar, points, device=0, timing=None):
    """ug_points_scale (test tooling): [scalar * P] for G1 records P (64 bytes, all-zero is infinity), scalar an integer below r"""
    pts = _joined(points, 64)
    out = C.create_string_buffer(max(1, 64 * len(points)))
    ms = (C.c_double * 1)()
    _setup_call(load().ug_points_scale, device, bytes(_le32(scalar, "scalar")), pts, len(points), out, ms)
    if timing is not None:
        timing.append(ms[0])
    return [out.raw[64 * i:64 * i + 64] for i in range(len(points))]


UG_RATIO_LISTED = 16


class _RatioReport(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("bad_blocks", C.c_uint64), ("resolved_blocks", C.c_uint64), ("bad_records", C.c_uint64),
                ("resolved_records", C.c_uint64), ("exact", C.c_uint32), ("n_listed", C.c_uint32), ("index", C.c_uint64 * UG_RATIO_LISTED),
                ("kernel_ms", C.c_double * 2)]


def points_ratio_mask(x, y, q, device=0, max_blocks=0, timing=None):
    """ug_points_ratio_mask (test tooling): the ratio test alone. x, y: G1 records (64 bytes, all-zero is infinity) that passed the
    point check; q: a G2 record (128 bytes), not infinity, in the subgroup. Which i have e(x_i, q) != e(y_i, G2)? Blocks of 256
    records under fresh 128-bit weights first, then every record of the first max_blocks failing blocks (0: 64) by its own
    pairings. Returns (record_mask, block_mask, report): one byte per record of the resolved blocks, block after block (1 =
    wrong), one byte per block (1 = fails), and {"blocks", "bad_blocks", "resolved_blocks", "exact", "bad_records", "index"}:
    index the first 16 wrong records, ascending. device=-1: host threads, the same answers. timing: a list that receives
    (block-sums ms, pairings ms)."""
    if len(x) != len(y):
        raise SetupError("setup: x and y differ in length")
    n = len(x)
    xs, ys, qs = _joined(x, 64), _joined(y, 64), _joined([q], 128)
    rec_mask, blk_mask = C.create_string_buffer(max(1, n)), C.create_string_buffer(max(1, (n + 255) // 256))
    rep = _RatioReport()
    _setup_call(load().ug_points_ratio_mask, device, xs, ys, n, qs, int(max_blocks), rec_mask, blk_mask, C.byref(rep))
    if timing is not None:
        timing.append((rep.kernel_ms[0], rep.kernel_ms[1]))
    report = {"blocks": rep.blocks, "bad_blocks": rep.bad_blocks, "resolved_blocks": rep.resolved_blocks, "exact": rep.exact,
              "bad_records": rep.bad_records, "index": [rep.index[i] for i in range(rep.n_listed)]}
    return rec_mask.raw[:rep.resolved_records], blk_mask.raw[:rep.blocks], report


class _UltraSetupPtauOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_domain", C.c_uint32), ("validate", C.c_uint32), ("contribute", C.c_uint32),
                ("delta_round", C.c_ubyte * 32), ("delta_final", C.c_ubyte * 32), ("rand_indx", C.c_uint32), ("reserved", C.c_uint32),
                ("round_signals", C.POINTER(C.c_uint32)), ("n_round", C.c_uint64),
                ("final_signals", C.POINTER(C.c_uint32)), ("n_final", C.c_uint64)]


class _ScaleSegment(C.Structure):
    _fields_ = [("scalar", C.c_void_p), ("index", C.POINTER(C.c_uint32)), ("count", C.c_uint64)]


def ultra_setup_from_ptau(r1cs, ptau, ultra, delta=None, log_domain=0, device=0, validate=1, timings=None):
    """ug_ultra_setup_ptau_run: an UltraGroth (protocol 1337) proving key and verification key from a circuit's .r1cs, a .ptau
    prepared for phase 2 and the commitment rounds. Returns (zkey_bytes, vkey_dict, phase_ms_dict) as setup_from_ptau does.

    ultra: {"rand_indx": n, "round_signals": [...], "final_signals": [...]}, dev_setup's spec: the public signal that carries the
    challenge and the private signals committed before and after it; the lists must partition the private signals and go into
    the key in the order given. Which signal sits in which round is what the protocol's soundness rests on: it is the caller's.
    delta: None writes delta_round = delta_final = 1 -- ANYONE forges proofs for such a key until a contribution is applied; a pair
    (d_round, d_final) of integers below r applies those; "draw" draws both independently from OS entropy, applies and wipes them
    (a single-party phase 2 with no transcript: sound only if both are gone and the .ptau is honest).
    ptau, validate, device, timings: as setup_from_ptau. Transcripts, beacons and verifying the .ptau's ceremony are out of scope.
    Refusals raise SetupError ("ptau: ..." / "r1cs: ..." / "setup: ...")."""
    L = load()
    opt = _UltraSetupPtauOptions()
    opt.size = C.sizeof(_UltraSetupPtauOptions)
    opt.log_domain, opt.validate = log_domain, validate
    if ultra is None:
        raise SetupError("setup: an UltraGroth key needs ultra = {rand_indx, round_signals, final_signals}")
    keep = _ultra_lists(opt, ultra, "setup: ")
    if delta is None:
        opt.contribute = 0
    elif isinstance(delta, str):
        if delta != "draw":
            raise SetupError("setup: delta is None, a pair of integers or \"draw\"")
        opt.contribute = 2
    else:
        try:
            d_round, d_final = delta
        except (TypeError, ValueError):
            raise SetupError("setup: delta is None, a pair of integers or \"draw\"")
        opt.contribute = 1
        opt.delta_round = _le32(d_round, "delta_round")
        opt.delta_final = _le32(d_final, "delta_final")
    res = _setup_ptau_call(L.ug_ultra_setup_ptau_size, L.ug_ultra_setup_ptau_run, opt, r1cs, ptau, device, timings)
    del keep
    return res


def points_scale_segments(segments, points, device=0, timing=None):
    """ug_points_scale_segments (test tooling): the delta step of an UltraGroth key. segments: at most three (scalar, index, count),
    scalar an integer below r, index a list of count indexes into points or None (the first count records); points: G1 records
    (64 bytes, all-zero is infinity). Returns one list of records per segment: [scalar * points[index[i]]]. On the device all
    segments are one launch. device=-1: host threads. timing: a list that receives the kernel's ms."""
    pts = _joined(points, 64)
    segs = (_ScaleSegment * max(1, len(segments)))()
    keep = []
    total = 0
    for i, (scalar, index, count) in enumerate(segments):
        sc = C.create_string_buffer(bytes(_le32(scalar, "scalar")), 32)
        keep.append(sc)
        segs[i].scalar = C.cast(sc, C.c_void_p)
        if index is not None:
            if len(index) != count:
                raise SetupError("setup: an index list of another length")
            arr = (C.c_uint32 * max(1, count))(*index)
            keep.append(arr)
            segs[i].index = C.cast(arr, C.POINTER(C.c_uint32))
        segs[i].count = count
        total += count
    out = C.create_string_buffer(max(1, 64 * total))
    ms = (C.c_double * 1)()
    _setup_call(load().ug_points_scale_segments, device, len(segments), segs, pts, len(points), out, ms)
    if timing is not None:
        timing.append(ms[0])
    res, at = [], 0
    for _, _, count in segments:
        res.append([out.raw[64 * (at + i):64 * (at + i) + 64] for i in range(count)])
        at += count
    return res


PTAU_PREPARE_PHASES = ("parse", "point_check", "g1", "g2", "compare")


class _PtauPrepareOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("power", C.c_uint32), ("validate", C.c_uint32), ("mode", C.c_uint32)]


def _ptau_prepare_options(power, validate, mode):
    opt = _PtauPrepareOptions()
    opt.size = C.sizeof(_PtauPrepareOptions)
    for name, value in (("power", power), ("validate", validate)):
        if not 0 <= int(value) < 1 << 32:
            raise SetupError("setup: %s %d cannot be represented" % (name, value))
    opt.power, opt.validate, opt.mode = int(power), int(validate), mode
    return opt


def ptau_prepare(ptau, power=0, device=0, validate=1, timings=None):
    """ug_ptau_prepare_run: the .ptau prepared for phase 2 (what `snarkjs powersoftau prepare phase2` does), as bytes: the input's
    sections other than 12 - 15 in their order, then sections 12 - 15, the Lagrange forms of the powers of sections 2 - 5, made by
    an inverse transform over the points. Sections 12 - 15 already there are dropped and made again.

    ptau: bytes, a memoryview / mmap, or a path that is mapped here. power: 0 the file's own; a smaller one cuts the file to it
    first (the header's power changes, ceremonyPower stays). validate: as setup_from_ptau, over the records of sections 2 - 5 that
    are read. device=-1 runs on host threads and gives the same bytes. timings: a dict that receives the phase times in ms.
    Transcripts, beacons and verifying the ceremony's own contributions are out of scope. Refusals raise SetupError ("ptau: ...")."""
    L = load()
    opt = _ptau_prepare_options(power, validate, 0)
    with _Mapped(ptau) as m:
        size = C.c_uint64()
        _setup_call(L.ug_ptau_prepare_size, C.byref(opt), m.address, m.length, C.byref(size))
        out = C.create_string_buffer(max(1, size.value))
        wrote = C.c_uint64()
        ms = (C.c_double * len(PTAU_PREPARE_PHASES))()
        _setup_call(L.ug_ptau_prepare_run, C.byref(opt), m.address, m.length, device, out, size.value, C.byref(wrote), ms)
    if timings is not None:
        timings.update(zip(PTAU_PREPARE_PHASES, ms))
    return out.raw[:wrote.value]


def ptau_check(ptau, device=0, validate=1):
    """ug_ptau_prepare_run in check mode: sections 12 - 15 of a prepared .ptau are made again from its sections 2 - 5 and compared
    with the file's own, which setup_from_ptau takes on trust. None when all four agree; (section, index, message) for the first
    record that differs, in section order, the index counted in the section. Every other refusal (an unprepared file among
    them) raises SetupError."""
    import re
    L = load()
    opt = _ptau_prepare_options(0, validate, 1)
    with _Mapped(ptau) as m:
        _setup_call(L.ug_ptau_prepare_size, C.byref(opt), m.address, m.length, None)
        try:
            _setup_call(L.ug_ptau_prepare_run, C.byref(opt), m.address, m.length, device, None, 0, None, None)
        except SetupError as e:
            hit = re.fullmatch(r"ptau: section (\d+) point (\d+): does not match the powers", str(e))
            if not hit:
                raise
            return int(hit.group(1)), int(hit.group(2)), str(e)
    return None


def points_intt(points, log_n, g2=False, device=0, timing=None):
    """ug_points_intt (test tooling): ONE inverse transform of size N = 2^log_n over points: out[k] = (1 / N) sum_j omega^(-j k)
    points[j] with omega = 5^((r - 1) / N); points: at most N zkey-format records (64 bytes for G1, 128 for G2; all-zero is
    infinity), the rest taken as infinity. Returns N records. device=-1: host threads. timing: a list that receives
    (ms of the 1 / N products, ms of the stages)."""
    rec = 128 if g2 else 64
    pts = _joined(points, rec)
    if not 0 <= int(log_n) <= 28:
        raise SetupError("setup: log_n %d is not in 0 .. 28" % log_n)
    n = 1 << int(log_n)
    out = C.create_string_buffer(rec * n)
    ms = (C.c_double * 2)()
    _setup_call(load().ug_points_intt, device, 1 if g2 else 0, int(log_n), pts, len(points), out, ms)
    if timing is not None:
        timing.append((ms[0], ms[1]))
    return [out.raw[rec * i:rec * i + rec] for i in range(n)]


# ---------------------------------------------------------------------------------------------------
# a Groth16 key against its circuit and a prepared powers-of-tau file (include/ultragroth_hip.h: ug_zkey_verify_run, ug_r1cs_fold)
ZKEY_VERIFY_PHASES = ("parse", "point_check", "weights", "fold", "slice_msm", "key_msm", "h_msm", "pairing")
UG_ZKEY_INVALID = 2


class _ZkeyVerifyOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("validate", C.c_uint32)]


class _ZkeyVerifyReport(C.Structure):
    _fields_ = [("failed_sections", C.c_uint32), ("first_failed", C.c_int32), ("subgroup_checked", C.c_uint32), ("reserved", C.c_uint32),
                ("peak_device_bytes", C.c_uint64), ("fold_kernel_ms", C.c_double)]


def zkey_verify(r1cs, ptau, zkey, device=0, validate=2, timings=None):
    """ug_zkey_verify_run: is this Groth16 key the one `setup_from_ptau(r1cs, ptau)` gives under ONE delta, which nobody has to
    know? None when it is; (first_section, failed_sections, message) when not -- the sections 2 - 9 whose relation fails, in
    ascending order, and the section and message of the first failing relation. Refusals -- a file that cannot be read, sizes
    that do not belong together, a bad point, an UltraGroth key -- raise SetupError ("r1cs: ..." / "ptau: ..." / "zkey: ...").

    ptau and zkey: bytes, a memoryview / mmap, or a path that is mapped here. validate: 2 checks every point's field range and
    curve and every G2 point's subgroup; 1 leaves the subgroup out and is for timing only -- the relations' soundness needs the
    subgroup check, timings["subgroup_checked"] says False then. device=-1 evaluates the same relations on host threads.
    timings: a dict that receives the milliseconds of ZKEY_VERIFY_PHASES, "fold_kernel" and "peak_device_bytes".
    Who contributed (section 10's transcript, beacons, the .ptau's own ceremony) is not checked."""
    return _zkey_verify_call(load().ug_zkey_verify_run, _zkey_verify_options(_ZkeyVerifyOptions, validate), 9, r1cs, ptau, zkey, device, timings)


def _zkey_verify_options(struct, validate):
    opt = struct()
    opt.size = C.sizeof(struct)
    if not 0 <= int(validate) < 1 << 32:
        raise SetupError("zkey: validate %d is not 1 or 2" % validate)
    opt.validate = int(validate)
    return opt


def _zkey_verify_call(entry, opt, last_section, r1cs, ptau, zkey, device, timings):
    """one key check through `entry`: None, or (first_section, failed_sections, message) over the sections 2 .. last_section"""
    r1cs = bytes(r1cs)
    with _Mapped(ptau) as mp, _Mapped(zkey) as mz:
        rep = _ZkeyVerifyReport()
        ms = (C.c_double * len(ZKEY_VERIFY_PHASES))()
        err = C.create_string_buffer(1024)
        rc = entry(C.byref(opt), r1cs, len(r1cs), mp.address, mp.length, mz.address, mz.length, device, C.byref(rep), ms, err, len(err) - 1)
    msg = err.value.decode(errors="replace")
    if rc not in (0, UG_ZKEY_INVALID):
        raise SetupError(msg)
    if timings is not None:
        timings.update(zip(ZKEY_VERIFY_PHASES, ms))
        timings.update(fold_kernel=rep.fold_kernel_ms, peak_device_bytes=rep.peak_device_bytes, subgroup_checked=bool(rep.subgroup_checked))
    if rc == 0:
        return None
    return rep.first_failed, [i for i in range(2, last_section + 1) if rep.failed_sections >> i & 1], msg


class _UltraZkeyVerifyOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("validate", C.c_uint32), ("check_spec", C.c_uint32), ("rand_indx", C.c_uint32),
                ("round_signals", C.POINTER(C.c_uint32)), ("n_round", C.c_uint64),
                ("final_signals", C.POINTER(C.c_uint32)), ("n_final", C.c_uint64)]


def _ultra_lists(opt, ultra, prefix):
    """rand_indx and the two lists of a spec into an options struct; returns the arrays it points into"""
    try:
        rand, lists = int(ultra["rand_indx"]), [[int(x) for x in ultra[k]] for k in ("round_signals", "final_signals")]
    except (KeyError, TypeError, ValueError):
        raise SetupError(prefix + "ultra is {rand_indx, round_signals, final_signals}")
    if not all(0 <= x < 1 << 32 for x in [rand] + lists[0] + lists[1]):
        raise SetupError(prefix + "a signal of the spec is not below 2^32")
    opt.rand_indx = rand
    keep = []
    for name, count, lst in (("round_signals", "n_round", lists[0]), ("final_signals", "n_final", lists[1])):
        arr = (C.c_uint32 * max(1, len(lst)))(*lst)
        keep.append(arr)
        setattr(opt, name, C.cast(arr, C.POINTER(C.c_uint32)))
        setattr(opt, count, len(lst))
    return keep


def ultra_zkey_verify(r1cs, ptau, zkey, ultra=None, device=0, validate=2, timings=None):
    """ug_ultra_zkey_verify_run: is this UltraGroth key the one `ultra_setup_from_ptau(r1cs, ptau, ...)` gives under ONE delta_round
    and ONE delta_final, which nobody has to know? The report has zkey_verify's shape: None when it is; (first_section,
    failed_sections, message) when not, sections 2 - 12. Refusals -- zkey_verify's, a Groth16 key, a rand_indx that is not public,
    lists that do not partition the private signals -- raise SetupError.

    ultra: a spec {"rand_indx", "round_signals", "final_signals"} the key's own rounds must equal; None takes the key's rounds as
    they are -- WHO CHOSE THEM IS THEN NOT CHECKED, and which signal is committed before the challenge is what the protocol's
    soundness rests on. ptau, zkey, validate, device, timings: as zkey_verify. Transcripts, beacons and the .ptau's own ceremony
    are not checked."""
    opt = _zkey_verify_options(_UltraZkeyVerifyOptions, validate)
    keep = []
    if ultra is not None:
        opt.check_spec = 1
        keep = _ultra_lists(opt, ultra, "zkey: ")
    res = _zkey_verify_call(load().ug_ultra_zkey_verify_run, opt, 12, r1cs, ptau, zkey, device, timings)
    del keep
    return res


# naming the wrong records of a failing section (include/ultragroth_hip.h: ug_zkey_locate_run, ug_ultra_zkey_locate_run)
UG_ZKEY_LOCATE_SECTIONS, UG_ZKEY_LOCATE_LISTED = 7, 1024
LOCATE_METHODS = ("bytes", "ratio")


class _ZkeyLocateOptions(C.Structure):
    _fields_ = _ZkeyVerifyOptions._fields_ + [("max_listed", C.c_uint32), ("max_blocks", C.c_uint32)]


class _UltraZkeyLocateOptions(C.Structure):
    _fields_ = _UltraZkeyVerifyOptions._fields_ + [("max_listed", C.c_uint32), ("max_blocks", C.c_uint32)]


class _ZkeyLocateSection(C.Structure):
    _fields_ = [("section", C.c_uint32), ("method", C.c_uint32), ("records", C.c_uint64), ("blocks", C.c_uint64), ("bad_blocks", C.c_uint64),
                ("resolved_blocks", C.c_uint64), ("bad_records", C.c_uint64), ("exact", C.c_uint32), ("n_listed", C.c_uint32),
                ("kernel_ms", C.c_double * 2), ("index", C.c_uint64 * UG_ZKEY_LOCATE_LISTED)]


class _ZkeyLocateReport(C.Structure):
    _fields_ = [("n_sections", C.c_uint32), ("reserved", C.c_uint32), ("locate_ms", C.c_double),
                ("section", _ZkeyLocateSection * UG_ZKEY_LOCATE_SECTIONS)]


def _zkey_locate_call(entry, opt, last_section, r1cs, ptau, zkey, device, max_listed, max_blocks, timings):
    """one locate call: the verify call's answer with the located dict behind it"""
    for name, value in (("max_listed", max_listed), ("max_blocks", max_blocks)):
        if not 0 <= int(value) < 1 << 32:
            raise SetupError("zkey: %s %d is not below 2^32" % (name, value))
        setattr(opt, name, int(value))
    located = _ZkeyLocateReport()
    res = _zkey_verify_call(lambda *a: entry(*a[:9], C.byref(located), *a[9:]), opt, last_section, r1cs, ptau, zkey, device, timings)
    if timings is not None:
        timings.update(locate=located.locate_ms)
    if res is None:
        return None
    out = {}
    for e in located.section[:located.n_sections]:
        out[e.section] = {"records": e.records, "method": LOCATE_METHODS[e.method], "blocks": e.blocks, "bad_blocks": e.bad_blocks,
                          "resolved_blocks": e.resolved_blocks, "exact": e.exact, "bad_records": e.bad_records,
                          "index": [e.index[i] for i in range(e.n_listed)], "kernel_ms": (e.kernel_ms[0], e.kernel_ms[1])}
    return res + (out,)


def zkey_locate(r1cs, ptau, zkey, device=0, validate=2, max_listed=16, max_blocks=0, timings=None):
    """ug_zkey_locate_run: zkey_verify's answer, and WHICH RECORDS of every failing point section are wrong. None for a valid key;
    otherwise (first_section, failed_sections, message, located): the first three are zkey_verify's on the same files, located is
    a dict keyed by section -- 3, 5, 6, 7, 8, 9 where they fail -- of {"records", "method", "blocks", "bad_blocks",
    "resolved_blocks", "exact", "bad_records", "index", "kernel_ms"}. method "bytes" (5, 6, 7): the expected records were made and
    compared, the answer is complete. method "ratio" (3, 8, 9): blocks of 256 records are tested under fresh random weights, then
    every record of the first max_blocks failing blocks (0: 64) by its own pairings; exact = 0 says that more blocks fail than
    were resolved, and bad_records then counts the resolved ones only. index: the first max_listed wrong records, ascending, as
    places in the section (section 8: wire nPublic + 1 + i). A valid key costs what zkey_verify costs. timings also receives
    "locate", the milliseconds after the verdict."""
    return _zkey_locate_call(load().ug_zkey_locate_run, _zkey_verify_options(_ZkeyLocateOptions, validate), 9, r1cs, ptau, zkey, device,
                             max_listed, max_blocks, timings)


def ultra_zkey_locate(r1cs, ptau, zkey, ultra=None, device=0, validate=2, max_listed=16, max_blocks=0, timings=None):
    """ug_ultra_zkey_locate_run: ultra_zkey_verify's answer with zkey_locate's located dict, sections 3, 5, 6, 7, 8, 9 and 12. An
    index of section 8 is a place in the key's round list (record i is wire round_signals[i]), of section 9 in its final list."""
    opt = _zkey_verify_options(_UltraZkeyLocateOptions, validate)
    keep = []
    if ultra is not None:
        opt.check_spec = 1
        keep = _ultra_lists(opt, ultra, "zkey: ")
    res = _zkey_locate_call(load().ug_ultra_zkey_locate_run, opt, 12, r1cs, ptau, zkey, device, max_listed, max_blocks, timings)
    del keep
    return res


def r1cs_fold_classes(r1cs, rho, cls, log_domain=0, device=0, timing=None):
    """ug_r1cs_fold_classes (test tooling): the fold of an UltraGroth key check. rho as r1cs_fold; cls: one class 0, 1 or 2 per wire.
    Returns eleven lists of N integers: (a, b, c) over class 0, over class 1, over class 2, then a and b over all wires."""
    return _r1cs_fold_call(11, r1cs, rho, cls, log_domain, device, timing)


def r1cs_fold(r1cs, rho, log_domain=0, device=0, timing=None):
    """ug_r1cs_fold (test tooling): the fold of a key check. rho: one integer below 2^256 per wire, taken mod r. Returns six lists
    of N = 2^log_domain integers, (a_pub, b_pub, c_pub, a_priv, b_priv, c_priv): per row the sums of its A, B, C terms times rho
    over the wires 0 .. nPublic and over the others; the public rows carry rho_s in a_pub. log_domain 0: the smallest domain
    that fits. device=-1: host threads. timing: a list that receives the kernel's milliseconds."""
    return _r1cs_fold_call(6, r1cs, rho, None, log_domain, device, timing)


def _r1cs_fold_call(vectors, r1cs, rho, cls, log_domain, device, timing):
    """a fold entry: `vectors` lists of N integers; cls: the class list of ug_r1cs_fold_classes, None for ug_r1cs_fold"""
    r1cs = bytes(r1cs)
    try:
        info = r1cs_info(r1cs)
    except DeviceError as e:
        raise SetupError(str(e) if str(e).startswith("r1cs: ") else "r1cs: " + str(e))
    rho = [int(x) for x in rho]
    if cls is not None:
        cls = [int(x) for x in cls]
    if len(rho) != info["n_wires"] or any(not 0 <= x < 1 << 256 for x in rho):
        raise SetupError("r1cs: rho takes one integer below 2^256 per wire (%d wires)" % info["n_wires"])
    if cls is not None and (len(cls) != info["n_wires"] or any(not 0 <= x < 256 for x in cls)):
        raise SetupError("r1cs: cls takes one class per wire (%d wires)" % info["n_wires"])
    rows = info["n_constraints"] + info["n_pub_out"] + info["n_pub_in"] + 1
    log_n = int(log_domain) if log_domain else max(1, (rows - 1).bit_length())
    if not 0 < log_n <= 27:
        raise SetupError("r1cs: log_domain %d is not in 1 .. 27" % log_n)
    n = 1 << log_n
    out = C.create_string_buffer(vectors * 32 * n)
    ms = C.c_double()
    weights = b"".join(x.to_bytes(32, "little") for x in rho)
    if cls is None:
        _setup_call(load().ug_r1cs_fold, r1cs, len(r1cs), weights, log_n, device, out, C.byref(ms))
    else:
        _setup_call(load().ug_r1cs_fold_classes, r1cs, len(r1cs), weights, bytes(cls), log_n, device, out, C.byref(ms))
    if timing is not None:
        timing.append(ms.value)
    raw = out.raw
    return tuple([int.from_bytes(raw[32 * (v * n + k):32 * (v * n + k) + 32], "little") for k in range(n)] for v in range(vectors))


# ---------------------------------------------------------------------------------------------------
# verifier mirror (src/verifier.h)
VERIFIER_VALID_PROOF, VERIFIER_INVALID_PROOF, VERIFIER_ERROR = 0, 1, 2


class VerifierError(RuntimeError):
    pass


def _verify(fn, proof, inputs, verification_key):
    import json
    enc = lambda v: v if isinstance(v, bytes) else (v if isinstance(v, str) else json.dumps(v)).encode()
    err = C.create_string_buffer(256)
    rc = fn(enc(proof), enc(inputs), enc(verification_key), err, 255)
    if rc == VERIFIER_ERROR:
        raise VerifierError(err.value.decode(errors="replace"))
    return rc == VERIFIER_VALID_PROOF


def groth16_verify(proof, inputs, verification_key):
    """groth16_verify (src/verifier.h:22-29): JSON texts or parsed objects; True / False, VerifierError on bad data"""
    return _verify(load().groth16_verify, proof, inputs, verification_key)


def ultra_groth_verify(proof, inputs, verification_key):
    return _verify(load().ultra_groth_verify, proof, inputs, verification_key)


def _verify_batch(name, proofs, inputs, verification_key, device, judge=None, search_width=None, judge_min=None):
    import json
    from ._lib import VerifyBatchOptions, VerifyBatchStats, VerifyBatchStatsEx
    enc = lambda v: v if isinstance(v, bytes) else (v if isinstance(v, str) else json.dumps(v)).encode()
    if len(proofs) != len(inputs):
        raise ValueError("as many inputs as proofs")
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[enc(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[enc(p) for p in inputs])
    verdicts = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    err = C.create_string_buffer(512)
    if judge is None and search_width is None and judge_min is None:
        stats = VerifyBatchStats()
        rc = getattr(load(), name)(device, n, pa, ia, enc(verification_key), verdicts, C.byref(stats), err, 511)
        out = {f: getattr(stats, f) for f, _ in VerifyBatchStats._fields_}
    else:
        dflt = lambda v: -1 if v is None else int(v)
        opt = VerifyBatchOptions(C.sizeof(VerifyBatchOptions), int(bool(judge)), dflt(search_width), dflt(judge_min))
        stats = VerifyBatchStatsEx()
        rc = getattr(load(), name + "_opt")(device, n, pa, ia, enc(verification_key), verdicts, C.byref(opt), C.byref(stats), err, 511)
        out = {f: getattr(stats.base, f) for f, _ in VerifyBatchStats._fields_}
        out.update({f: getattr(stats, f) for f in ("judged", "judge_launches", "judge_ms")})
    if rc == VERIFIER_ERROR:
        raise VerifierError(err.value.decode(errors="replace"))
    return list(verdicts[:n]), out


def groth16_verify_batch(proofs, inputs, verification_key, device=0, judge=None, search_width=None, judge_min=None):
    """ug_groth16_verify_batch (include/verifier.h): many proofs under one key, one Miller loop each on `device` (host threads for
    device < 0) and one final exponentiation for a batch that holds. Returns (verdicts, stats): verdicts[i] is VERIFIER_VALID_PROOF,
    VERIFIER_INVALID_PROOF or VERIFIER_ERROR, what groth16_verify says of proof i alone; stats is the call's ug_verify_batch_stats
    as a dict. VerifierError for a key that does not parse or a device error.
    judge / search_width / judge_min: ug_groth16_verify_batch_opt. judge=True has the suspects of a rejected batch decided by
    their own equations on the device instead of searched and verified one by one on the host; search_width and judge_min None
    are the library's defaults. With any of the three given, stats also carries judged, judge_launches and judge_ms; with none,
    the call is the plain one (ULTRAGROTH_VERIFY_JUDGE in the environment decides)."""
    return _verify_batch("ug_groth16_verify_batch", proofs, inputs, verification_key, device, judge, search_width, judge_min)


def ultra_groth_verify_batch(proofs, inputs, verification_key, device=0, judge=None, search_width=None, judge_min=None):
    return _verify_batch("ug_ultra_groth_verify_batch", proofs, inputs, verification_key, device, judge, search_width, judge_min)


# ---- packed proof records (include/verifier.h) ----
def _enc_json(v):
    import json
    return v if isinstance(v, bytes) else (v if isinstance(v, str) else json.dumps(v)).encode()


def proof_pack(proof, ultra=False):
    """ug_proof_pack: proof.json (text or parsed) -> its 256-byte (UltraGroth: 320-byte) record. ValueError for a text that is no
    proof of that protocol or holds a value >= 2^256."""
    rec = C.create_string_buffer(320 if ultra else 256)
    if load().ug_proof_pack(1 if ultra else 0, _enc_json(proof), rec) != 0:
        raise ValueError("not a proof that a record can hold")
    return rec.raw


def proof_unpack(record, ultra=False):
    """ug_proof_unpack: the proof.json text a record stands for"""
    if len(record) != (320 if ultra else 256):
        raise ValueError("a record is %d bytes" % (320 if ultra else 256))
    out = C.create_string_buffer(1400)
    if load().ug_proof_unpack(1 if ultra else 0, bytes(record), out, 1400) != 0:
        raise ValueError("record does not unpack")
    return out.value.decode()


def inputs_pack(inputs, n_pub=None):
    """ug_inputs_pack: public.json (text or list) -> n_pub x 32 bytes; n_pub None: as many as the list holds"""
    import json
    if n_pub is None:
        n_pub = len(json.loads(inputs) if isinstance(inputs, (str, bytes)) else inputs)
    out = C.create_string_buffer(max(1, 32 * n_pub))
    if load().ug_inputs_pack(_enc_json(inputs), out, n_pub) != 0:
        raise ValueError("not %d inputs below 2^256" % n_pub)
    return out.raw[:32 * n_pub]


def inputs_unpack(block, n_pub=None):
    """ug_inputs_unpack: the public.json text of one proof's input block"""
    if n_pub is None:
        n_pub = len(block) // 32
    if n_pub <= 0 or len(block) != 32 * n_pub:
        raise ValueError("an input block is n_pub x 32 bytes")
    out = C.create_string_buffer(81 * n_pub + 3)
    if load().ug_inputs_unpack(bytes(block), n_pub, out, 81 * n_pub + 3) != 0:
        raise ValueError("inputs do not unpack")
    return out.value.decode()


# the record layouts of include/verifier.h (UG_RECORDS_*), described there
RECORDS_PLAIN, RECORDS_EVM, RECORDS_COMPRESSED = 0, 1, 2


def _record_bytes(ultra, format):
    size = load().ug_proof_record_bytes(1 if ultra else 0, int(format))
    if not size:
        raise ValueError("format: not one of RECORDS_PLAIN, RECORDS_EVM, RECORDS_COMPRESSED")
    return size


def proof_record_convert(record, from_format, to_format, ultra=False):
    """ug_proof_record_convert: one record from one layout to another, coordinates reduced mod q. ValueError when the source holds no
    point to convert: a compressed x without a y on the curve, or a point off its curve on the way to RECORDS_COMPRESSED."""
    if len(record) != _record_bytes(ultra, from_format):
        raise ValueError("a record of this layout is %d bytes" % _record_bytes(ultra, from_format))
    out = C.create_string_buffer(_record_bytes(ultra, to_format))
    rc = load().ug_proof_record_convert(1 if ultra else 0, int(from_format), bytes(record), int(to_format), out)
    if rc:
        raise ValueError("the record holds a point that does not convert" if rc == 1 else "record does not convert")
    return out.raw


def inputs_convert(block, from_format, to_format):
    """ug_inputs_convert: one proof's input block (n_pub x 32 bytes) from the byte order of one layout to that of another"""
    if not block or len(block) % 32:
        raise ValueError("an input block is n_pub x 32 bytes")
    out = C.create_string_buffer(len(block))
    if load().ug_inputs_convert(int(from_format), bytes(block), len(block) // 32, int(to_format), out) != 0:
        raise ValueError("format: not one of RECORDS_PLAIN, RECORDS_EVM, RECORDS_COMPRESSED")
    return out.raw


def _verify_batch_records(name, ultra, records, inputs, n_pub, verification_key, device, judge, search_width, judge_min, format=RECORDS_PLAIN):
    from ._lib import VerifyBatchOptions, VerifyBatchStats, VerifyBatchStatsEx
    size = _record_bytes(ultra, format)
    records, inputs = bytes(records), bytes(inputs)
    if len(records) % size:
        raise ValueError("records: a multiple of %d bytes" % size)
    n = len(records) // size
    if n_pub > 0 and len(inputs) != n * n_pub * 32:
        raise ValueError("inputs: count x n_pub x 32 bytes")
    verdicts = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    err = C.create_string_buffer(512)
    opt = None
    if not (judge is None and search_width is None and judge_min is None):
        dflt = lambda v: -1 if v is None else int(v)
        opt = C.byref(VerifyBatchOptions(C.sizeof(VerifyBatchOptions), int(bool(judge)), dflt(search_width), dflt(judge_min)))
    stats = VerifyBatchStatsEx()
    if format == RECORDS_PLAIN:                                     # the existing symbol
        rc = getattr(load(), name)(device, n, records or b"\0", inputs or b"\0", n_pub, _enc_json(verification_key), verdicts, opt, C.byref(stats), err, 511)
    else:
        rc = getattr(load(), name + "_fmt")(device, int(format), n, records or b"\0", inputs or b"\0", n_pub, _enc_json(verification_key), verdicts, opt,
                                            C.byref(stats), err, 511)
    if rc == VERIFIER_ERROR:
        raise VerifierError(err.value.decode(errors="replace"))
    out = {f: getattr(stats.base, f) for f, _ in VerifyBatchStats._fields_}
    out.update({f: getattr(stats, f) for f in ("judged", "judge_launches", "judge_ms")})
    return list(verdicts[:n]), out


def groth16_verify_batch_records(records, inputs, n_pub, verification_key, device=0, judge=None, search_width=None, judge_min=None,
                                 format=RECORDS_PLAIN):
    """ug_groth16_verify_batch_records (include/verifier.h): as groth16_verify_batch for proofs held as packed records -- `records`
    count x 256 bytes (proof_pack), `inputs` count x n_pub x 32 bytes (inputs_pack). On a device the raw records are uploaded once
    and reduced, checked and converted there; device < 0 is the same protocol on host threads. Returns (verdicts, stats) with the
    judge's counters always present; judge None takes it from the environment. format: the layout of `records` and the byte order of
    `inputs`, RECORDS_PLAIN (the default), RECORDS_EVM or RECORDS_COMPRESSED (count x 128 bytes), as include/verifier.h describes them."""
    return _verify_batch_records("ug_groth16_verify_batch_records", False, records, inputs, n_pub, verification_key, device, judge, search_width, judge_min,
                                 format)


def ultra_groth_verify_batch_records(records, inputs, n_pub, verification_key, device=0, judge=None, search_width=None, judge_min=None,
                                     format=RECORDS_PLAIN):
    return _verify_batch_records("ug_ultra_groth_verify_batch_records", True, records, inputs, n_pub, verification_key, device, judge, search_width,
                                 judge_min, format)


# ---- several keys in one call (include/verifier.h: the _keys calls) ----
def _keys_call(name, head, n, keys, key_of, tail, judge, search_width, judge_min):
    """the shared part of the _keys calls: key texts, key_of, options, stats; `head` / `tail` are the arguments before n_keys and
    between key_of and verdicts. Returns (verdicts, stats)."""
    from ._lib import VerifyBatchOptions, VerifyBatchStats, VerifyBatchStatsKeys
    if len(key_of) != n:
        raise ValueError("as many key indices as proofs")
    texts = [_enc_json(k) for k in keys]
    ka = (C.c_char_p * max(len(texts), 1))(*texts)
    ko = (C.c_int * max(n, 1))(*[int(q) for q in key_of])
    verdicts = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    err = C.create_string_buffer(512)
    opt = None
    if not (judge is None and search_width is None and judge_min is None):
        dflt = lambda v: -1 if v is None else int(v)
        opt = C.byref(VerifyBatchOptions(C.sizeof(VerifyBatchOptions), int(bool(judge)), dflt(search_width), dflt(judge_min)))
    stats = VerifyBatchStatsKeys()
    rc = getattr(load(), name)(*(head + [len(texts), ka, ko] + tail + [verdicts, opt, C.byref(stats), err, 511]))
    if rc == VERIFIER_ERROR:
        raise VerifierError(err.value.decode(errors="replace"))
    out = {f: getattr(stats.ex.base, f) for f, _ in VerifyBatchStats._fields_}
    out.update({f: getattr(stats.ex, f) for f in ("judged", "judge_launches", "judge_ms")})
    out.update({f: getattr(stats, f) for f in ("segments", "tree_launches", "key_checks")})
    return list(verdicts[:n]), out


def _verify_batch_keys(name, proofs, inputs, keys, key_of, device, judge, search_width, judge_min):
    if len(proofs) != len(inputs):
        raise ValueError("as many inputs as proofs")
    n = len(proofs)
    pa = (C.c_char_p * max(n, 1))(*[_enc_json(p) for p in proofs])
    ia = (C.c_char_p * max(n, 1))(*[_enc_json(p) for p in inputs])
    return _keys_call(name, [device, n, pa, ia], n, keys, key_of, [], judge, search_width, judge_min)


def groth16_verify_batch_keys(proofs, inputs, keys, key_of, device=0, judge=None, search_width=None, judge_min=None):
    """ug_groth16_verify_batch_keys (include/verifier.h): as groth16_verify_batch for proofs under several keys, one device pass and
    one final exponentiation per 65536 proofs whatever the number of keys. keys: the verification keys (texts or parsed); key_of[i]:
    the index of proof i's key. Proofs may come in any order; verdicts are in the caller's. Returns (verdicts, stats); stats carries
    the judge's counters and segments, tree_launches, key_checks. VerifierError for a bad key_of, a key that does not parse
    ("key <k>: ..."), or a device error."""
    return _verify_batch_keys("ug_groth16_verify_batch_keys", proofs, inputs, keys, key_of, device, judge, search_width, judge_min)


def ultra_groth_verify_batch_keys(proofs, inputs, keys, key_of, device=0, judge=None, search_width=None, judge_min=None):
    return _verify_batch_keys("ug_ultra_groth_verify_batch_keys", proofs, inputs, keys, key_of, device, judge, search_width, judge_min)


def inputs_pack_ragged(inputs, format=RECORDS_PLAIN):
    """The input block of the records calls under several keys: every proof's inputs (public.json text, list, or an input block of
    n x 32 plain bytes) one behind the other, each proof as many as its key has, in the byte order of `format`."""
    out = []
    for item in inputs:
        block = bytes(item) if isinstance(item, (bytes, bytearray)) and len(item) % 32 == 0 and len(item) else inputs_pack(item)
        out.append(block if format == RECORDS_PLAIN else inputs_convert(block, RECORDS_PLAIN, format))
    return b"".join(out)


def _verify_batch_records_keys(name, ultra, records, inputs, keys, key_of, device, format, judge, search_width, judge_min):
    import json
    size = _record_bytes(ultra, format)
    records, inputs = bytes(records), bytes(inputs)
    if len(records) % size:
        raise ValueError("records: a multiple of %d bytes" % size)
    n = len(records) // size
    n_pub = []
    for k in keys:                                                  # a key that does not parse is the library's to report
        try:
            j = json.loads(k) if isinstance(k, (str, bytes)) else k
            n_pub.append(max(1, len(j["IC"]) - 1))
        except (ValueError, KeyError, TypeError):
            n_pub.append(1)
    np_arr = (C.c_int * max(len(n_pub), 1))(*n_pub)
    return _keys_call(name, [device, int(format), n, records or b"\0", inputs or b"\0"], n, keys, key_of, [np_arr], judge, search_width, judge_min)


def groth16_verify_batch_records_keys(records, inputs, keys, key_of, device=0, format=RECORDS_PLAIN, judge=None, search_width=None, judge_min=None):
    """ug_groth16_verify_batch_records_keys: groth16_verify_batch_keys for packed records of `format`. inputs: the ragged block of
    inputs_pack_ragged -- proof i owns as many 32-byte values as its key has public inputs (len(IC) - 1, read from the key here)."""
    return _verify_batch_records_keys("ug_groth16_verify_batch_records_keys", False, records, inputs, keys, key_of, device, format, judge, search_width, judge_min)


def ultra_groth_verify_batch_records_keys(records, inputs, keys, key_of, device=0, format=RECORDS_PLAIN, judge=None, search_width=None, judge_min=None):
    return _verify_batch_records_keys("ug_ultra_groth_verify_batch_records_keys", True, records, inputs, keys, key_of, device, format, judge, search_width,
                                      judge_min)


class _ProverBase:
    _create = _prove = _destroy = _public_size_fn = None
    _proof_size = staticmethod(groth16_proof_size)

    def __init__(self, zkey):
        L = load()
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = getattr(L, self._create)(C.byref(self._h), zkey, len(zkey), err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))
        self._public_size = _public_size(getattr(L, self._public_size_fn), zkey)

    def prove(self, wtns, proof_size=None, public_size=None):
        """Returns (proof_json, public_json) -- the buffers up to their first NUL, as the CLI writes them."""
        L = load()
        psz = C.c_ulonglong(self._proof_size() if proof_size is None else proof_size)
        qsz = C.c_ulonglong(self._public_size if public_size is None else public_size)
        proof = C.create_string_buffer(max(psz.value, 1))
        pub = C.create_string_buffer(max(qsz.value, 1))
        err = C.create_string_buffer(1024)
        rc = getattr(L, self._prove)(self._h, wtns, len(wtns), proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    def prove_batch(self, wtns_list, proof_size=None, public_size=None):
        """ug_groth16_prover_prove_batch: [(proof_json, public_json), ...], one pair per witness, each what prove() returns for it
        (several witnesses per device pass on a created Groth16 or UltraGroth prover, one after the other on any other handle)"""
        k = len(wtns_list)
        keep = [bytes(w) for w in wtns_list]
        wb = (C.c_char_p * max(k, 1))(*keep)
        ws = (C.c_ulonglong * max(k, 1))(*[len(w) for w in keep])
        psz = (C.c_ulonglong * max(k, 1))(*([self._proof_size() if proof_size is None else proof_size] * k))
        qsz = (C.c_ulonglong * max(k, 1))(*([self._public_size if public_size is None else public_size] * k))
        proofs = [C.create_string_buffer(max(psz[i], 1)) for i in range(k)]
        pubs = [C.create_string_buffer(max(qsz[i], 1)) for i in range(k)]
        pb = (C.c_void_p * max(k, 1))(*[C.cast(b, C.c_void_p) for b in proofs])
        qb = (C.c_void_p * max(k, 1))(*[C.cast(b, C.c_void_p) for b in pubs])
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_prove_batch(self._h, k, wb, ws, pb, psz, qb, qsz, err, len(err) - 1)
        if rc != PROVER_OK:
            e = ProverError(rc, err.value.decode(errors="replace"))
            e.proof_sizes, e.public_sizes = list(psz[:k]), list(qsz[:k])
            raise e
        return [(p.raw.split(b"\0", 1)[0].decode(), q.raw.split(b"\0", 1)[0].decode()) for p, q in zip(proofs, pubs)]

    # the phases of a proof on a witness that stays resident in HBM (include/prover.h: ug_groth16_prover_load_witness / _run /
    # _finish; bench.py times run + finish): available on every prover object
    def load_witness(self, wtns):
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_load_witness(self._h, wtns, len(wtns), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def prove_resident(self):
        """ug_groth16_prover_prove_resident: one whole proof of the witness load_witness left in HBM"""
        psz = C.c_ulonglong(self._proof_size())
        qsz = C.c_ulonglong(self._public_size)
        proof = C.create_string_buffer(psz.value)
        pub = C.create_string_buffer(max(qsz.value, 1))
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_prove_resident(self._h, proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    def run(self):
        out = C.create_string_buffer(GROTH16_PARTIALS_SIZE)
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_run(self._h, out, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return out.raw

    def finish(self, partials_sum):
        psz = C.c_ulonglong(self._proof_size())
        qsz = C.c_ulonglong(self._public_size)
        proof = C.create_string_buffer(psz.value)
        pub = C.create_string_buffer(max(qsz.value, 1))
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_finish(self._h, bytes(partials_sum), proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    def attach_r1cs(self, r1cs):
        """ug_prover_attach_r1cs: from now on every proof of this prover checks its witness against the circuit's .r1cs and fails
        with "witness: constraint <k> does not hold (<n> of <m> fail)" when it breaks one; None detaches. ProverError when the
        file is not this zkey's circuit or the prover is of a kind that cannot check (nothing is attached then)."""
        err = C.create_string_buffer(1024)
        data = bytes(r1cs) if r1cs else None
        rc = load().ug_prover_attach_r1cs(self._h, data, len(data) if data else 0, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def batch_info(self):
        """ug_prover_batch_info: (passes, witnesses, last_width) of this prover's prove_batch calls since creation -- a pass of width V
        proved V witnesses together, so passes < witnesses says that passes were shared"""
        a, b, w = C.c_ulonglong(), C.c_ulonglong(), C.c_int()
        if load().ug_prover_batch_info(self._h, C.byref(a), C.byref(b), C.byref(w)) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "ug_prover_batch_info failed")
        return a.value, b.value, w.value

    def last_timings(self):
        """(msm_ms, fft_ms, total_ms) of the last prove: device time of the MSM and H-polynomial parts, host wall time."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        load().ug_prover_last_timings(self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def kernel_stats(self, g2=False, reset=False, which=None):
        """(avg launch ms, launches, units) since creation / last reset of the G1 (which 0) / G2 (1) bucket-accumulation
        kernel or the NTT pass kernel (2)."""
        a, l, e = C.c_double(), C.c_ulonglong(), C.c_ulonglong()
        w = (1 if g2 else 0) if which is None else which
        load().ug_prover_kernel_stats(self._h, w, C.byref(a), C.byref(l), C.byref(e), 1 if reset else 0)
        return a.value, l.value, e.value

    def last_upload_ms(self):
        """host wall time the last prove / load_witness spent bringing the witness into HBM"""
        a = C.c_double()
        load().ug_prover_last_upload_ms(self._h, C.byref(a))
        return a.value

    def tables_ready(self, wait=False):
        """ug_prover_tables_ready: True once the fixed-base window tables (built in the background after create) are in use;
        wait=True blocks until they are"""
        rc = load().ug_prover_tables_ready(self._h, 1 if wait else 0)
        if rc < 0:
            raise ProverError(PROVER_ERROR, "ug_prover_tables_ready failed")
        return rc == 1

    def table_plan(self):
        """ug_prover_table_plan for every schedule group of the prover: a list of (c, stride, bytes, ready) -- c = 0: classic
        windows; ready: the proofs use the tables"""
        L, plan, g = load(), [], 0
        c, st, b, r = C.c_int(), C.c_int(), C.c_ulonglong(), C.c_int()
        while L.ug_prover_table_plan(self._h, g, C.byref(c), C.byref(st), C.byref(b), C.byref(r)) == PROVER_OK:
            plan.append((c.value, st.value, b.value, bool(r.value)))
            g += 1
        return plan

    def close(self):
        if getattr(self, "_h", None):
            getattr(load(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Groth16Prover(_ProverBase):
    """groth16_prover_create / _prove / _destroy (src/prover.h:80-87,127-138,156-159)."""
    _create, _prove, _destroy = "groth16_prover_create", "groth16_prover_prove", "groth16_prover_destroy"
    _public_size_fn = "groth16_public_size_for_zkey_buf"


class UltraGrothProver(_ProverBase):
    """ultra_groth_prover_create / _prove / _destroy (src/prover.h:89-96,140-151,161-164)."""
    _create, _prove, _destroy = "ultra_groth_prover_create", "ultra_groth_prover_prove", "ultra_groth_prover_destroy"
    _public_size_fn = "ultra_groth_public_size_for_zkey_buf"
    _proof_size = staticmethod(ultra_groth_proof_size)


def _one_shot(fn, public_size_fn, proof_size, zkey, wtns):
    L = load()
    psz = C.c_ulonglong(proof_size)
    qsz = C.c_ulonglong(_public_size(getattr(L, public_size_fn), zkey))
    proof = C.create_string_buffer(max(psz.value, 1))
    pub = C.create_string_buffer(max(qsz.value, 1))
    err = C.create_string_buffer(1024)
    rc = getattr(L, fn)(zkey, len(zkey), wtns, len(wtns), proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
    if rc != PROVER_OK:
        raise ProverError(rc, err.value.decode(errors="replace"))
    return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()


def groth16_prover(zkey, wtns):
    """The reference's one-shot entry point groth16_prover (src/prover.h:173-185): create, prove once, destroy -- no window
    tables are built for it (they cannot pay for one proof)."""
    return _one_shot("groth16_prover", "groth16_public_size_for_zkey_buf", groth16_proof_size(), zkey, wtns)


def ultra_groth_prover(zkey, wtns):
    """ultra_groth_prover (src/prover.h:187-199)"""
    return _one_shot("ultra_groth_prover", "ultra_groth_public_size_for_zkey_buf", ultra_groth_proof_size(), zkey, wtns)


class Registry:
    """ug_registry_* (include/prover.h): several resident circuits on one device under an HBM budget -- the GPU form of
    the reference's FullProver map<circuit, Prover> (src/fullprover.cpp:21-63)."""
    NOT_LOADED, RESIDENT, RESIDENT_WITH_TABLES, EVICTED = 0, 1, 2, 3

    def __init__(self, device=0, hbm_budget_bytes=0):
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = load().ug_registry_create(C.byref(self._h), device, hbm_budget_bytes, err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))

    def _call(self, name, *args):
        err = C.create_string_buffer(1024)
        rc = getattr(load(), name)(self._h, *args, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def load(self, circuit, zkey):
        self._call("ug_registry_load", circuit.encode(), zkey, len(zkey))

    def load_file(self, path):
        self._call("ug_registry_load_file", path.encode())

    def prove(self, circuit, wtns, proof_size=1400, public_size=1 << 16):
        psz, qsz = C.c_ulonglong(proof_size), C.c_ulonglong(public_size)
        proof, pub = C.create_string_buffer(psz.value), C.create_string_buffer(qsz.value)
        self._call("ug_registry_prove", circuit.encode(), wtns, len(wtns), proof, C.byref(psz), pub, C.byref(qsz))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    def prove_batch(self, circuit, wtns_list, proof_size=1400, public_size=1 << 16):
        """ug_registry_prove_batch: [(proof_json, public_json), ...], one pair per witness, each what prove() returns for it; the
        circuit's prover shares a device pass among as many witnesses as the budget's free room holds"""
        k = len(wtns_list)
        keep = [bytes(w) for w in wtns_list]
        wb = (C.c_char_p * max(k, 1))(*keep)
        ws = (C.c_ulonglong * max(k, 1))(*[len(w) for w in keep])
        psz = (C.c_ulonglong * max(k, 1))(*([proof_size] * k))
        qsz = (C.c_ulonglong * max(k, 1))(*([public_size] * k))
        proofs = [C.create_string_buffer(max(proof_size, 1)) for _ in range(k)]
        pubs = [C.create_string_buffer(max(public_size, 1)) for _ in range(k)]
        pb = (C.c_void_p * max(k, 1))(*[C.cast(b, C.c_void_p) for b in proofs])
        qb = (C.c_void_p * max(k, 1))(*[C.cast(b, C.c_void_p) for b in pubs])
        err = C.create_string_buffer(1024)
        rc = load().ug_registry_prove_batch(self._h, circuit.encode(), k, wb, ws, pb, psz, qb, qsz, err, len(err) - 1)
        if rc != PROVER_OK:
            e = ProverError(rc, err.value.decode(errors="replace"))
            e.proof_sizes, e.public_sizes = list(psz[:k]), list(qsz[:k])
            raise e
        return [(p.raw.split(b"\0", 1)[0].decode(), q.raw.split(b"\0", 1)[0].decode()) for p, q in zip(proofs, pubs)]

    def attach_r1cs(self, circuit, r1cs):
        """ug_registry_attach_r1cs / _file: from now on every proof of the circuit, single or batched, checks its witness against
        this .r1cs -- bytes (the registry keeps a copy) or a path (str; read again when the circuit comes back after an eviction);
        None detaches. Rules and messages as Prover.attach_r1cs."""
        if isinstance(r1cs, str):
            self._call("ug_registry_attach_r1cs_file", circuit.encode(), r1cs.encode())
        else:
            data = bytes(r1cs) if r1cs else None
            self._call("ug_registry_attach_r1cs", circuit.encode(), data, len(data) if data else 0)

    def batch_info(self, circuit):
        """ug_registry_batch_info: (passes, witnesses, last_width) of the circuit's prove_batch calls since it was (re)loaded"""
        a, b, w = C.c_ulonglong(), C.c_ulonglong(), C.c_int()
        if load().ug_registry_batch_info(self._h, circuit.encode(), C.byref(a), C.byref(b), C.byref(w)) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "ug_registry_batch_info: circuit not loaded: " + circuit)
        return a.value, b.value, w.value

    def evict(self, circuit):
        self._call("ug_registry_evict", circuit.encode())

    def info(self, circuit=None):
        """(resident bytes, state, proofs) of a circuit; (bytes in use, resident circuits, proofs) for circuit=None"""
        b, st, n = C.c_ulonglong(), C.c_int(), C.c_ulonglong()
        load().ug_registry_info(self._h, circuit.encode() if circuit else None, C.byref(b), C.byref(st), C.byref(n))
        return b.value, st.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            load().ug_registry_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ShardLayout:
    """out[12] of ug_groth16_shard_layout (include/prover.h): what one rank of a many-device prover owns"""

    def __init__(self, raw):
        self.raw = list(raw)
        self.ranges = ((raw[0], raw[1]), (raw[2], raw[3]), (raw[4], raw[5]))      # witness, C, H -- as shard_ranges returns them
        self.witness, self.c, self.h = self.ranges
        self.q_log, self.first_residue, self.residues = raw[6], raw[7], raw[8]
        self.special = (raw[9], raw[10])
        self.chains = [k for k in range(3) if (raw[11] >> k) & 1]

    def __repr__(self):
        cls = "classes %d..%d of %d" % (self.first_residue, self.first_residue + self.residues, 1 << self.q_log) if self.q_log else "all buckets"
        return "ShardLayout(witness %s, h %s, %s, chains %s)" % (self.witness, self.h, cls, self.chains)


class ShardedGroth16Prover:
    """One rank of a sharded Groth16 prover (one process per GPU): see include/prover.h."""

    def __init__(self, zkey, device, rank, world, witness_range=None):
        """witness_range = (first, end): this rank's slice of the witness-indexed sections, chosen by the caller
        (ug_groth16_prover_create_sharded_range); None = the even split"""
        L = load()
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        if witness_range is None:
            rc = L.ug_groth16_prover_create_sharded(C.byref(self._h), zkey, len(zkey), device, rank, world, err, len(err) - 1)
        else:
            rc = L.ug_groth16_prover_create_sharded_range(C.byref(self._h), zkey, len(zkey), device, rank, world,
                                                          witness_range[0], witness_range[1], err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))
        self._public_size = groth16_public_size_for_zkey_buf(zkey)

    @classmethod
    def from_slices(cls, header, coefs, n_coefs, slices, device, rank, world, witness_range=None, public_size=None, layout=None):
        """ug_groth16_prover_create_sharded_slices: header = zkey section 2, coefs = section 4 records (None: no chain on
        this rank), slices = (A, B1, B2, C, H) buffers holding this rank's points only (shard_ranges tells which).
        layout (a ShardLayout from shard_layout): ug_groth16_prover_create_sharded_layout -- the rank's part of a many-device
        layout with bucket classes; the slices are those of layout.ranges"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        wr = (C.c_ulonglong * 2)(*witness_range) if witness_range is not None else None
        sizes = (C.c_ulonglong * 5)(*[len(x) for x in slices])
        if layout is not None:
            rc = load().ug_groth16_prover_create_sharded_layout(C.byref(self._h), header, len(header), coefs, n_coefs, *slices, sizes,
                                                                device, rank, world, (C.c_ulonglong * 12)(*layout.raw), err, len(err) - 1)
        else:
            rc = load().ug_groth16_prover_create_sharded_slices(C.byref(self._h), header, len(header), coefs, n_coefs, *slices, sizes,
                                                                device, rank, world, wr, err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))
        self._public_size = public_size
        return self

    @staticmethod
    def balanced_witness_range(n_vars, rank, world):
        """ug_groth16_balanced_witness_range: the witness range of a rank when ranks 0..2 also run an NTT chain each"""
        out = (C.c_ulonglong * 2)()
        if load().ug_groth16_balanced_witness_range(n_vars, rank, world, out) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "invalid shard rank / count")
        return out[0], out[1]

    @staticmethod
    def shard_layout(n_vars, n_public, domain, rank, world, point_ranges=0, hbm_bytes=0):
        """ug_groth16_shard_layout: the rank's part of the many-device layout the library would choose (point_ranges = 0), or of
        the one with that many base-point ranges (world / point_ranges ranks share a range through bucket classes)"""
        out = (C.c_ulonglong * 12)()
        if load().ug_groth16_shard_layout(n_vars, n_public, domain, rank, world, point_ranges, hbm_bytes, out) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "invalid shard rank / count or layout")
        return ShardLayout(list(out))

    @staticmethod
    def shard_ranges(n_vars, n_public, domain, rank, world, witness_range=None):
        """((witness first, end), (C first, end), (H first, end)) of a rank"""
        out = (C.c_ulonglong * 6)()
        wr = (C.c_ulonglong * 2)(*witness_range) if witness_range is not None else None
        if load().ug_groth16_shard_ranges(n_vars, n_public, domain, rank, world, wr, out) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "invalid shard rank / count or witness range")
        return (out[0], out[1]), (out[2], out[3]), (out[4], out[5])

    def load_witness(self, wtns):
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_load_witness(self._h, wtns, len(wtns), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def load_witness_part(self, wtns, part):
        """part 0: the scalars of this rank's MSM slice; part 1: the rest (only ranks that run an H-polynomial chain)"""
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_load_witness_part(self._h, wtns, len(wtns), part, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def run(self):
        """Device part on the resident witness; returns this rank's 384-byte partial sums."""
        out = C.create_string_buffer(GROTH16_PARTIALS_SIZE)
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_run(self._h, out, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return out.raw

    def _phase(self, name, *args):
        out = C.create_string_buffer(GROTH16_PARTIALS_SIZE)
        err = C.create_string_buffer(1024)
        rc = getattr(load(), name)(self._h, *args, *([out] if name.endswith(("_msm", "_msm_end")) else []), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return out.raw

    def run_witness_msm(self):
        """A, B1, B2, C partial sums of this rank (H record at infinity)"""
        return self._phase("ug_groth16_prover_run_witness_msm")

    def witness_msm_begin(self):
        """run_witness_msm without the wait: the four products are queued on the witness stream; drive the H branch (hpoly_chain,
        the slice exchange, hpoly_combine, run_h_msm) from this thread meanwhile, then witness_msm_end()"""
        self._phase("ug_groth16_prover_witness_msm_begin")

    def witness_msm_end(self):
        """the partial sums of the products witness_msm_begin queued (waits for them)"""
        return self._phase("ug_groth16_prover_witness_msm_end")

    def run_h_msm(self):
        """H partial sum of this rank from the h slice on the device (other records at infinity)"""
        return self._phase("ug_groth16_prover_run_h_msm")

    def hpoly_chain(self, which, device_ptr):
        """coset evaluations of polynomial `which` (0: A.w, 1: B.w, 2: their product) into device memory"""
        self._phase("ug_groth16_prover_hpoly_chain", which, C.c_void_p(device_ptr))

    def hpoly_combine(self, ptr_a, ptr_b, ptr_c):
        """this rank's slices of the three evaluation vectors (device pointers) -> its slice of h"""
        self._phase("ug_groth16_prover_hpoly_combine", C.c_void_p(ptr_a), C.c_void_p(ptr_b), C.c_void_p(ptr_c))

    def h_range(self):
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        load().ug_groth16_prover_h_range(self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    @staticmethod
    def add_partials(acc, other):
        a = C.create_string_buffer(bytes(acc), GROTH16_PARTIALS_SIZE)
        if load().ug_groth16_partials_add(a, bytes(other)) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "partials add failed")
        return a.raw

    def finish(self, partials_sum):
        psz = C.c_ulonglong(groth16_proof_size())
        qsz = C.c_ulonglong(self._public_size)
        proof = C.create_string_buffer(psz.value)
        pub = C.create_string_buffer(max(qsz.value, 1))
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_finish(self._h, bytes(partials_sum), proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    last_timings = _ProverBase.last_timings
    kernel_stats = _ProverBase.kernel_stats
    last_upload_ms = _ProverBase.last_upload_ms

    def close(self):
        if getattr(self, "_h", None):
            load().groth16_prover_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedUltraGrothProver(ShardedGroth16Prover):
    """One rank of a sharded UltraGroth prover (include/prover.h: ug_ultra_groth_prover_create_sharded and the phase
    calls it shares with the Groth16 one). Per proof: load_witness(uwtns) / round_commit() on every rank, the parts
    added (add_records), round_finish(sum) on one rank, apply_commitment(commitment) on every rank, then the Groth16
    phases and finish() on the rank that closed the round."""

    def __init__(self, zkey, device, rank, world):
        L = load()
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = L.ug_ultra_groth_prover_create_sharded(C.byref(self._h), zkey, len(zkey), device, rank, world, err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))
        self._public_size = ultra_groth_public_size_for_zkey_buf(zkey)

    @classmethod
    def from_slices(cls, header, coefs, n_coefs, slices, device, rank, world, public_size):
        """ug_ultra_groth_prover_create_sharded_slices: header = zkey section 2, coefs = section 4 records (None: no chain on this
        rank), slices = (A, B1, B2, C1, C2, H, round_indexes, final_round_indexes) buffers holding this rank's part only
        (shard_ranges tells which)"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        err = C.create_string_buffer(1024)
        sizes = (C.c_ulonglong * 8)(*[len(x) for x in slices])
        rc = load().ug_ultra_groth_prover_create_sharded_slices(C.byref(self._h), header, len(header), coefs, n_coefs, *slices, sizes,
                                                                device, rank, world, err, len(err) - 1)
        if rc != PROVER_OK:
            self._h = None
            raise ProverError(rc, err.value.decode(errors="replace"))
        self._public_size = public_size
        return self

    @staticmethod
    def shard_ranges(n_vars, domain, n_round, n_final, rank, world):
        """((witness first, end), (round set first, end), (final set first, end), (H first, end)) of a rank"""
        out = (C.c_ulonglong * 8)()
        if load().ug_ultra_groth_shard_ranges(n_vars, domain, n_round, n_final, rank, world, out) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "invalid shard rank / count")
        return (out[0], out[1]), (out[2], out[3]), (out[4], out[5]), (out[6], out[7])

    def _call(self, name, *args):
        err = C.create_string_buffer(1024)
        rc = getattr(load(), name)(self._h, *args, err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))

    def round_commit(self):
        out = C.create_string_buffer(64)
        self._call("ug_ultra_groth_prover_round_commit", out)
        return out.raw

    def round_finish(self, commit_sum):
        out = C.create_string_buffer(64)
        self._call("ug_ultra_groth_prover_round_finish", bytes(commit_sum), out)
        return out.raw

    def apply_commitment(self, commitment):
        self._call("ug_ultra_groth_prover_apply_commitment", bytes(commitment))

    @staticmethod
    def add_records(acc, other):
        a = C.create_string_buffer(bytes(acc), 64)
        if load().ug_g1_record_add(a, bytes(other)) != PROVER_OK:
            raise ProverError(PROVER_ERROR, "record add failed")
        return a.raw

    def finish(self, partials_sum):
        psz = C.c_ulonglong(ultra_groth_proof_size())
        qsz = C.c_ulonglong(self._public_size)
        proof = C.create_string_buffer(psz.value)
        pub = C.create_string_buffer(max(qsz.value, 1))
        err = C.create_string_buffer(1024)
        rc = load().ug_groth16_prover_finish(self._h, bytes(partials_sum), proof, C.byref(psz), pub, C.byref(qsz), err, len(err) - 1)
        if rc != PROVER_OK:
            raise ProverError(rc, err.value.decode(errors="replace"))
        return proof.raw.split(b"\0", 1)[0].decode(), pub.raw.split(b"\0", 1)[0].decode()

    def close(self):
        if getattr(self, "_h", None):
            load().ultra_groth_prover_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------------------------------------------
# inner ABI (include/ultragroth_hip.h)

class _TableGroup(C.Structure):
    _fields_ = [("scalars", C.c_uint64), ("g1_points", C.c_uint64), ("g2_points", C.c_uint64)]


class _TableChoice(C.Structure):
    _fields_ = [("c", C.c_int), ("stride", C.c_int), ("bytes", C.c_uint64)]


def tables_bytes(n, g2, c, stride=1):
    """ug_bases_tables_bytes_strided: the device memory window tables of width c and this stride add to n points"""
    return load().ug_bases_tables_bytes_strided(n, 1 if g2 else 0, c, stride)


def plan_window_tables(groups, budget):
    """ug_plan_window_tables (host only): groups = [(scalars, g1_points, g2_points), ...] -> [(c, stride, bytes), ...] within
    `budget` bytes (c = 0: classic windows)"""
    k = len(groups)
    arr = (_TableGroup * max(k, 1))(*[_TableGroup(*g) for g in groups])
    out = (_TableChoice * max(k, 1))()
    _check(load().ug_plan_window_tables(arr, k, budget, out))
    return [(out[i].c, out[i].stride, out[i].bytes) for i in range(k)]


BATCH_MAX = 16          # include/ultragroth_hip.h: UG_BATCH_MAX


class _BatchSchedule(C.Structure):
    _fields_ = [("scalars", C.c_uint64), ("c", C.c_int), ("stride", C.c_int)]


def plan_proof_batch(schedules, n_vars, domain, free_bytes, requested):
    """ug_plan_proof_batch (host only): schedules = [(scalars, c, stride), ...] (c = 0: classic windows) -> witnesses per device
    pass, 1 <= V <= min(requested, BATCH_MAX)"""
    k = len(schedules)
    arr = (_BatchSchedule * max(k, 1))(*[_BatchSchedule(*s) for s in schedules])
    v = load().ug_plan_proof_batch(arr, k, n_vars, domain, free_bytes, requested)
    if v < 1:
        raise ValueError("ug_plan_proof_batch: bad arguments")
    return v


def plan_proof_batch_aux(schedules, n_vars, domain, aux_bytes_per_witness, free_bytes, requested):
    """ug_plan_proof_batch_aux (host only): plan_proof_batch with aux_bytes_per_witness more device bytes per witness of a pass"""
    k = len(schedules)
    arr = (_BatchSchedule * max(k, 1))(*[_BatchSchedule(*s) for s in schedules])
    v = load().ug_plan_proof_batch_aux(arr, k, n_vars, domain, aux_bytes_per_witness, free_bytes, requested)
    if v < 1:
        raise ValueError("ug_plan_proof_batch_aux: bad arguments")
    return v


class _LookupLists(C.Structure):
    _fields_ = [("frequencies", C.c_void_p), ("lookup_size", C.c_uint64), ("chunks", C.c_void_p), ("n_chunks", C.c_uint64),
                ("w_idx", C.c_void_p), ("p_idx", C.c_void_p), ("n", C.c_uint64)]


def _lookup_lists(lists):
    """lists = [dict(freq=, chunks=, w_idx=, p_idx=, lookup_size=) ...] (numpy uint32 arrays; freq or the index lists may be
    missing) -> (ug_lookup_lists array, the arrays it points into)"""
    import numpy as np
    keep, arr = [], (_LookupLists * len(lists))()
    for v, l in enumerate(lists):
        a = {k: np.ascontiguousarray(l.get(k, ()), dtype=np.uint32) for k in ("freq", "chunks", "w_idx", "p_idx")}
        keep.append(a)
        arr[v] = _LookupLists(a["freq"].ctypes.data, l.get("lookup_size", len(a["freq"])), a["chunks"].ctypes.data, len(a["chunks"]),
                              a["w_idx"].ctypes.data, a["p_idx"].ctypes.data, len(a["w_idx"]))
    return arr, keep


def lookup_vectors_bytes(vector_stride, lists):
    """ug_lookup_vectors_bytes (host only): device bytes a vector lookup call takes for these lists"""
    arr, _keep = _lookup_lists(lists)
    return load().ug_lookup_vectors_bytes(vector_stride, arr, len(lists))


class Device:
    """A ug_ctx plus convenience wrappers in the reference's byte formats."""

    def __init__(self, device=0):
        self._L = load()
        self._h = C.c_void_p()
        _check(self._L.ug_ctx_create(C.byref(self._h), device))

    def close(self):
        if getattr(self, "_h", None):
            self._L.ug_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check_points(self, points, n, g2=False, level=1):
        """ug_points_check over n zkey-format records: None when every point passes, else (index, reason) of the lowest bad one"""
        f = _PointFault()
        _check(self._L.ug_points_check(self._h, 1 if g2 else 0, points, n, level, C.byref(f)))
        return None if f.reason == UG_POINT_OK else (f.index, f.reason)

    def points_check_mask(self, points, n, g2=False, level=1):
        """ug_points_check_mask over n zkey-format records: n bytes, byte i = UG_POINT_OK or the first rule record i breaks"""
        out = C.create_string_buffer(max(1, n))
        _check(self._L.ug_points_check_mask(self._h, 1 if g2 else 0, points, n, level, out))
        return out.raw[:n]

    def check_on_create(self, level):
        """ug_ctx_check_points: the sets created on this device from now on check their records (0: off)"""
        _check(self._L.ug_ctx_check_points(self._h, level))

    # -- raw handles
    def bases(self, points, n, g2=False, global_first=0, table_c=0, table_stride=1):
        """table_c: also precompute the fixed-base window tables of that width (ug_bases_precompute; with table_stride > 1
        the strided tables of ug_bases_precompute_strided)"""
        h = C.c_void_p()
        fn = self._L.ug_bases_create_g2 if g2 else self._L.ug_bases_create_g1
        _check(fn(self._h, points, n, global_first, C.byref(h)))
        b = _Handle(h, self._L.ug_bases_destroy, self)
        if table_c:
            if table_stride == 1:
                _check(self._L.ug_bases_precompute(h, table_c))
            else:
                _check(self._L.ug_bases_precompute_strided(h, table_c, table_stride))
        return b

    def bases_group(self, members, group_first, slots, table_c=0, table_stride=1):
        """ug_bases_create_group_g1: members = [(points bytes, n, first scalar index), ...] (2 or 3 G1 sets sharing their scalars)"""
        k = len(members)
        keep = [_buf(bytes(p)) if not isinstance(p, C.Array) else p for p, _, _ in members]
        hosts = (C.c_void_p * k)(*[C.cast(b, C.c_void_p) for b in keep])
        ns = (C.c_uint64 * k)(*[n for _, n, _ in members])
        firsts = (C.c_uint64 * k)(*[f for _, _, f in members])
        h = C.c_void_p()
        if table_stride == 1:
            _check(self._L.ug_bases_create_group_g1(self._h, k, hosts, ns, firsts, group_first, slots, table_c, C.byref(h)))
        else:
            _check(self._L.ug_bases_create_group_strided_g1(self._h, k, hosts, ns, firsts, group_first, slots, table_c, table_stride,
                                                            C.byref(h)))
        g = _Handle(h, self._L.ug_bases_destroy, self)
        g.members = k
        return g

    def msm_group(self, group, schedule):
        """the K sums of a base group over a schedule (ug_msm_group_enqueue + ug_ctx_collect): K affine records (V records each
        over a schedule of V vectors)"""
        outs = [C.create_string_buffer(64 * getattr(schedule, "vectors", 1)) for _ in range(group.members)]
        arr = (C.c_void_p * group.members)(*[C.cast(o, C.c_void_p) for o in outs])
        _check(self._L.ug_msm_group_enqueue(self._h, group.h, schedule.h, arr))
        _check(self._L.ug_ctx_collect(self._h))
        return [o.raw for o in outs]

    def msm_witness(self, group, g2set, schedule):
        """the witness products of a proof (ug_msm_witness_enqueue + ug_ctx_collect): the K sums of a base group, then the sum of
        a G2 set over the same schedule -- K records of 64 bytes and one of 128 (V records each over a schedule of V vectors)"""
        v = getattr(schedule, "vectors", 1)
        outs = [C.create_string_buffer(64 * v) for _ in range(group.members)]
        out2 = C.create_string_buffer(128 * v)
        arr = (C.c_void_p * group.members)(*[C.cast(o, C.c_void_p) for o in outs])
        _check(self._L.ug_msm_witness_enqueue(self._h, group.h, g2set.h, schedule.h, arr, out2))
        _check(self._L.ug_ctx_collect(self._h))
        return [o.raw for o in outs] + [out2.raw]

    def dvec(self, n, data=None):
        h = C.c_void_p()
        _check(self._L.ug_dvec_create(self._h, n, C.byref(h)))
        v = _Handle(h, self._L.ug_dvec_destroy, self)
        if data is not None:
            _check(self._L.ug_dvec_upload(h, data, len(data) // 32))
        return v

    def download(self, dvec, first, n):
        out = C.create_string_buffer(n * 32)
        _check(self._L.ug_dvec_download(dvec.h, out, first, n))
        return out.raw

    def apply_lookup(self, dvec, w_idx, p_idx, chunks, table, lookup_size):
        """ug_dvec_apply_lookup: dvec[w_idx[i]] = push[p_idx[i]] in order (numpy uint32 index arrays, table bytes)"""
        import numpy as np
        w = np.ascontiguousarray(w_idx, dtype=np.uint32); p = np.ascontiguousarray(p_idx, dtype=np.uint32)
        c = np.ascontiguousarray(chunks, dtype=np.uint32)
        _check(self._L.ug_dvec_apply_lookup(dvec.h, w.ctypes.data, p.ctypes.data, len(w), c.ctypes.data, len(c), table, lookup_size))

    def lookup_table(self, rand_plain, freq):
        """ug_fr_lookup_table: [rand | inv2 | prod] as bytes for a 32-byte plain challenge and uint32 frequencies"""
        import numpy as np
        f = np.ascontiguousarray(freq, dtype=np.uint32)
        out = C.create_string_buffer((1 + 2 * len(f)) * 32)
        _check(self._L.ug_fr_lookup_table(self._h, rand_plain, f.ctypes.data, len(f), out))
        return out.raw

    def lookup_tables(self, rands_plain, freqs):
        """ug_fr_lookup_tables: the tables of V challenges (V * 32 bytes) and V frequency lists, one device call"""
        arr, _keep = _lookup_lists([dict(freq=f) for f in freqs])
        outs = [C.create_string_buffer((1 + 2 * len(f)) * 32) for f in freqs]
        ptrs = (C.c_void_p * len(outs))(*[C.cast(o, C.c_void_p) for o in outs])
        _check(self._L.ug_fr_lookup_tables(self._h, len(freqs), rands_plain, arr, ptrs))
        return [o.raw for o in outs]

    def apply_lookup_vectors(self, dvec, vector_stride, lists, tables):
        """ug_dvec_apply_lookup_vectors: apply_lookup for V witnesses, vector v of dvec at v * vector_stride; lists = [dict(w_idx=,
        p_idx=, chunks=, lookup_size=) ...], tables = V byte strings"""
        arr, _keep = _lookup_lists(lists)
        bufs = [_buf(bytes(t)) for t in tables]
        ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p) for b in bufs])
        _check(self._L.ug_dvec_apply_lookup_vectors(dvec.h, vector_stride, len(lists), arr, ptrs))

    def complete_lookup_vectors(self, dvec, vector_stride, rands_plain, lists, want_tables=True):
        """ug_dvec_complete_lookup_vectors: tables and writes of V witnesses in one call; lists = [dict(freq=, chunks=, w_idx=,
        p_idx=) ...]; returns the V tables (or None)"""
        arr, _keep = _lookup_lists(lists)
        outs = [C.create_string_buffer((1 + 2 * len(l["freq"])) * 32) for l in lists]
        ptrs = (C.c_void_p * len(outs))(*[C.cast(o, C.c_void_p) for o in outs])
        _check(self._L.ug_dvec_complete_lookup_vectors(dvec.h, vector_stride, len(lists), rands_plain, arr, ptrs if want_tables else None))
        return [o.raw for o in outs] if want_tables else None

    def schedule(self, dvec, first, count, table_c=0, classes=None, table_stride=1):
        """classes (ug_schedule_set_classes): (q_log, first_residue, residues, specials, special_first, special_count);
        table_c / table_stride: a schedule for (strided) window tables"""
        h = C.c_void_p()
        _check(self._L.ug_schedule_create(self._h, C.byref(h)))
        s = _Handle(h, self._L.ug_schedule_destroy, self)
        if classes is not None:
            _check(self._L.ug_schedule_set_classes(h, *classes))
        if table_c and table_stride != 1:
            _check(self._L.ug_schedule_build_tables_strided(h, dvec.h, first, count, table_c, table_stride))
        elif table_c:
            _check(self._L.ug_schedule_build_tables(h, dvec.h, first, count, table_c))
        else:
            _check(self._L.ug_schedule_build(h, dvec.h, first, count))
        return s

    def schedule_vectors(self, dvec, first, count, vectors, vector_stride, table_c=0, table_stride=1):
        """ug_schedule_build_vectors: `vectors` scalar vectors of `count` scalars, vector v at first + v * vector_stride; products
        over the schedule return `vectors` consecutive records"""
        h = C.c_void_p()
        _check(self._L.ug_schedule_create(self._h, C.byref(h)))
        s = _Handle(h, self._L.ug_schedule_destroy, self)
        _check(self._L.ug_schedule_build_vectors(h, dvec.h, first, count, vectors, vector_stride, table_c, table_stride))
        s.vectors = vectors
        return s

    def gather_index_at(self, out, out_first, src, host_index):
        """ug_index_create + ug_dvec_gather_index_at: out[out_first + i] = src[host_index[i]]"""
        import numpy as np
        idx = np.ascontiguousarray(host_index, dtype=np.uint32)
        h = C.c_void_p()
        _check(self._L.ug_index_create(self._h, idx.ctypes.data, len(idx), C.byref(h)))
        try:
            _check(self._L.ug_dvec_gather_index_at(out.h, out_first, src.h, h))
            _check(self._L.ug_ctx_sync(self._h))
        finally:
            self._L.ug_index_destroy(h)

    def table_window(self, n):
        return self._L.ug_msm_table_window(n)

    def tables_bytes(self, n, g2, c, s=1):
        return tables_bytes(n, g2, c, s)

    def mem_info(self):
        f, t = C.c_uint64(), C.c_uint64()
        _check(self._L.ug_ctx_mem_info(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def msm(self, bases, schedule, index_shift=0, g2=False):
        out = C.create_string_buffer((128 if g2 else 64) * getattr(schedule, "vectors", 1))
        fn = self._L.ug_msm_g2 if g2 else self._L.ug_msm_g1
        _check(fn(self._h, bases.h, schedule.h, index_shift, out))
        return out.raw

    def msm_batch(self, bases_list, schedule, index_shifts=None):
        """ug_msm_batch: several products over one schedule with one host synchronisation; bases_list holds
        (bases handle, is_g2) pairs; returns the affine records"""
        n = len(bases_list)
        outs = [C.create_string_buffer((128 if g2 else 64) * getattr(schedule, "vectors", 1)) for _, g2 in bases_list]
        arr_b = (C.c_void_p * n)(*[b.h for b, _ in bases_list])
        arr_o = (C.c_void_p * n)(*[C.cast(o, C.c_void_p) for o in outs])
        arr_s = (C.c_int64 * n)(*index_shifts) if index_shifts is not None else None
        _check(self._L.ug_msm_batch(self._h, n, arr_b, schedule.h, arr_s, arr_o))
        return [o.raw for o in outs]

    # -- one-shot helpers
    def msm_g1(self, points, scalars, n, table_c=0):
        """sum scalars[i] * points[i]; points n x 64 B zkey records, scalars n x 32 B plain integers."""
        b = self.bases(points, n, table_c=table_c)
        s = self.schedule(self.dvec(max(n, 1), scalars if n else None), 0, n, table_c=table_c)
        return self.msm(b, s)

    def msm_g2(self, points, scalars, n, table_c=0):
        b = self.bases(points, n, g2=True, table_c=table_c)
        s = self.schedule(self.dvec(max(n, 1), scalars if n else None), 0, n, table_c=table_c)
        return self.msm(b, s, g2=True)

    def ntt(self, data, logn, inverse=False):
        buf = C.create_string_buffer(bytes(data), len(data))
        _check(self._L.ug_fr_ntt(self._h, buf, logn, 1 if inverse else 0))
        return buf.raw

    def field_op(self, field, op, a, b):
        n = len(a) // 32
        out = C.create_string_buffer(max(len(a), 1))
        _check(self._L.ug_field_op(self._h, field, op, out, bytes(a), bytes(b), n))
        return out.raw[:len(a)]

    def hpoly(self, coefs, ncoefs, domain, nvars):
        h = C.c_void_p()
        _check(self._L.ug_hpoly_create(self._h, coefs, ncoefs, domain, nvars, C.byref(h)))
        return _HPoly(h, self, domain)

    def r1cs(self, data):
        """ug_r1cs_create: the three matrices of an .r1cs resident on this device"""
        h = C.c_void_p()
        _check(self._L.ug_r1cs_create(self._h, data, len(data), C.byref(h)))
        return _R1cs(h, self)

    def timings(self, reset=False):
        a, b = C.c_double(), C.c_double()
        _check(self._L.ug_ctx_timings(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return a.value, b.value

    def kernel_stats(self, g2=False, reset=False, which=None):
        a, l, e = C.c_double(), C.c_uint64(), C.c_uint64()
        w = (1 if g2 else 0) if which is None else which
        _check(self._L.ug_ctx_kernel_stats(self._h, w, C.byref(a), C.byref(l), C.byref(e), 1 if reset else 0))
        return a.value, l.value, e.value


class _Handle:
    def __init__(self, h, destroy, owner):
        self.h, self._destroy, self._owner = h, destroy, owner

    def __del__(self):
        try:
            if self.h and getattr(self._owner, "_h", None):
                self._destroy(self.h)
            self.h = None
        except Exception:
            pass


class _HPoly(_Handle):
    def __init__(self, h, dev, domain):
        super().__init__(h, dev._L.ug_hpoly_destroy, dev)
        self.dev, self.domain = dev, domain

    def run(self, wtns_dvec):
        """h vector (domain x 32 B plain integers) as a device vector"""
        out = self.dev.dvec(self.domain)
        _check(self.dev._L.ug_hpoly_run(self.h, wtns_dvec.h, out.h))
        return out

    def run_vectors(self, wtns_dvec, stride, vectors, out=None, h_stride=None):
        """ug_hpoly_run_vectors: the block for `vectors` witnesses, witness v at element v * stride of wtns_dvec; h vector v at
        element v * h_stride (default: the domain) of `out` (default: a fresh device vector), which is returned"""
        h_stride = self.domain if h_stride is None else h_stride
        if out is None:
            out = self.dev.dvec(max(vectors, 1) * h_stride)
        _check(self.dev._L.ug_hpoly_run_vectors(self.h, wtns_dvec.h, stride, vectors, out.h, h_stride))
        return out

    def reserve_vectors(self, g):
        """ug_hpoly_reserve_vectors: workspaces for launch groups of g vectors (hpoly_vectors_bytes(domain, g) bytes)"""
        _check(self.dev._L.ug_hpoly_reserve_vectors(self.h, g))

    @property
    def group(self):
        """ug_hpoly_group: the largest launch group of the last run_vectors call (before any: the reserved group)"""
        return self.dev._L.ug_hpoly_group(self.h)

    def debug_abc(self):
        bufs = [C.create_string_buffer(self.domain * 32) for _ in range(3)]
        _check(self.dev._L.ug_hpoly_debug_abc(self.h, *bufs))
        return [b.raw for b in bufs]


HPoly = _HPoly


class _R1cs(_Handle):
    def __init__(self, h, dev):
        super().__init__(h, dev._L.ug_r1cs_destroy, dev)
        self.dev = dev

    def info(self):
        info = _R1csInfo()
        _check(self.dev._L.ug_r1cs_get_info(self.h, C.byref(info)))
        return info.as_dict()

    def check(self, dvec, first=0, want_mask=False):
        """ug_r1cs_check of the witness at elements [first, first + n_wires) of a device vector: a dict with failed, first, a, b, c
        (integers; a, b, c None when nothing fails), device_ms, and mask (bytes, one per constraint: 0 holds, 1 fails) if asked for"""
        rep = _R1csReport()
        mask = C.create_string_buffer(max(1, self.info()["n_constraints"])) if want_mask else None
        _check(self.dev._L.ug_r1cs_check(self.h, dvec.h, first, C.byref(rep), mask))
        out = {"failed": rep.failed, "first": rep.first if rep.failed else None, "device_ms": rep.device_ms,
               "a": _le(rep.a) if rep.failed else None, "b": _le(rep.b) if rep.failed else None, "c": _le(rep.c) if rep.failed else None}
        if want_mask:
            out["mask"] = mask.raw[:self.info()["n_constraints"]]
        return out

    def check_vectors(self, dvec, count, stride=None, first=0, want_masks=False):
        """ug_r1cs_check_vectors: the `count` witnesses at elements first + v * stride of a device vector (stride None: n_wires)
        checked in one launch; a list of dicts as check() returns them (device_ms: the one launch's time, in every dict)"""
        info = self.info()
        rows = info["n_constraints"]
        stride = info["n_wires"] if stride is None else stride
        reps = (_R1csReport * max(count, 1))()
        masks = C.create_string_buffer(max(1, rows * count)) if want_masks else None
        _check(self.dev._L.ug_r1cs_check_vectors(self.h, dvec.h, first, stride, count, reps, masks))
        out = []
        for v in range(count):
            rep = reps[v]
            d = {"failed": rep.failed, "first": rep.first if rep.failed else None, "device_ms": rep.device_ms,
                 "a": _le(rep.a) if rep.failed else None, "b": _le(rep.b) if rep.failed else None, "c": _le(rep.c) if rep.failed else None}
            if want_masks:
                d["mask"] = masks.raw[v * rows:(v + 1) * rows]
            out.append(d)
        return out

    def match(self, hpoly, n_public):
        """ug_r1cs_match_hpoly: None when the .r1cs is the circuit of the zkey whose coefficient matrix `hpoly` holds, else
        (matrix, row) of the lowest differing row (matrix 0 = A, 1 = B)"""
        m, row = C.c_int(), C.c_uint64()
        _check(self.dev._L.ug_r1cs_match_hpoly(self.h, hpoly.h, n_public, C.byref(m), C.byref(row)))
        return None if m.value < 0 else (m.value, row.value)

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = None


def hpoly_vectors_bytes(domain, group):
    """ug_hpoly_vectors_bytes: what the H-polynomial workspaces for launch groups of `group` vectors take"""
    return load().ug_hpoly_vectors_bytes(domain, group)
