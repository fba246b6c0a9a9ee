"""Shared case builders of the NTT tests (test_ntt_cases.py checks them on the host against the CPU oracle, test_gpu_ntt_shapes.py
runs them on the device). Everything here is Python integers and numpy index arithmetic: no oracle, no library under test.

Conventions: n = 2^logn, omega = 5^((r-1)/n); forward X_k = sum_i x_i omega^(i k), inverse x_i = n^-1 sum_k X_k omega^(-i k). The
transform is linear, so the closed forms hold on the stored 256-bit words as they are (Montgomery values: x R with the SAME plain
omega); every expected word is canonical (< r).

  families        zero | constant c | delta c at place p | single frequency c omega^(-m i) | alternating (c, -c, ..) | geometric c g^i |
                  all r - 1, with c in {1, r - 1, 2^256 mod r}. Almost every intermediate value of a transform of these is a zero
                  residue -- which a lazily reduced butterfly carries as q, 2q or 3q -- and the results are zero in all but one place
                  (or in none: delta, geometric)
  twin            the same vector with r, 2r, 3r, 4r added to its words (all stay below 2^256): the transform must not notice
  spliced         uniform data below r with the field's edge values and unreduced words at the borders of the first pass's tile
  hpoly_*         a matrix of two records, whose H polynomial has a closed form

A dense expected vector is an index pattern into a cached table scale * omega^j (j < n), so a case costs one numpy gather."""
import functools
import struct

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R                       # the stored word of 1
C_VALUES = (1, R - 1, MONT)
FAMILIES = ("zero", "constant", "delta", "frequency", "alternating", "geometric", "all_r_minus_1")
G = pow(3, 0xC0FFEE, R)                     # ratio of the geometric family: of no 2-power order (asserted per size)
TILE = 1 << 10                              # the first pass of the device transform takes 2^10 consecutive elements
EDGES = (0, 1, 2, R - 1, R - 2, MONT, (1 << 255) % R)          # as _rand_elems of test_gpu_parity.py
UNREDUCED = (R, R + 1, 2 * R - 1, 3 * R, 4 * R + 5, 5 * R, (1 << 256) - 1, 1 << 255)


def omega(logn):
    return pow(5, (R - 1) >> logn, R)


def to_words(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def to_ints(data):
    return [int.from_bytes(data[k:k + 32], "little") for k in range(0, len(data), 32)]


def _rows(data):
    return np.frombuffer(data, dtype="V32")


# ------------------------------------------------------------------------------------------- tables
_TABLES = {}


def power_ints(logn, scale=1, inverse=False):
    """[scale * w^j for j < n], w = omega or its inverse"""
    w = omega(logn)
    if inverse:
        w = pow(w, -1, R)
    out, x = [], scale % R
    for _ in range(1 << logn):
        out.append(x)
        x = x * w % R
    return out


def scaled_powers(logn, scale):
    """numpy rows (V32) of scale * omega^j, j < n. The table of -scale is the same table turned by n / 2 (omega^(n/2) = -1)."""
    scale %= R
    key = (logn, scale)
    if key not in _TABLES:
        other = _TABLES.get((logn, R - scale)) if logn else None
        if other is not None:
            return np.roll(other, -(1 << (logn - 1)))
        _TABLES[key] = _rows(to_words(power_ints(logn, scale)))
    return _TABLES[key]


def forget_tables(keep_logn=None):
    """drop the cached tables (of every size but keep_logn): the large ones are 32 bytes per point each"""
    for key in [k for k in _TABLES if k[0] != keep_logn]:
        del _TABLES[key]
    for cached in (_inverse_denominators,):
        cached.cache_clear()


def _gather(logn, scale, step):
    """rows scale * omega^(step k) for k < n"""
    n = 1 << logn
    idx = (np.arange(n, dtype=np.int64) * (step % n)) % n
    return scaled_powers(logn, scale)[idx].tobytes()


def _one_place(logn, place, value):
    out = bytearray(32 << logn)
    out[32 * place:32 * place + 32] = (value % R).to_bytes(32, "little")
    return bytes(out)


# ------------------------------------------------------------------------------------------- families
class Case:
    """one input vector with its expected transform in both directions. expected(inverse) gives the bytes, or None for the
    geometric family, which geometric_holds checks multiplicatively."""

    def __init__(self, name, logn, c, data, forward=None, inverse=None):
        self.name, self.logn, self.c, self._data = name, logn, c, data
        self._forward, self._inverse = forward, inverse

    @property
    def data(self):
        """the input vector (built when asked for: a size's cases together would not fit a cache)"""
        return self._data() if callable(self._data) else self._data

    def expected(self, inverse):
        f = self._inverse if inverse else self._forward
        return f() if f is not None else None

    def holds(self, out, inverse, places=None):
        """out is the transform of the case: byte for byte where the expected vector is explicit, else through the product form"""
        exp = self.expected(inverse)
        if exp is not None:
            return out == exp
        return geometric_holds(out, self.logn, self.c, inverse, places)

    def __repr__(self):
        return "Case(%s, 2^%d)" % (self.name, self.logn)


def delta_places(logn):
    n = 1 << logn
    places = [0, 1, n // 2, n - 1]
    if logn > 10:
        places += [TILE - 1, TILE, n - TILE]
    return sorted(set(p for p in places if 0 <= p < n))


def frequencies(logn):
    n = 1 << logn
    m = [0, 1, n // 2, n - 1] + ([TILE] if n > TILE else [])
    return sorted(set(x for x in m if 0 <= x < n))


def _c_name(c):
    return {1: "1", R - 1: "r-1", MONT: "R"}.get(c, hex(c))


def family(logn, name, only_c=None):
    """the cases of one family at one size (logn >= 1); only_c: those of one value of c (zero has c = 0, all_r_minus_1 c = r - 1)"""
    assert logn >= 1 and name in FAMILIES
    if only_c is not None:
        return [case for case in family(logn, name) if case.c == only_c]
    n = 1 << logn
    ninv = pow(n, -1, R)
    zeros = bytes(32 * n)
    cases = []
    if name == "zero":
        cases.append(Case("zero", logn, 0, zeros, lambda: zeros, lambda: zeros))
    elif name in ("constant", "all_r_minus_1"):
        for c in (C_VALUES if name == "constant" else (R - 1,)):
            word = c.to_bytes(32, "little")
            cases.append(Case("%s(%s)" % (name, _c_name(c)), logn, c, word * n,
                              lambda c=c: _one_place(logn, 0, n * c), lambda c=c: _one_place(logn, 0, c)))
    elif name == "delta":
        for p in delta_places(logn):
            for c in C_VALUES:
                cases.append(Case("delta(%s at %d)" % (_c_name(c), p), logn, c, lambda c=c, p=p: _one_place(logn, p, c),
                                  lambda c=c, p=p: _gather(logn, c, p), lambda c=c, p=p: _gather(logn, c * ninv, -p)))
    elif name == "frequency":
        # x_i = c omega^(-m i): forward n c at k = m; inverse c at i = -m
        for m in frequencies(logn):
            for c in C_VALUES:
                cases.append(Case("frequency(%s, m = %d)" % (_c_name(c), m), logn, c, lambda c=c, m=m: _gather(logn, c, -m),
                                  lambda c=c, m=m: _one_place(logn, m, n * c), lambda c=c, m=m: _one_place(logn, (n - m) % n, c)))
    elif name == "alternating":
        for c in C_VALUES:
            pair = c.to_bytes(32, "little") + ((R - c) % R).to_bytes(32, "little")
            cases.append(Case("alternating(%s)" % _c_name(c), logn, c, pair * (n // 2),
                              lambda c=c: _one_place(logn, n // 2, n * c), lambda c=c: _one_place(logn, n // 2, c)))
    else:
        assert pow(G, n, R) != 1
        for c in C_VALUES:
            cases.append(Case("geometric(%s)" % _c_name(c), logn, c, lambda c=c: geometric_input(logn, c)))
    return cases


def all_cases(logn):
    return [case for name in FAMILIES for case in family(logn, name)]


@functools.lru_cache(maxsize=8)
def geometric_input(logn, c):
    out, x = [], c % R
    for _ in range(1 << logn):
        out.append(x.to_bytes(32, "little"))
        x = x * G % R
    return b"".join(out)


def sample_places(logn, seed=7):
    """every 64th place and 4096 random ones"""
    n = 1 << logn
    rng = np.random.Generator(np.random.PCG64(seed + logn))
    return sorted(set(range(0, n, 64)) | set(int(k) for k in rng.integers(0, n, size=4096)))


def geometric_holds(out, logn, c, inverse, places=None):
    """X_k (g omega^k - 1) == c (g^n - 1) and X_k < r at every place (or at `places`); inverse: omega^-1 and the right side / n.
    g omega^k != 1 for every k (g^n != 1), so the product form pins X_k down."""
    n = 1 << logn
    if len(out) != 32 * n:
        return False
    rhs = c * (pow(G, n, R) - 1) % R
    if inverse:
        rhs = rhs * pow(n, -1, R) % R
    w = omega(logn)
    if inverse:
        w = pow(w, -1, R)
    if places is None:
        gw = G
        for k in range(n):
            x = int.from_bytes(out[32 * k:32 * k + 32], "little")
            if x >= R or x * (gw - 1) % R != rhs:
                return False
            gw = gw * w % R
        return True
    for k in places:
        x = int.from_bytes(out[32 * k:32 * k + 32], "little")
        if x >= R or x * (G * pow(w, k, R) - 1) % R != rhs:
            return False
    return True


def definition_sum(data, logn, k, inverse=False):
    """output k straight from the definition: the O(n) sum"""
    n = 1 << logn
    w = pow(omega(logn), (-k if inverse else k) % n, R)
    acc, x = 0, 1
    for i in range(n):
        acc += int.from_bytes(data[32 * i:32 * i + 32], "little") * x
        x = x * w % R
    if inverse:
        acc *= pow(n, -1, R)
    return acc % R


# ------------------------------------------------------------------------------------------- unreduced words
_MULTIPLES = np.array([[(k * R >> (64 * l)) & ((1 << 64) - 1) for l in range(4)] for k in range(5)], dtype=np.uint64)


def add_multiples(data, ks):
    """word i of data plus ks[i] * r (ks in 0 .. 4), as 256-bit integers; asserts that no sum reaches 2^256"""
    a = np.frombuffer(data, dtype="<u8").reshape(-1, 4)
    ks = np.asarray(ks, dtype=np.int64)
    assert len(ks) == len(a) and ks.min() >= 0 and ks.max() <= 4
    period = 4 if len(a) % 4 == 0 and (ks.reshape(-1, 4) == ks[:4]).all() else 0       # (a pattern of period 4: no gather per word)
    out = np.empty_like(a)
    carry = np.zeros(len(a), dtype=np.uint64)
    for l in range(4):
        m = np.tile(_MULTIPLES[ks[:4], l], len(a) // 4) if period else _MULTIPLES[ks, l]
        s = a[:, l] + m
        c1 = s < m
        s2 = s + carry
        c2 = s2 < s
        out[:, l] = s2
        carry = (c1 | c2).astype(np.uint64)
    assert not carry.any()
    return out.tobytes()


def twin(data, shift=0):
    """the unreduced twin of a vector of words below r: r, 2r, 3r, 4r added in turn, beginning with (1 + shift mod 4) r. Every sum
    stays below 5 r < 2^256."""
    n = len(data) // 32
    return add_multiples(data, 1 + (np.arange(n, dtype=np.int64) + shift) % 4)


def reduce_words(data):
    return to_words(v % R for v in to_ints(data))


def splice_places(logn):
    """first and last element, both sides of the first tile's border, the middle"""
    n = 1 << logn
    return sorted(set(p for p in (0, 1, n // 2, TILE - 2, TILE - 1, TILE, TILE + 1, n - TILE - 1, n - TILE, n - 2, n - 1) if 0 <= p < n))


def spliced_random(logn, seed=5):
    """(data, reduced): uniform words below 2^252 from numpy with EDGES and UNREDUCED written over them at splice_places and at
    random places; `reduced` is the same vector mod r, word by word"""
    n = 1 << logn
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * logn))
    x = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    x[:, 3] &= np.uint64((1 << 60) - 1)
    data = bytearray(x.tobytes())
    special = EDGES + UNREDUCED
    places = splice_places(logn) + [int(p) for p in rng.integers(0, n, size=min(n, 3 * len(special)))]
    written = {}
    for t, p in enumerate(places):
        written[p] = special[(t + logn) % len(special)]
    for p, v in written.items():
        data[32 * p:32 * p + 32] = v.to_bytes(32, "little")
    reduced = bytearray(data)
    for p, v in written.items():
        reduced[32 * p:32 * p + 32] = (v % R).to_bytes(32, "little")
    return bytes(data), bytes(reduced)


# ------------------------------------------------------------------------------------------- H polynomial of two records
@functools.lru_cache(maxsize=2)
def _inverse_denominators(logn):
    """[1 / (omega_2n omega^j - 1) for j < n] by one batch inversion (omega_2n omega^j is no n-th root of unity: its n-th power
    is -1)"""
    n = 1 << logn
    w2n = omega(logn + 1)
    w = w2n * w2n % R
    d, x = [], w2n
    for _ in range(n):
        d.append((x - 1) % R)
        x = x * w % R
    prefix, acc = [], 1
    for v in d:
        prefix.append(acc)
        acc = acc * v % R
    inv = pow(acc, -1, R)
    out = [0] * n
    for j in range(n - 1, -1, -1):
        out[j] = inv * prefix[j] % R
        inv = inv * d[j] % R
    return out


def hpoly_records(ra, rb, s1, s2, alpha, beta):
    """the 44-byte records (A, row ra, signal s1, alpha) and (B, row rb, signal s2, beta): values stored times 2^512 mod r"""
    r2 = pow(2, 512, R)
    return (struct.pack("<III", 0, ra, s1) + (alpha * r2 % R).to_bytes(32, "little") +
            struct.pack("<III", 1, rb, s2) + (beta * r2 % R).to_bytes(32, "little"))


def hpoly_closed_form(logn, ra, rb, a, b):
    """h of the matrices with the single entries a in row ra of A and b in row rb of B (a = alpha w[s1], b = beta w[s2]), as the
    bytes of n plain integers. With E_k(v, row) = -2 v n^-1 / (omega_2n omega^(k - row) - 1), the coset evaluation of the
    polynomial that is v at omega^row and zero on the rest of the domain:
        h_k = E_k(a, ra) E_k(b, rb) - [ra == rb] E_k(a b, ra)"""
    n = 1 << logn
    inv = _inverse_denominators(logn)
    ninv = pow(n, -1, R)
    k2 = 4 * a * b * ninv * ninv % R
    k1 = -2 * a * b * ninv % R
    ia = inv[n - ra:] + inv[:n - ra] if ra else inv                 # ia[k] = inv[(k - ra) mod n]
    if ra == rb:
        return to_words(x * (k2 * x - k1) % R for x in ia)
    ib = inv[n - rb:] + inv[:n - rb] if rb else inv
    return to_words(k2 * x * y % R for x, y in zip(ia, ib))


HPOLY_WITNESS = (1, 7, R - 2, 12345678901234567890, 3, R - 1, MONT)
HPOLY_ALPHA, HPOLY_BETA = 5, R - 3


def hpoly_case(logn, ra, rb, s1=2, s2=3):
    """(records, record count, witness bytes, signal count, expected h) of a two-record matrix"""
    a = HPOLY_ALPHA * HPOLY_WITNESS[s1] % R
    b = HPOLY_BETA * HPOLY_WITNESS[s2] % R
    return (hpoly_records(ra, rb, s1, s2, HPOLY_ALPHA, HPOLY_BETA), 2, to_words(HPOLY_WITNESS), len(HPOLY_WITNESS),
            hpoly_closed_form(logn, ra, rb, a, b))
