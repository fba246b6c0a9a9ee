// pairing.hpp -- the optimal-ate Miller loop of BN254 on F29 field elements, shared by the host verifier
// (verifier_api.cpp) and the batch-verification kernels (pairing.hip).
//
// Fq12 = Fq[w]/(w^12 - 18 w^6 + 82) as 12 coefficients (u = w^6 - 9), D-type twist (x, y) -> (x w^2, y w^3), Miller loop
// over 6t+2 with affine G2 steps and the two Frobenius lines at the end: the pairing restated from the definition, see the
// header comment of verifier_api.cpp. Every value is canonical ([0, q), device Montgomery form), so a result does not depend
// on where it was computed: the device's f equals the host's limb for limb.
//
// The small constants the formulas need (3, 9, 18, 82 and the Frobenius coefficients of the twist) travel in a
// PairingConsts: a kernel argument on the device, part of consts() on the host. The second half of a pairing -- the final
// exponentiation's is-one test -- adds the twelve gamma^k and the hard exponent: a FinalExpConsts, which the kernels that
// decide an equation take in its place.
#pragma once
#include "ec.hpp"

namespace ug {
namespace pr {

// ---- canonical field wrappers (always in [0, q), device Montgomery form) -------------------------------------------
struct F1 { Fq v; };
UG_HD F1 f1_zero() { return F1{fp_zero<FqParams>()}; }
UG_HD F1 f1_one() { return F1{canon(fp_one<FqParams>())}; }
// sums and differences of canonical values are below 2q, products of canonical values are strict and below 2q:
// one conditional subtraction restores [0, q)
UG_HD F1 operator+(const F1& a, const F1& b) { return F1{cond_sub_q(norm_strict(add(a.v, b.v)))}; }
UG_HD F1 operator-(const F1& a, const F1& b) { return F1{cond_sub_q(norm_strict(sub<1>(a.v, b.v)))}; }
UG_HD F1 operator*(const F1& a, const F1& b) { return F1{cond_sub_q(mul(a.v, b.v))}; }
UG_HD F1 operator-(const F1& a) { return F1{cond_sub_q(norm_strict(neg<1>(a.v)))}; }
UG_HD bool is0(const F1& a) { return limbs_all_zero(a.v); }
UG_HD bool operator==(const F1& a, const F1& b) {
    u32 o = 0;
    for (int i = 0; i < NL; i++) o |= a.v.l[i] ^ b.v.l[i];
    return o == 0;
}
UG_HD F1 f1_inv(const F1& a) { return F1{canon(inv(a.v))}; }
UG_HD F1 f1_small(u32 k) { u32 w[8] = {k, 0, 0, 0, 0, 0, 0, 0}; return F1{canon(from_normal<FqParams>(w))}; }

struct F2 { F1 a, b; };                                            // a + b u, u^2 = -1
UG_HD F2 f2_zero() { return F2{f1_zero(), f1_zero()}; }
UG_HD F2 operator+(const F2& x, const F2& y) { return F2{x.a + y.a, x.b + y.b}; }
UG_HD F2 operator-(const F2& x, const F2& y) { return F2{x.a - y.a, x.b - y.b}; }
UG_HD F2 operator-(const F2& x) { return F2{-x.a, -x.b}; }
UG_HD F2 operator*(const F2& x, const F2& y) { return F2{x.a * y.a - x.b * y.b, x.a * y.b + x.b * y.a}; }
UG_HD F2 f2_scale(const F2& x, const F1& k) { return F2{x.a * k, x.b * k}; }
UG_HD F2 f2_conj(const F2& x) { return F2{x.a, -x.b}; }
UG_HD bool is0(const F2& x) { return is0(x.a) && is0(x.b); }
UG_HD bool operator==(const F2& x, const F2& y) { return x.a == y.a && x.b == y.b; }
UG_HD F2 f2_inv(const F2& x) {
    F1 n = f1_inv(x.a * x.a + x.b * x.b);
    return F2{x.a * n, -(x.b * n)};
}

struct PairingConsts {
    F1 k3, k9, k18, k82;
    F2 g12, g13;           // xi^((p-1)/3), xi^((p-1)/2)
    F1 g22, g23;           // xi^((p^2-1)/3), xi^((p^2-1)/2) (both in Fq)
};

// (p^4 - p^2 + 1) / r, 761 bits, little-endian words
constexpr int HARD_BITS = 761;
struct FinalExpConsts : PairingConsts {
    F1 gamma[12];          // gamma^k, gamma = 82^((p-1)/6): the p^2 Frobenius maps w^k to gamma^k w^k
    u32 hard[24];
};

#if !defined(__HIP_DEVICE_COMPILE__)
// the constants on the host: a decimal literal -> value mod q
inline F1 f1_from_digits(const char* s) {
    const F1 ten = f1_small(10);
    F1 acc = f1_zero();
    for (; *s; s++) acc = acc * ten + f1_small((u32)(*s - '0'));
    return acc;
}
inline PairingConsts pairing_consts() {
    PairingConsts k;
    k.k3 = f1_small(3); k.k9 = f1_small(9); k.k18 = f1_small(18); k.k82 = f1_small(82);
    k.g12 = F2{f1_from_digits("21575463638280843010398324269430826099269044274347216827212613867836435027261"),
               f1_from_digits("10307601595873709700152284273816112264069230130616436755625194854815875713954")};
    k.g13 = F2{f1_from_digits("2821565182194536844548159561693502659359617185244120367078079554186484126554"),
               f1_from_digits("3505843767911556378687030309984248845540243509899259641013678093033130930403")};
    k.g22 = f1_from_digits("21888242871839275220042445260109153167277707414472061641714758635765020556616");
    k.g23 = f1_from_digits("21888242871839275222246405745257275088696311157297823662689037894645226208582");
    return k;
}
inline FinalExpConsts final_exp_consts() {
    static const u32 HARD_EXPONENT[24] = {
        0xccdf42b1u, 0xe81bb482u, 0xf49c36d4u, 0x5abf5cc4u, 0x1da014fdu, 0xf1154e7eu, 0x87cdbacfu, 0xdcc7b44cu,
        0x954bcf8au, 0xaaa441e3u, 0xd5095f23u, 0x6b887d56u, 0xf3fd90c6u, 0x79581e16u, 0xd189227du, 0x3b1b1355u,
        0x61876f6bu, 0x4e529a58u, 0xd5b12278u, 0x6c0eb522u, 0x83177fafu, 0x331ec151u, 0x0b0759adu, 0x01baaa71u};
    FinalExpConsts k;
    static_cast<PairingConsts&>(k) = pairing_consts();
    const F1 g = f1_from_digits("21888242871839275220042445260109153167277707414472061641714758635765020556617");
    k.gamma[0] = f1_one();
    for (int i = 1; i < 12; i++) k.gamma[i] = k.gamma[i - 1] * g;
    for (int i = 0; i < 24; i++) k.hard[i] = HARD_EXPONENT[i];
    return k;
}
#endif

// ---- Fq12, 12 coefficients in w ----------------------------------------------------------------------------------------
struct F12 { F1 c[12]; };
UG_HD F12 f12_one() { F12 r; for (int i = 0; i < 12; i++) r.c[i] = f1_zero(); r.c[0] = f1_one(); return r; }
// Products are accumulated lazily: up to 6 limb-column products of canonical operands share one Montgomery reduction
// ((6 * 9 + 9) * 2^58 < 2^64 per column; 6 q^2 / 2^261 + q < 2q for the value), so a full product costs 144 column
// products and ~40 reductions instead of 144 of each.
struct LazySum {
    u64 c[2 * NL];
    int terms;
    F1 total;
    UG_HD LazySum() : terms(0), total(f1_zero()) { cols_zero(c); }
    UG_HD void flush() {
        if (!terms) return;
        total = total + F1{cond_sub_q(redc<FqParams>(c))};
        cols_zero(c);
        terms = 0;
    }
    UG_HD void add(const F1& x, const F1& y) {
        if (terms == 6) flush();
#if defined(UG_CHECK_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
        // room for this product's 9 and the reduction's 9 column terms of (2^29 + 16)^2 each
        for (int k = 0; k < 2 * NL; k++)
            if (c[k] > ~(u64)0 - 18 * (((u64)1 << LB) + 16) * (((u64)1 << LB) + 16)) { fprintf(stderr, "UG_CHECK_BOUNDS: column overflow in LazySum\n"); abort(); }
        UG_BOUND(x.v, 1, "LazySum operand");
        UG_BOUND(y.v, 1, "LazySum operand");
#endif
        cols_mul(c, x.v, y.v);
        terms++;
    }
    UG_HD F1 value() { flush(); return total; }
};
// The loops over coefficients stay loops on the device (an Fq12 value is 108 words, three of them do not fit the register
// file beside a column sum): the values live in private memory, the 81 multiply-adds per 18 words read keep that cheap.
UG_HD F12 f12_reduce(const PairingConsts& kc, F1* t) {            // w^12 = 18 w^6 - 82
#pragma unroll 1
    for (int k = 22; k >= 12; k--) {
        if (is0(t[k])) continue;
        t[k - 6] = t[k - 6] + kc.k18 * t[k];
        t[k - 12] = t[k - 12] - kc.k82 * t[k];
    }
    F12 r;
    for (int i = 0; i < 12; i++) r.c[i] = t[i];
    return r;
}
UG_HD F12 f12_mul(const PairingConsts& kc, const F12& a, const F12& b) {
    bool za[12], zb[12];
    for (int i = 0; i < 12; i++) { za[i] = is0(a.c[i]); zb[i] = is0(b.c[i]); }
    F1 t[23];
#pragma unroll 1
    for (int k = 0; k < 23; k++) {
        LazySum sum;
#pragma unroll 1
        for (int i = (k > 11 ? k - 11 : 0); i <= (k < 11 ? k : 11); i++)
            if (!za[i] && !zb[k - i]) sum.add(a.c[i], b.c[k - i]);
        t[k] = sum.value();
    }
    return f12_reduce(kc, t);
}
UG_HD F12 f12_sqr(const PairingConsts& kc, const F12& a) {
    F1 t[23];
#pragma unroll 1
    for (int k = 0; k < 23; k++) {
        LazySum cross;                                              // sum over i < j, i + j = k  (at most 6 pairs)
#pragma unroll 1
        for (int i = (k > 11 ? k - 11 : 0); 2 * i < k; i++) cross.add(a.c[i], a.c[k - i]);
        F1 s = cross.value();
        t[k] = s + s;
        if (!(k & 1)) t[k] = t[k] + a.c[k >> 1] * a.c[k >> 1];
    }
    return f12_reduce(kc, t);
}
// (a + b u) w^k with u = w^6 - 9, added into f
UG_HD void f12_add_embedded(const PairingConsts& kc, F12& f, const F2& c, int k) {
    f.c[k] = f.c[k] + (c.a - kc.k9 * c.b);
    f.c[k + 6] = f.c[k + 6] + c.b;
}

// ---- curve points, affine with an infinity flag -----------------------------------------------------------------------
struct G1A { F1 x, y; bool inf; };
struct G2A { F2 x, y; bool inf; };

UG_HD G2A g2_inf() { return G2A{f2_zero(), f2_zero(), true}; }
// One Miller step: l = the line through the twist points r and t (the tangent when they are equal) evaluated at the G1
// point pt, then r <- r + t. Line and sum share the slope, so a step costs one Fq2 inversion.
UG_HD void miller_step(const PairingConsts& kc, G2A& r, const G2A& t, const G1A& pt, F12& l) {
    for (int i = 0; i < 12; i++) l.c[i] = f1_zero();
    F2 m = f2_zero();
    bool sloped = true, tangent = false;
    if (!(r.x == t.x)) m = (t.y - r.y) * f2_inv(t.x - r.x);
    else if (r.y == t.y && !is0(r.y)) { m = f2_scale(r.x * r.x, kc.k3) * f2_inv(r.y + r.y); tangent = true; }
    else sloped = false;
    if (sloped) {                                                   // -yP + (m xP) w + (y1 - m x1) w^3
        l.c[0] = -pt.y;
        f12_add_embedded(kc, l, f2_scale(m, pt.x), 1);
        f12_add_embedded(kc, l, r.y - m * r.x, 3);
    } else {                                                        // vertical: xP - x1 w^2
        l.c[0] = pt.x;
        f12_add_embedded(kc, l, -r.x, 2);
    }
    if (r.inf) { r = t; return; }
    if (t.inf) return;
    if (!sloped) { r = g2_inf(); return; }
    F2 x = tangent ? m * m - (r.x + r.x) : m * m - r.x - t.x;
    r = G2A{x, m * (r.x - x) - r.y, false};
}

constexpr u64 ATE_LOOP_LOW = 0x9d797039be763ba8ull;                 // 6 t + 2 = 2^64 + this = 29793968203157093288

// the Miller function f_{6t+2,Q}(P) times the two Frobenius lines; q and pt are not infinity
UG_HD F12 miller(const PairingConsts& kc, const G2A& q, const G1A& pt) {
    F12 f = f12_one();
    G2A r = q;
    const G2A q1{f2_conj(q.x) * kc.g12, f2_conj(q.y) * kc.g13, false};
    const G2A nq2{f2_scale(q.x, kc.g22), -f2_scale(q.y, kc.g23), false};
    // steps 2j and 2j + 1 are the doubling and the addition of bit 63 - j (bit 64 is the leading one), 128 and 129 the
    // Frobenius lines: one loop body, so that the device code holds each product once
#pragma unroll 1
    for (int s = 0; s < 130; s++) {
        const bool dbl = s < 128 && !(s & 1);
        if (s < 128 && (s & 1) && !((ATE_LOOP_LOW >> (63 - (s >> 1))) & 1)) continue;
        const G2A t = dbl ? r : s < 128 ? q : s == 128 ? q1 : nq2;
        F12 l;
        if (dbl) f = f12_sqr(kc, f);
        miller_step(kc, r, t, pt, l);
        f = f12_mul(kc, f, l);
    }
    return f;
}

// ---- final exponentiation: is f^((p^12 - 1)/r) one? --------------------------------------------------------------------
// With G = (f^(p^2) f)^((p^4 - p^2 + 1)/r) the full power equals conj(G)/G (conj = the p^6 Frobenius, w -> -w), which is 1
// exactly when G lies in Fq6, i.e. when its odd coefficients vanish: one 761-bit exponentiation, no Fq12 inversion.
UG_HD bool is0(const F12& f) {
    bool zero = true;
    for (int i = 0; i < 12; i++) zero = zero && is0(f.c[i]);
    return zero;
}
UG_HD F12 final_exp_hard(const FinalExpConsts& kc, const F12& f) {
    F12 base;
    for (int i = 0; i < 12; i++) base.c[i] = f.c[i] * kc.gamma[i];
    base = f12_mul(kc, base, f);
    F12 g = base;                                                   // bit HARD_BITS - 1, the leading one
#pragma unroll 1
    for (int i = HARD_BITS - 2; i >= 0; i--) {
        g = f12_sqr(kc, g);
        if ((kc.hard[i >> 5] >> (i & 31)) & 1) g = f12_mul(kc, g, base);
    }
    return g;
}
// g = G (zero for f = 0, which is not one)
UG_HD bool final_exp_is_one(const FinalExpConsts& kc, const F12& f, F12& g) {
    if (is0(f)) { g = f; return false; }
    g = final_exp_hard(kc, f);
    for (int i = 1; i < 12; i += 2) if (!is0(g.c[i])) return false;
    return true;
}

// ---- square roots and point decompression (the compressed records of include/verifier.h) ----------------------------------
// q = 3 mod 4, so a^((q + 1)/4) is a square root of a whenever a has one: a fixed-exponent power, squared once more to tell.
// Over u^2 = -1 the complex method takes it from there: the norm's root s, then (a.c0 +- s)/2 -- one of the two is a square
// when a is -- its root x0, and x1 = a.c1 / (2 x0). Every result is checked by squaring, and values are canonical, so the
// device and the host return the same limbs. IngestConsts are the curves' constant terms, what the ingest of plain records
// needs; DecompressConsts add 1/2, the exponent and the bound of the sign rule. Kernel arguments on the device, as PairingConsts.
constexpr int ROOT_BITS = 252;                                      // (q + 1) / 4
struct IngestConsts { F1 b1; F2 b2; };                              // 3 and 3 / (9 + u)
struct DecompressConsts : IngestConsts {
    F1 half;                                                        // 1 / 2
    u32 root_exp[8];                                                // (q + 1) / 4, little-endian words
    u32 half_q[8];                                                  // (q - 1) / 2: y is "the larger root" when y > (q - 1) / 2
};
// (host functions; plain inline so that the host code of pairing.hip may call them as well)
inline IngestConsts ingest_consts() { return IngestConsts{f1_small(3), f2_scale(f2_inv(F2{f1_small(9), f1_small(1)}), f1_small(3))}; }
inline DecompressConsts decompress_consts() {
    static const u32 ROOT_EXPONENT[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    static const u32 HALF_Q[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
    DecompressConsts c;
    static_cast<IngestConsts&>(c) = ingest_consts();
    c.half = f1_inv(f1_small(2));
    for (int i = 0; i < 8; i++) { c.root_exp[i] = ROOT_EXPONENT[i]; c.half_q[i] = HALF_Q[i]; }
    return c;
}
// root = a^((q + 1)/4); true when that is a square root of a (a = 0: root 0)
UG_HD bool f1_sqrt(const DecompressConsts& c, const F1& a, F1& root) {
    F1 r = a;                                                       // bit ROOT_BITS - 1, the leading one
#pragma unroll 1
    for (int i = ROOT_BITS - 2; i >= 0; i--) {
        r = r * r;
        if ((c.root_exp[i >> 5] >> (i & 31)) & 1) r = r * a;
    }
    root = r;
    return r * r == a;
}
// the sign rule of the compressed layout: y > -y as integers. Fq2 compares c1, and c0 when c1 is zero.
UG_HD bool f1_larger(const DecompressConsts& c, const F1& y) {
    u32 w[8];
    to_normal(w, y.v);
    for (int i = 7; i >= 0; i--) if (w[i] != c.half_q[i]) return w[i] > c.half_q[i];
    return false;
}
UG_HD bool f2_larger(const DecompressConsts& c, const F2& y) { return is0(y.b) ? f1_larger(c, y.a) : f1_larger(c, y.b); }
// a root of a in Fq2, or false when a is no square (root is then zero)
UG_HD bool f2_sqrt(const DecompressConsts& c, const F2& a, F2& root) {
    root = f2_zero();
    F1 s, x0;
    if (is0(a.b)) {                                                 // a in Fq: a real root, or an imaginary one since -1 is no square
        if (f1_sqrt(c, a.a, s)) { root.a = s; return true; }
        if (f1_sqrt(c, -a.a, s)) { root.b = s; return true; }
        return false;
    }
    if (!f1_sqrt(c, a.a * a.a + a.b * a.b, s)) return false;        // the norm is no square in Fq: a is none in Fq2
    if (!f1_sqrt(c, (a.a + s) * c.half, x0) && !f1_sqrt(c, (a.a - s) * c.half, x0)) return false;
    if (is0(x0)) return false;                                      // (x0 = 0 needs a.c1 = 0, handled above: never divide by it)
    const F2 r{x0, a.b * c.half * f1_inv(x0)};
    if (!(r * r == a)) return false;
    root = r;
    return true;
}
// y of the curve point with this x whose sign is `larger`; false when x^3 + b has no root
UG_HD bool g1_decompress(const DecompressConsts& c, const F1& x, bool larger, F1& y) {
    if (!f1_sqrt(c, x * x * x + c.b1, y)) return false;
    if (f1_larger(c, y) != larger) y = -y;
    return true;
}
UG_HD bool g2_decompress(const DecompressConsts& c, const F2& x, bool larger, F2& y) {
    if (!f2_sqrt(c, x * x * x + c.b2, y)) return false;
    if (f2_larger(c, y) != larger) y = -y;
    return true;
}

// ---- batch verification (verifier_api.cpp, pairing.hip) ----------------------------------------------------------------
// Records in memory: an Fq value is its 9 limbs; a G1 point 18 words (x, y; canonical; all zero = infinity), a G2 point 36
// (x.a, x.b, y.a, y.b), an XYZZ sum 36 (x, y, zz, zzz as ec.hpp leaves them), an Fq12 value 108.
constexpr int F12_WORDS = 12 * NL, G1_WORDS = 2 * NL, G2_WORDS = 4 * NL, XYZZ_WORDS = 4 * NL;

UG_HD F1 f1_load(const u32* p) { return F1{fp_from<FqParams>(p)}; }
UG_HD void fq_store(u32* p, const Fq& a) { for (int i = 0; i < NL; i++) p[i] = a.l[i]; }
UG_HD bool words_all_zero(const u32* p, int n) { u32 o = 0; for (int i = 0; i < n; i++) o |= p[i]; return o == 0; }
UG_HD void f12_load(F12& f, const u32* p) { for (int i = 0; i < 12; i++) f.c[i] = f1_load(p + i * NL); }
UG_HD void f12_store(u32* p, const F12& f) { for (int i = 0; i < 12; i++) fq_store(p + i * NL, f.c[i].v); }
UG_HD G1XYZZ xyzz_load(const u32* p) {
    G1XYZZ r;
    r.x = fp_from<FqParams>(p); r.y = fp_from<FqParams>(p + NL); r.zz = fp_from<FqParams>(p + 2 * NL); r.zzz = fp_from<FqParams>(p + 3 * NL);
    return r;
}
UG_HD void xyzz_store(u32* p, const G1XYZZ& v) { fq_store(p, v.x); fq_store(p + NL, v.y); fq_store(p + 2 * NL, v.zz); fq_store(p + 3 * NL, v.zzz); }

// One proof's leaves: f = miller(B, r A) (1 when a point of the pair is infinity, the rule of pairing_check) and r G_s for
// its k G1 points (C; or pi_f and pi_r). r is 128 bits, 4 words.
UG_HD void batch_leaf(const PairingConsts& kc, const u32* a, const u32* b, const u32* g, int k, const u32* r, u32* f_out, u32* g_out) {
    Fq ax = fp_zero<FqParams>(), ay = ax;
    bool a_live = false;
#pragma unroll 1
    for (int s = 0; s <= k; s++) {                                  // s = 0: A, s >= 1: the G1 points -- one copy of the ladder
        const u32* p = s ? g + (s - 1) * G1_WORDS : a;
        G1XYZZ acc = xyzz_inf<Fq>();
        if (!words_all_zero(p, G1_WORDS))
            acc = xyzz_mul_scalar(xyzz_from_affine(fp_from<FqParams>(p), fp_from<FqParams>(p + NL)), r, 128);
        if (s) xyzz_store(g_out + (s - 1) * XYZZ_WORDS, acc);
        else if (!is_inf(acc)) { xyzz_to_affine(ax, ay, acc); a_live = true; }
    }
    F12 f = f12_one();
    if (a_live && !words_all_zero(b, G2_WORDS)) {
        const G2A q{F2{f1_load(b), f1_load(b + NL)}, F2{f1_load(b + 2 * NL), f1_load(b + 3 * NL)}, false};
        f = miller(kc, q, G1A{F1{ax}, F1{ay}, false});
    }
    f12_store(f_out, f);
}

// ---- one proof's own equation (the judge of a rejected pass) -----------------------------------------------------------
UG_HD G1A g1_load(const u32* p, bool negate) {
    if (words_all_zero(p, G1_WORDS)) return G1A{f1_zero(), f1_zero(), true};
    const F1 y = f1_load(p + NL);
    return G1A{f1_load(p), negate ? -y : y, false};
}
UG_HD G2A g2_load(const u32* p) {
    if (words_all_zero(p, G2_WORDS)) return g2_inf();
    return G2A{F2{f1_load(p), f1_load(p + NL)}, F2{f1_load(p + 2 * NL), f1_load(p + 3 * NL)}, false};
}
// the rule of pairingCheck (src/groth16.cpp:679-681): a pair with a point at infinity is skipped
UG_HD bool pair_live(const G1A& p, const G2A& q) { return !p.inf && !q.inf; }

// column c of vkX: scalar * point as an XYZZ record; the scalar is a plain 256-bit integer, used as the single verifier's
// inputs_combination uses it (all 256 bits, no reduction beyond the parser's)
UG_HD void vkx_term(const u32* point, const u32* scalar, u32* out) {
    G1XYZZ acc = xyzz_inf<Fq>();
    if (!words_all_zero(point, G1_WORDS))
        acc = xyzz_mul_scalar(xyzz_from_affine(fp_from<FqParams>(point), fp_from<FqParams>(point + NL)), scalar, 256);
    xyzz_store(out, acc);
}
// -sum as an affine G1 record
UG_HD void vkx_finish(const G1XYZZ& sum, u32* out) {
    if (is_inf(sum)) { for (int i = 0; i < G1_WORDS; i++) out[i] = 0; return; }
    Fq x, y;
    xyzz_to_affine(x, y, sum);
    fq_store(out, x);
    fq_store(out + NL, (-F1{y}).v);
}
// e(A, B) e(-alpha, beta) e(-vkX, gamma) e(-G_s, delta_s) == 1 for one proof: a, b, its k points g as parsed, neg_vkx from
// vkx_finish, key_g2 = gamma, delta_0 [, delta_1], f_ab = miller(beta, -alpha) (one when that pair is skipped)
UG_HD bool judge_proof(const FinalExpConsts& kc, const u32* a, const u32* b, const u32* neg_vkx, const u32* g, int k, const u32* key_g2,
                       const u32* f_ab) {
    F12 acc;
    f12_load(acc, f_ab);
#pragma unroll 1
    for (int s = 0; s < k + 2; s++) {
        const G1A p = g1_load(s == 0 ? a : s == 1 ? neg_vkx : g + (s - 2) * G1_WORDS, s >= 2);
        const G2A q = g2_load(s == 0 ? b : key_g2 + (s - 1) * G2_WORDS);
        if (!pair_live(p, q)) continue;
        acc = f12_mul(kc, acc, miller(kc, q, p));
    }
    F12 hard;
    return final_exp_is_one(kc, acc, hard);
}

// ---- the ratio test of two G1 records (setup_host.hpp: Backend::ratio; pairing.hip: ratio_judge_kernel) ------------------
// A point of a zkey-format record: coordinates in Montgomery form with radix 2^256, 8 words each, all zero = infinity
UG_HD F1 record_coord(const u32* w) { return F1{cond_sub_q(from_mont256<FqParams>(w))}; }
UG_HD G1A g1_from_record(const u32* rec, bool negate) {
    if (words_all_zero(rec, 16)) return G1A{f1_zero(), f1_zero(), true};
    const F1 y = record_coord(rec + 8);
    return G1A{record_coord(rec), negate ? -y : y, false};
}
UG_HD G2A g2_from_record(const u32* rec) {
    if (words_all_zero(rec, 32)) return g2_inf();
    return G2A{F2{record_coord(rec), record_coord(rec + 8)}, F2{record_coord(rec + 16), record_coord(rec + 24)}, false};
}
// e(X, Q) e(-Y, G2) == 1 for the records x and y; q2: Q, then the generator of G2, G2_WORDS each, neither infinity. Both
// records infinity: holds; exactly one: does not, without a pairing. No random scalar: the answer is exact.
UG_HD bool ratio_holds(const FinalExpConsts& kc, const u32* x, const u32* y, const u32* q2) {
    if (words_all_zero(x, 16) || words_all_zero(y, 16)) return words_all_zero(x, 16) && words_all_zero(y, 16);
    F12 acc = f12_one();
#pragma unroll 1
    for (int s = 0; s < 2; s++)                                     // (one copy of the Miller loop, as in judge_proof)
        acc = f12_mul(kc, acc, miller(kc, g2_load(q2 + s * G2_WORDS), g1_from_record(s ? y : x, s == 1)));
    F12 hard;
    return final_exp_is_one(kc, acc, hard);
}

// a node of the product tree: the product of its two children, or the left one alone (right == nullptr: an odd last node)
UG_HD void f12_node(const PairingConsts& kc, const u32* left, const u32* right, u32* out) {
    F12 x;
    f12_load(x, left);
    if (right) { F12 y; f12_load(y, right); x = f12_mul(kc, x, y); }
    f12_store(out, x);
}
UG_HD void g1_node(const u32* left, const u32* right, u32* out) {
    G1XYZZ x = xyzz_load(left);
    if (right) x = xyzz_add(x, xyzz_load(right));
    xyzz_store(out, x);
}
// nodes of the whole tree over n leaves: level 0 has n, each level above half of the one below, rounded up, down to one root
inline size_t tree_nodes(size_t n) {
    size_t t = n;
    while (n > 1) { n = (n + 1) / 2; t += n; }
    return t;
}

}  // namespace pr
}  // namespace ug
