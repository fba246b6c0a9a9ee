// verifier_records.hpp -- what verifier_api.cpp uses of verifier_records.cpp: the points of a proof, the curve tests, and the packed
// proof records of include/verifier.h read into such points.
#pragma once
#include <cstdint>
#include <cstring>
#include "pairing.hpp"
#include "pairing_dev.hpp"

namespace ugv {
using namespace ug;
using namespace ug::pr;

// A, B and the one or two other G1 points of a proof: (C) or (pi_f, pi_r); g[1] is infinity for Groth16
struct Points { G1A a, g[2]; G2A b; };

inline G1A g1_inf() { return G1A{f1_zero(), f1_zero(), true}; }
inline bool g1_on_curve(const G1A& p) { return p.inf || p.y * p.y == p.x * p.x * p.x + f1_small(3); }
inline bool g2_on_curve(const G2A& q) {
    if (q.inf) return true;
    static const F2 b = f2_scale(f2_inv(F2{f1_small(9), f1_small(1)}), f1_small(3));     // 3 / (9 + u)
    return q.y * q.y == q.x * q.x * q.x + b;
}
inline void f1_to_plain(u32 out[8], const F1& a) { to_normal(out, a.v); }

constexpr bool known_format(int format) { return format == RECORDS_PLAIN || format == RECORDS_EVM || format == RECORDS_COMPRESSED; }
constexpr size_t record_bytes(bool ultra, int format = RECORDS_PLAIN) { return record_words(ultra ? 2 : 1, format) * sizeof(u32); }
const DecompressConsts& root_consts();

F1 f1_from_u256(const uint8_t* p);                                  // any 256-bit value, reduced mod q as f1_from_decimal reduces
void f1_to_le256(uint8_t* p, const F1& a);
// A whole record of `format`: pi_a | pi_b | the one or two other G1 points. false: a compressed x without a y on the curve; that point
// is then left at infinity. record_write is the way back, every coordinate reduced; false: a point off its curve has no compressed form.
bool record_read(int format, bool ultra, const uint8_t* rec, Points& pts);
bool record_write(int format, bool ultra, const Points& pts, uint8_t* rec);
bool record_read_pi_r(int format, const uint8_t* rec, G1A& pi_r);   // the last point of an UltraGroth record alone
// an input block of n_pub values in the byte order of `format` -> plain little-endian (EVM: every value byte-reversed); inline: once per input
inline void reverse32(uint8_t* out, const uint8_t* in) { for (int i = 0; i < 32; i++) out[i] = in[31 - i]; }
inline void inputs_to_plain(int format, const uint8_t* in, size_t n_pub, uint8_t* out) {
    if (format != RECORDS_EVM) { memmove(out, in, n_pub * 32); return; }
    for (size_t c = 0; c < n_pub; c++) { uint8_t t[32]; reverse32(t, in + c * 32); memcpy(out + c * 32, t, 32); }
}

}  // namespace ugv
