// verifier_records.cpp -- the packed proof records of include/verifier.h: the three layouts read into points and written from them,
// 256-bit integers as decimal strings, and the exported conversions (ug_proof_pack / _unpack / _record_convert, ug_inputs_*).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "json_min.hpp"
#include "verifier_records.hpp"
#include "../../include/verifier.h"

namespace ugv {

// A record is the proof.json whose decimal strings are its integers; these are the two directions of that sentence.
// The layouts (UG_RECORDS_*): plain little-endian coordinates, the big-endian EVM order with the imaginary half of an Fq2
// coordinate first, and compressed -- x and two flag bits per point. Every layout is read into the same points and written from
// them, so a conversion is a read and a write, and a record of any layout stands for the plain record it converts to.
static_assert((int)UG_RECORDS_PLAIN == (int)RECORDS_PLAIN && (int)UG_RECORDS_EVM == (int)RECORDS_EVM && (int)UG_RECORDS_COMPRESSED == (int)RECORDS_COMPRESSED, "layouts");
const DecompressConsts& root_consts() { static const DecompressConsts c = decompress_consts(); return c; }

namespace {
constexpr size_t g1_bytes(int format) { return format == RECORDS_COMPRESSED ? 32 : 64; }      // a G2 point takes twice that
// decimal string -> 256-bit integer, little-endian; false for anything but digits and for a value >= 2^256
bool u256_from_decimal(uint8_t out[32], const std::string& s) {
    if (s.empty()) return false;
    u32 w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        uint64_t carry = (uint64_t)(ch - '0');
        for (int k = 0; k < 8; k++) { const uint64_t v = (uint64_t)w[k] * 10 + carry; w[k] = (u32)v; carry = v >> 32; }
        if (carry) return false;
    }
    memcpy(out, w, 32);
    return true;
}
std::string u256_to_decimal(const uint8_t in[32]) {
    u32 w[8];
    memcpy(w, in, 32);
    std::vector<u32> chunks;                                        // base 10^9, lowest first
    u32 any;
    do {
        uint64_t rem = 0;
        any = 0;
        for (int k = 7; k >= 0; k--) { const uint64_t v = (rem << 32) | w[k]; w[k] = (u32)(v / 1000000000u); rem = v % 1000000000u; any |= w[k]; }
        chunks.push_back((u32)rem);
    } while (any);
    char buf[16];
    snprintf(buf, sizeof buf, "%u", chunks.back());
    std::string digits = buf;
    for (size_t c = chunks.size() - 1; c-- > 0;) { snprintf(buf, sizeof buf, "%09u", chunks[c]); digits += buf; }
    return digits;
}
}  // namespace

F1 f1_from_u256(const uint8_t* p) {
    u32 w[8];
    memcpy(w, p, 32);
    return F1{canon(from_normal<FqParams>(w))};
}
void f1_to_le256(uint8_t* p, const F1& a) {
    u32 w[8];
    f1_to_plain(w, a);
    memcpy(p, w, 32);
}

namespace {
F1 f1_from_layout(int format, const uint8_t* p) {                   // big-endian in the EVM layout
    if (format != RECORDS_EVM) return f1_from_u256(p);
    uint8_t le[32];
    reverse32(le, p);
    return f1_from_u256(le);
}
void f1_to_layout(int format, uint8_t* p, const F1& a) {
    uint8_t le[32];
    f1_to_le256(le, a);
    if (format == RECORDS_EVM) reverse32(p, le); else memcpy(p, le, 32);
}
// One point of a record in `format`. false: a compressed x without a y on the curve; the point is then left at infinity.
bool g1_from_layout(int format, const uint8_t* p, G1A& out) {
    if (format != RECORDS_COMPRESSED) {
        out = G1A{f1_from_layout(format, p), f1_from_layout(format, p + 32), false};
        out.inf = is0(out.x) && is0(out.y);
        return true;
    }
    uint8_t x[32];
    memcpy(x, p, 32);
    const bool inf = (x[31] & 0x40) != 0, larger = (x[31] & 0x80) != 0;
    x[31] &= 0x3f;
    out = g1_inf();
    if (inf) return true;
    const F1 xv = f1_from_u256(x);
    F1 y;
    if (!g1_decompress(root_consts(), xv, larger, y)) return false;
    out = G1A{xv, y, false};
    return true;
}
bool g2_from_layout(int format, const uint8_t* p, G2A& out) {
    if (format != RECORDS_COMPRESSED) {                             // EVM: x.c1, x.c0, y.c1, y.c0
        const size_t c0 = format == RECORDS_EVM ? 32 : 0, c1 = 32 - c0;
        out = G2A{F2{f1_from_layout(format, p + c0), f1_from_layout(format, p + c1)}, F2{f1_from_layout(format, p + 64 + c0), f1_from_layout(format, p + 64 + c1)}, false};
        out.inf = is0(out.x) && is0(out.y);
        return true;
    }
    uint8_t x1[32];
    memcpy(x1, p + 32, 32);
    const bool inf = (x1[31] & 0x40) != 0, larger = (x1[31] & 0x80) != 0;
    x1[31] &= 0x3f;
    out = g2_inf();
    if (inf) return true;
    const F2 xv{f1_from_u256(p), f1_from_u256(x1)};
    F2 y;
    if (!g2_decompress(root_consts(), xv, larger, y)) return false;
    out = G2A{xv, y, false};
    return true;
}
// ... and the way back, every coordinate reduced. false: a point off its curve has no compressed form (a sign bit cannot stand for it).
bool g1_to_layout(int format, const G1A& pt, uint8_t* p) {
    const bool compressed = format == RECORDS_COMPRESSED;
    memset(p, 0, g1_bytes(format));
    if (pt.inf) { if (compressed) p[31] = 0x40; return true; }
    if (compressed && !g1_on_curve(pt)) return false;
    f1_to_layout(format, p, pt.x);
    if (!compressed) f1_to_layout(format, p + 32, pt.y);
    else if (f1_larger(root_consts(), pt.y)) p[31] |= 0x80;
    return true;
}
bool g2_to_layout(int format, const G2A& q, uint8_t* p) {
    const bool compressed = format == RECORDS_COMPRESSED;
    const size_t c0 = format == RECORDS_EVM ? 32 : 0, c1 = 32 - c0;     // EVM: x.c1, x.c0, y.c1, y.c0
    memset(p, 0, 2 * g1_bytes(format));
    if (q.inf) { if (compressed) p[63] = 0x40; return true; }
    if (compressed && !g2_on_curve(q)) return false;
    f1_to_layout(format, p + c0, q.x.a); f1_to_layout(format, p + c1, q.x.b);
    if (!compressed) { f1_to_layout(format, p + 64 + c0, q.y.a); f1_to_layout(format, p + 64 + c1, q.y.b); }
    else if (f2_larger(root_consts(), q.y)) p[63] |= 0x80;
    return true;
}
}  // namespace

bool record_read_pi_r(int format, const uint8_t* rec, G1A& pi_r) { return g1_from_layout(format, rec + 4 * g1_bytes(format), pi_r); }
bool record_read(int format, bool ultra, const uint8_t* rec, Points& pts) {
    const size_t w = g1_bytes(format);
    pts.g[1] = g1_inf();
    bool ok = g1_from_layout(format, rec, pts.a);
    ok = g2_from_layout(format, rec + w, pts.b) && ok;
    ok = g1_from_layout(format, rec + 3 * w, pts.g[0]) && ok;
    if (ultra) ok = record_read_pi_r(format, rec, pts.g[1]) && ok;
    return ok;
}
bool record_write(int format, bool ultra, const Points& pts, uint8_t* rec) {
    const size_t w = g1_bytes(format);
    bool ok = g1_to_layout(format, pts.a, rec);
    ok = g2_to_layout(format, pts.b, rec + w) && ok;
    ok = g1_to_layout(format, pts.g[0], rec + 3 * w) && ok;
    if (ultra) ok = g1_to_layout(format, pts.g[1], rec + 4 * w) && ok;
    return ok;
}

namespace {
std::string record_to_json(bool ultra, const uint8_t* rec) {
    auto g1 = [&](size_t at) { return "[\"" + u256_to_decimal(rec + at) + "\",\"" + u256_to_decimal(rec + at + 32) + "\",\"1\"]"; };
    std::string t = "{\"pi_a\":" + g1(0) + ",\"pi_b\":[[\"" + u256_to_decimal(rec + 64) + "\",\"" + u256_to_decimal(rec + 96) + "\"],[\"" +
                    u256_to_decimal(rec + 128) + "\",\"" + u256_to_decimal(rec + 160) + "\"],[\"1\",\"0\"]],";
    if (ultra) t += "\"pi_f\":" + g1(192) + ",\"pi_r\":" + g1(256) + ",\"protocol\":\"ultragroth\"";
    else t += "\"pi_c\":" + g1(192) + ",\"protocol\":\"groth16\"";
    return t + ",\"curve\":\"bn128\"}";
}
std::string inputs_to_json(const uint8_t* in, size_t n_pub) {
    std::string t = "[";
    for (size_t c = 0; c < n_pub; c++) t += (c ? ",\"" : "\"") + u256_to_decimal(in + c * 32) + "\"";
    return t + "]";
}
int copy_text(const std::string& t, char* json, unsigned long maxsize) {
    if (!json || t.size() + 1 > maxsize) return 1;
    memcpy(json, t.c_str(), t.size() + 1);
    return 0;
}
}  // namespace

}  // namespace ugv

using namespace ugv;

extern "C" {

unsigned long ug_proof_record_bytes(int ultra, int format) { return known_format(format) ? (unsigned long)record_bytes(ultra != 0, format) : 0; }
int ug_proof_record_convert(int ultra, int from_format, const void* from, int to_format, void* to) {
    if (!from || !to || !known_format(from_format) || !known_format(to_format)) return 2;
    try {
        Points pts;
        uint8_t out[320];
        if (!record_read(from_format, ultra != 0, static_cast<const uint8_t*>(from), pts)) return 1;
        if (!record_write(to_format, ultra != 0, pts, out)) return 1;
        memcpy(to, out, record_bytes(ultra != 0, to_format));
        return 0;
    } catch (...) { return 2; }
}
int ug_inputs_convert(int from_format, const void* from, int n_pub, int to_format, void* to) {
    if (!from || !to || n_pub <= 0 || !known_format(from_format) || !known_format(to_format)) return 2;
    // one byte order to the other, or a copy: the block of a compressed record is the plain one
    inputs_to_plain((from_format == RECORDS_EVM) != (to_format == RECORDS_EVM) ? RECORDS_EVM : RECORDS_PLAIN,
                    static_cast<const uint8_t*>(from), (size_t)n_pub, static_cast<uint8_t*>(to));
    return 0;
}

int ug_proof_pack(int ultra, const char* proof_json, void* record) {
    if (!proof_json || !record) return 1;
    try {
        const JVal j = JParser(proof_json).parse_document();
        if (j.at("protocol").string() != (ultra ? "ultragroth" : "groth16")) return 1;
        uint8_t rec[320];
        bool ok = true;
        auto g1 = [&](const char* name, size_t at) {
            const JVal& v = j.at(name);
            ok = ok && u256_from_decimal(rec + at, v.at((size_t)0).string()) && u256_from_decimal(rec + at + 32, v.at((size_t)1).string());
        };
        g1("pi_a", 0);
        const JVal& b = j.at("pi_b");
        for (size_t c = 0; c < 4; c++) ok = ok && u256_from_decimal(rec + 64 + c * 32, b.at(c >> 1).at(c & 1).string());
        if (ultra) { g1("pi_f", 192); g1("pi_r", 256); } else g1("pi_c", 192);
        if (!ok) return 1;
        memcpy(record, rec, record_bytes(ultra != 0));
        return 0;
    } catch (...) { return 1; }
}
int ug_inputs_pack(const char* inputs_json, void* out, int n_pub) {
    if (!inputs_json || !out || n_pub <= 0) return 1;
    try {
        const JVal j = JParser(inputs_json).parse_document();
        if (j.type != JVal::Array || j.arr.size() != (size_t)n_pub) return 1;
        std::vector<uint8_t> buf((size_t)n_pub * 32);
        for (size_t c = 0; c < j.arr.size(); c++) if (!u256_from_decimal(&buf[c * 32], j.arr[c].string())) return 1;
        memcpy(out, buf.data(), buf.size());
        return 0;
    } catch (...) { return 1; }
}
int ug_proof_unpack(int ultra, const void* record, char* json, unsigned long maxsize) {
    if (!record) return 1;
    try { return copy_text(record_to_json(ultra != 0, static_cast<const uint8_t*>(record)), json, maxsize); } catch (...) { return 1; }
}
int ug_inputs_unpack(const void* in, int n_pub, char* json, unsigned long maxsize) {
    if (!in || n_pub <= 0) return 1;
    try { return copy_text(inputs_to_json(static_cast<const uint8_t*>(in), (size_t)n_pub), json, maxsize); } catch (...) { return 1; }
}

}  // extern "C"
