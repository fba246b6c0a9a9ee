// verifier_api.cpp -- groth16_verify / ultra_groth_verify (include/verifier.h), host code.
//
// Replaces src/verifier.cpp (JSON front end, error strings, return codes) and the verifier halves of
// src/groth16.cpp:298-690 / src/ultra_groth.cpp:565-975, whose arithmetic (Fq6/Fq12 tower, G2, mulByScalar) lives in
// the absent ffiasm submodule. Verification is milliseconds of CPU work in the reference and stays on the host here:
// SURVEY.md section 8(f) lists it as the first row after the prover hot path. The checks are the reference's:
//     groth16:    vkX = IC[0] + sum_i input_i IC[i+1];   e(A,B) e(-alpha1,beta2) e(-vkX,gamma2) e(-C,delta2) == 1
//     ultragroth: vkX = IC[0] + sum_i input_i IC[i+1] + derive_challenge(pi_r) IC_rand;
//                 e(A,B) e(-alpha1,beta2) e(-vkX,gamma2) e(-pi_f,delta_c2_2) e(-pi_r,delta_c1_2) == 1
// Pairs with a point at infinity are skipped (pairingCheck, src/groth16.cpp:673-690).
//
// The pairing is restated from the definition, not from the reference's line functions: Fq12 = Fq[w]/(w^12 - 18 w^6 + 82)
// as 12 coefficients (u = w^6 - 9), D-type twist (x, y) -> (x w^2, y w^3), optimal-ate Miller loop over 6t+2 with affine
// G2 steps, the two Frobenius lines at the end. The result is a yes/no, so any correct pairing gives the reference's
// answer. Final exponentiation: with G = (f^(p^2) f)^((p^4 - p^2 + 1)/r) the full power f^((p^12-1)/r) equals
// conj(G)/G (conj = the p^6 Frobenius, w -> -w), which is 1 exactly when G lies in Fq6, i.e. when its odd coefficients
// vanish: one 761-bit exponentiation, no Fq12 inversion. Like the Miller loop it lives in pairing.hpp, compiled for the
// host here and for the device in pairing.hip.
#include <sys/random.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <future>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "ec.hpp"
#include "host_util.hpp"
#include "pairing.hpp"
#include "pairing_dev.hpp"
#include "../../include/ultragroth_hip.h"
#include "../../include/verifier.h"

using namespace ug;
using namespace ug::pr;
using ughost::keccak256;

namespace {

// ---- field wrappers, Fq12, G2 steps and the Miller loop: pairing.hpp (shared with the device) -------------------------
// decimal string -> value mod q (E.f1.fromString); anything but digits is an error
F1 f1_from_decimal(const std::string& s) {
    if (s.empty()) throw std::invalid_argument("not a number");
    const F1 ten = f1_small(10);
    F1 acc = f1_zero();
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw std::invalid_argument("not a number");
        acc = acc * ten + f1_small((u32)(ch - '0'));
    }
    return acc;
}
void f1_to_plain(u32 out[8], const F1& a) { to_normal(out, a.v); }

bool g1_on_curve(const G1A& p) { return p.inf || p.y * p.y == p.x * p.x * p.x + f1_small(3); }
bool g2_on_curve(const G2A& q) {
    if (q.inf) return true;
    static const F2 b = f2_scale(f2_inv(F2{f1_small(9), f1_small(1)}), f1_small(3));     // 3 / (9 + u)
    return q.y * q.y == q.x * q.x * q.x + b;
}

// the constants of the Miller loop and of the final exponentiation's is-one test (pairing.hpp, shared with the device)
const FinalExpConsts& consts() { static const FinalExpConsts c = final_exp_consts(); return c; }
bool final_exponentiation_is_one(const F12& f) {
    F12 hard;
    return final_exp_is_one(consts(), f, hard);
}

// the four / five Miller loops are independent: one host thread each
bool pairing_check(const std::vector<G1A>& a, const std::vector<G2A>& b) {
    std::vector<std::future<F12>> parts;
    for (size_t i = 0; i < a.size(); i++) {
        if (!pair_live(a[i], b[i])) continue;                       // src/groth16.cpp:679-681
        parts.push_back(std::async(std::launch::async, [&, i] { return miller(consts(), b[i], a[i]); }));
    }
    F12 acc = f12_one();
    for (auto& p : parts) acc = f12_mul(consts(), acc, p.get());
    return final_exponentiation_is_one(acc);
}

// ---- G1 arithmetic for vkX (ec.hpp, host) -------------------------------------------------------------------------------
G1XYZZ to_xyzz(const G1A& p) { return p.inf ? xyzz_inf<Fq>() : xyzz_from_affine(p.x.v, p.y.v); }
G1A from_xyzz(const G1XYZZ& p) {
    if (is_inf(p)) return G1A{f1_zero(), f1_zero(), true};
    Fq x, y;
    xyzz_to_affine(x, y, p);
    return G1A{F1{x}, F1{y}, false};
}
G1A g1_neg(const G1A& p) { return p.inf ? p : G1A{p.x, -p.y, false}; }

// ---- minimal JSON (objects, arrays, strings, numbers, literals): what nlohmann::json::parse accepts of it --------------
struct JVal {
    enum Type { Null, Bool, Number, String, Array, Object } type = Null;
    std::string str;                       // String: the text; Number: its literal
    bool integral = false;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal& at(const char* key) const {
        if (type != Object) throw std::invalid_argument("not an object");
        const JVal* hit = nullptr;
        for (const auto& kv : obj) if (kv.first == key) hit = &kv.second;          // later duplicates win, as nlohmann
        if (!hit) throw std::invalid_argument("missing key");
        return *hit;
    }
    const JVal& at(size_t i) const {
        if (type != Array || i >= arr.size()) throw std::invalid_argument("not an array element");
        return arr[i];
    }
    const std::string& string() const {
        if (type != String) throw std::invalid_argument("not a string");
        return str;
    }
};
struct JParser {
    const char* p;
    explicit JParser(const char* s) : p(s) {}
    void ws() { while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') p++; }
    [[noreturn]] void bad() { throw std::invalid_argument("malformed json"); }
    JVal parse_document() {
        JVal v = value(0);
        ws();
        if (*p) bad();
        return v;
    }
    JVal value(int depth) {
        if (depth > 64) bad();
        ws();
        JVal v;
        if (*p == '{') {
            v.type = JVal::Object; p++; ws();
            if (*p == '}') { p++; return v; }
            for (;;) {
                ws();
                if (*p != '"') bad();
                std::string key = string_literal();
                ws();
                if (*p != ':') bad();
                p++;
                v.obj.emplace_back(std::move(key), value(depth + 1));
                ws();
                if (*p == ',') { p++; continue; }
                if (*p == '}') { p++; return v; }
                bad();
            }
        }
        if (*p == '[') {
            v.type = JVal::Array; p++; ws();
            if (*p == ']') { p++; return v; }
            for (;;) {
                v.arr.push_back(value(depth + 1));
                ws();
                if (*p == ',') { p++; continue; }
                if (*p == ']') { p++; return v; }
                bad();
            }
        }
        if (*p == '"') { v.type = JVal::String; v.str = string_literal(); return v; }
        if (!strncmp(p, "true", 4)) { p += 4; v.type = JVal::Bool; return v; }
        if (!strncmp(p, "false", 5)) { p += 5; v.type = JVal::Bool; return v; }
        if (!strncmp(p, "null", 4)) { p += 4; return v; }
        if (*p == '-' || (*p >= '0' && *p <= '9')) {
            const char* s = p;
            if (*p == '-') p++;
            if (*p == '0') p++;
            else if (*p >= '1' && *p <= '9') while (*p >= '0' && *p <= '9') p++;
            else bad();
            v.integral = true;
            if (*p == '.') { v.integral = false; p++; if (*p < '0' || *p > '9') bad(); while (*p >= '0' && *p <= '9') p++; }
            if (*p == 'e' || *p == 'E') {
                v.integral = false; p++;
                if (*p == '+' || *p == '-') p++;
                if (*p < '0' || *p > '9') bad();
                while (*p >= '0' && *p <= '9') p++;
            }
            v.type = JVal::Number; v.str.assign(s, p);
            return v;
        }
        bad();
    }
    std::string string_literal() {
        std::string out;
        p++;                                                        // opening quote
        for (;;) {
            unsigned char ch = (unsigned char)*p;
            if (ch == 0 || ch < 0x20) bad();
            if (ch == '"') { p++; return out; }
            if (ch == '\\') {
                p++;
                switch (*p) {
                    case '"': out += '"'; break;   case '\\': out += '\\'; break; case '/': out += '/'; break;
                    case 'b': out += '\b'; break;  case 'f': out += '\f'; break;  case 'n': out += '\n'; break;
                    case 'r': out += '\r'; break;  case 't': out += '\t'; break;
                    case 'u': {
                        unsigned cp = 0;
                        for (int i = 1; i <= 4; i++) {
                            char h = p[i];
                            cp <<= 4;
                            if (h >= '0' && h <= '9') cp |= (unsigned)(h - '0');
                            else if (h >= 'a' && h <= 'f') cp |= (unsigned)(h - 'a' + 10);
                            else if (h >= 'A' && h <= 'F') cp |= (unsigned)(h - 'A' + 10);
                            else bad();
                        }
                        p += 4;
                        if (cp < 0x80) out += (char)cp;
                        else if (cp < 0x800) { out += (char)(0xc0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3f)); }
                        else { out += (char)(0xe0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3f)); out += (char)(0x80 | (cp & 0x3f)); }
                        break;
                    }
                    default: bad();
                }
                p++;
                continue;
            }
            out += (char)ch;
            p++;
        }
    }
};

// G1PointAffineFromJson / G2PointAffineFromJson (src/groth16.cpp:254-268): x and y only; (0, 0) is the point at infinity
G1A g1_from_json(const JVal& v) {
    G1A p{f1_from_decimal(v.at((size_t)0).string()), f1_from_decimal(v.at((size_t)1).string()), false};
    p.inf = is0(p.x) && is0(p.y);
    return p;
}
G2A g2_from_json(const JVal& v) {
    G2A q{F2{f1_from_decimal(v.at((size_t)0).at((size_t)0).string()), f1_from_decimal(v.at((size_t)0).at((size_t)1).string())},
          F2{f1_from_decimal(v.at((size_t)1).at((size_t)0).string()), f1_from_decimal(v.at((size_t)1).at((size_t)1).string())}, false};
    q.inf = is0(q.x) && is0(q.y);
    return q;
}

// decimal string -> value mod r as a plain 256-bit integer (E.fr.fromString, then fromMontgomery in verify())
void fr_plain_from_decimal(u32 out[8], const std::string& s) {
    if (s.empty()) throw std::invalid_argument("not a number");
    u32 ten[8] = {10, 0, 0, 0, 0, 0, 0, 0};
    const Fr t = from_normal<FrParams>(ten);
    Fr acc = fp_zero<FrParams>();
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw std::invalid_argument("not a number");
        u32 d[8] = {(u32)(ch - '0'), 0, 0, 0, 0, 0, 0, 0};
        acc = canon(add(canon(mul(acc, t)), from_normal<FrParams>(d)));
    }
    to_normal(out, acc);
}

struct Inputs { std::vector<std::vector<u32>> plain; };
Inputs parse_inputs(const char* text) {                             // src/verifier.cpp:59-86
    Inputs in;
    try {
        JVal j = JParser(text).parse_document();
        if (j.type != JVal::Array || j.arr.empty()) throw std::invalid_argument("invalid inputs data");
        for (const JVal& e : j.arr) {
            std::vector<u32> w(8);
            fr_plain_from_decimal(w.data(), e.string());
            in.plain.push_back(std::move(w));
        }
    } catch (...) { throw std::invalid_argument("invalid inputs data"); }
    return in;
}

struct Groth16Proof { G1A a, c; G2A b; };
struct Groth16Key { G1A alpha; G2A beta, gamma, delta; std::vector<G1A> ic; };
struct UltraProof { G1A a, final_commit, round_commit; G2A b; };
struct UltraKey { G1A alpha, ic_rand; G2A beta, gamma, final_delta, round_delta; std::vector<G1A> ic; };

Groth16Proof parse_proof(const char* text) {                        // :16-36
    try {
        JVal j = JParser(text).parse_document();
        if (j.at("protocol").string() != "groth16") throw std::invalid_argument("invalid proof data");
        return Groth16Proof{g1_from_json(j.at("pi_a")), g1_from_json(j.at("pi_c")), g2_from_json(j.at("pi_b"))};
    } catch (...) { throw std::invalid_argument("invalid proof data"); }
}
UltraProof parse_ultra_proof(const char* text) {                    // :38-57
    try {
        JVal j = JParser(text).parse_document();
        if (j.at("protocol").string() != "ultragroth") throw std::invalid_argument("invalid proof data");
        return UltraProof{g1_from_json(j.at("pi_a")), g1_from_json(j.at("pi_f")), g1_from_json(j.at("pi_r")), g2_from_json(j.at("pi_b"))};
    } catch (...) { throw std::invalid_argument("invalid proof data"); }
}
void check_key_header(const JVal& j, const char* protocol) {
    const JVal& np = j.at("nPublic");
    if (np.type != JVal::Number) throw std::invalid_argument("nPublic");
    if (j.at("protocol").string() != protocol || j.at("curve").string() != "bn128") throw std::invalid_argument("protocol");
}
std::vector<G1A> parse_ic(const JVal& j) {
    std::vector<G1A> ic;
    const JVal& a = j.at("IC");
    if (a.type == JVal::Array) for (const JVal& e : a.arr) ic.push_back(g1_from_json(e));
    else if (a.type == JVal::Object) for (const auto& kv : a.obj) ic.push_back(g1_from_json(kv.second));   // json::items()
    if (ic.empty()) throw std::invalid_argument("IC");
    return ic;
}
Groth16Key parse_key(const char* text) {                            // :88-116
    try {
        JVal j = JParser(text).parse_document();
        check_key_header(j, "groth16");
        Groth16Key k{g1_from_json(j.at("vk_alpha_1")), g2_from_json(j.at("vk_beta_2")), g2_from_json(j.at("vk_gamma_2")),
                     g2_from_json(j.at("vk_delta_2")), {}};
        k.ic = parse_ic(j);
        return k;
    } catch (...) { throw std::invalid_argument("invalid verification key data"); }
}
UltraKey parse_ultra_key(const char* text) {                        // :118-146, src/ultra_groth.cpp:543-563
    try {
        JVal j = JParser(text).parse_document();
        check_key_header(j, "ultragroth");
        UltraKey k{g1_from_json(j.at("vk_alpha_1")), {}, g2_from_json(j.at("vk_beta_2")), g2_from_json(j.at("vk_gamma_2")),
                   g2_from_json(j.at("vk_delta_c2_2")), g2_from_json(j.at("vk_delta_c1_2")), {}};
        k.ic = parse_ic(j);
        k.ic_rand = g1_from_json(j.at("IC_rand"));
        return k;
    } catch (...) { throw std::invalid_argument("invalid verification key data"); }
}

// sum_i input_i IC[i+1]  (the loops at src/groth16.cpp:322-332, src/ultra_groth.cpp:589-601)
G1XYZZ inputs_combination(const Inputs& in, const std::vector<G1A>& ic) {
    G1XYZZ acc = xyzz_inf<Fq>();
    for (size_t i = 0; i < in.plain.size(); i++) acc = xyzz_add(acc, xyzz_mul_scalar(to_xyzz(ic[i + 1]), in.plain[i].data(), 256));
    return acc;
}

// derive_challenge (src/ultra_groth.cpp:33-58): keccak256(x_BE32 || y_BE32) of the round commitment as a big-endian
// integer, reduced mod r; returned as a plain integer
void derive_challenge_plain(u32 out[8], const G1A& commit) {
    u32 x[8], y[8];
    f1_to_plain(x, commit.x); f1_to_plain(y, commit.y);
    uint8_t buf[64], ch[32];
    for (int i = 0; i < 32; i++) {
        buf[i] = (uint8_t)(x[7 - (i >> 2)] >> (24 - 8 * (i & 3)));
        buf[32 + i] = (uint8_t)(y[7 - (i >> 2)] >> (24 - 8 * (i & 3)));
    }
    keccak256(ch, buf, 64);
    u32 w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 32; i++) w[7 - (i >> 2)] |= (u32)ch[i] << (24 - 8 * (i & 3));
    to_normal(out, from_normal<FrParams>(w));                       // from_normal reduces values >= r
}

bool all_on_curve(std::initializer_list<const G1A*> g1, std::initializer_list<const G2A*> g2) {
    for (const G1A* p : g1) if (!g1_on_curve(*p)) return false;
    for (const G2A* q : g2) if (!g2_on_curve(*q)) return false;
    return true;
}

void copy_error(char* dst, unsigned long cap, const char* msg) {
    if (dst && cap) strncpy(dst, msg, cap);                         // as the reference: no terminator added beyond strncpy's
}

}  // namespace

extern "C" {

int groth16_verify(const char* proof, const char* inputs, const char* verification_key, char* error_msg,
                   unsigned long error_msg_maxsize) {
    try {
        if (!proof || !inputs || !verification_key) throw std::invalid_argument("null argument");
        Groth16Proof pr = parse_proof(proof);
        Inputs in = parse_inputs(inputs);
        Groth16Key key = parse_key(verification_key);
        if (in.plain.size() + 1 != key.ic.size()) throw std::invalid_argument("len(inputs)+1 != len(vk.IC)");     // src/groth16.cpp:318-320
        // points that are not on their curve can only come from malformed data: no pairing is defined for them
        if (!all_on_curve({&pr.a, &pr.c, &key.alpha}, {&pr.b, &key.beta, &key.gamma, &key.delta})) return VERIFIER_INVALID_PROOF;
        for (const G1A& p : key.ic) if (!g1_on_curve(p)) return VERIFIER_INVALID_PROOF;
        G1A vkx = from_xyzz(xyzz_add(inputs_combination(in, key.ic), to_xyzz(key.ic[0])));
        bool ok = pairing_check({pr.a, g1_neg(key.alpha), g1_neg(vkx), g1_neg(pr.c)}, {pr.b, key.beta, key.gamma, key.delta});
        return ok ? VERIFIER_VALID_PROOF : VERIFIER_INVALID_PROOF;
    } catch (std::exception& e) {
        copy_error(error_msg, error_msg_maxsize, e.what());
        return VERIFIER_ERROR;
    } catch (...) {
        copy_error(error_msg, error_msg_maxsize, "unknown error");
        return VERIFIER_ERROR;
    }
}

int ultra_groth_verify(const char* proof, const char* inputs, const char* verification_key, char* error_msg,
                       unsigned long error_msg_maxsize) {
    try {
        if (!proof || !inputs || !verification_key) throw std::invalid_argument("null argument");
        UltraProof pr = parse_ultra_proof(proof);
        Inputs in = parse_inputs(inputs);
        UltraKey key = parse_ultra_key(verification_key);
        if (in.plain.size() + 1 != key.ic.size()) throw std::invalid_argument("len(inputs) != len(vk.IC)");       // src/ultra_groth.cpp:585-587
        if (!all_on_curve({&pr.a, &pr.final_commit, &pr.round_commit, &key.alpha, &key.ic_rand},
                          {&pr.b, &key.beta, &key.gamma, &key.final_delta, &key.round_delta})) return VERIFIER_INVALID_PROOF;
        for (const G1A& p : key.ic) if (!g1_on_curve(p)) return VERIFIER_INVALID_PROOF;
        u32 rand[8];
        derive_challenge_plain(rand, pr.round_commit);                                                             // :603-609
        G1XYZZ vk = xyzz_add(inputs_combination(in, key.ic), to_xyzz(key.ic[0]));
        vk = xyzz_add(vk, xyzz_mul_scalar(to_xyzz(key.ic_rand), rand, 256));                                       // :609-612
        G1A vkx = from_xyzz(vk);
        bool ok = pairing_check({pr.a, g1_neg(key.alpha), g1_neg(vkx), g1_neg(pr.final_commit), g1_neg(pr.round_commit)},
                                {pr.b, key.beta, key.gamma, key.final_delta, key.round_delta});
        return ok ? VERIFIER_VALID_PROOF : VERIFIER_INVALID_PROOF;
    } catch (std::exception& e) {
        copy_error(error_msg, error_msg_maxsize, e.what());
        return VERIFIER_ERROR;
    } catch (...) {
        copy_error(error_msg, error_msg_maxsize, "unknown error");
        return VERIFIER_ERROR;
    }
}

}  // extern "C"

// ==== batch verification (include/verifier.h: ug_groth16_verify_batch, ug_ultra_groth_verify_batch) ======================
// Small-exponent batching. For proofs i under one key and random 128-bit r_i, the single equations raised to r_i multiply to
//     prod_i e(r_i A_i, B_i) * e(-S alpha, beta) * e(-vkX_S, gamma) * e(-sum r_i C_i, delta) == 1,     S = sum r_i,
//     vkX_S = S IC_0 + sum_j (sum_i r_i pub_ij) IC_{j+1}   (UltraGroth: + (sum_i r_i challenge_i) IC_rand, two G1 sums),
// which holds when every proof is valid and fails, except with probability 2^-128, when one is not. The per-proof Miller
// loop and the r_i multiples are the device pass (pairing.hip; pairing.hpp on host threads for device < 0); both come back as
// complete binary trees of partial products / sums, and the scalar sums are kept as prefix sums, so the same check can be
// made for the range of any tree node: a rejected batch is searched from the root down to nodes of at most LEAF proofs,
// which go to the single-proof verifier. Proofs whose B is outside the order-r subgroup never enter the batch (the pairing
// is not bilinear in the scalar there); the single verifier judges them, as it does every proof when the key itself has a
// point off its curve or a G2 point outside the subgroup.
//
// The proofs of a call are JSON texts or packed records (include/verifier.h), a `Source` either way. Records on a device take the
// resident path: the raw records are uploaded, reduced, checked and converted there (pairing.hip: records_ingest_kernel), and the
// host reads of them only what the prefix sums and the UltraGroth challenge need.
//
// The judge (ug_verify_batch_options.judge, ULTRAGROTH_VERIFY_JUDGE=1; off by default). The search above costs the host two
// batch checks per level and bad proof and a single verification per proof of a failing leaf node, so the sender of the proofs
// decides what a call costs. With the judge on, a rejected pass is searched breadth first only while its failing nodes number
// at most search_width; every proof under a failing node is then a suspect, as are the proofs whose B is outside the subgroup,
// and when the call has at least judge_min suspects they are decided by their own equations -- judge_proof of pairing.hpp, the
// single verifier's arithmetic -- one lane each in launches of up to 65536 (pairing.hip; host threads for device < 0).
namespace {

constexpr size_t LEAF = 16;
// The library's defaults, from the sweep of profiles/verify_judge.txt. A launch of the judge takes ~170 ms whether it holds 16 or
// 16384 suspects (one lane's latency), what the single verifier needs for ~256 proofs on 16 threads: below that the host is
// quicker. Every level the search opens costs up to 2 * width checks of ~7 ms before the same launch; width 2 is the smallest
// of the sweep that still follows ONE bad proof to its leaf, where judge on and off do the same work.
constexpr int DEFAULT_SEARCH_WIDTH = 2, DEFAULT_JUDGE_MIN = 256;

struct BatchOptions { bool judge = false; int search_width = DEFAULT_SEARCH_WIDTH, judge_min = DEFAULT_JUDGE_MIN; };

// ULTRAGROTH_VERIFY_JUDGE: unset, empty or 0 = off, 1 = on; anything else fails the call (a mistyped setting must not leave the
// judge off without a word, as ULTRAGROTH_VALIDATE)
bool judge_from_environment() {
    const char* e = getenv("ULTRAGROTH_VERIFY_JUDGE");
    if (!e || !e[0]) return false;
    if (e[1] || (e[0] != '0' && e[0] != '1')) throw std::invalid_argument(std::string("ULTRAGROTH_VERIFY_JUDGE must be 0 or 1, not \"") + e + "\"");
    return e[0] == '1';
}

template <class Fn> void parallel_for(size_t n, const Fn& fn) {
    const size_t threads = std::min<size_t>(n, std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())));
    if (threads <= 1) { for (size_t i = 0; i < n; i++) fn(i); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (size_t t = 0; t < threads; t++)
        pool.emplace_back([&] { for (size_t i = next++; i < n; i = next++) fn(i); });
    for (auto& t : pool) t.join();
}

struct BatchKey {
    bool ultra = false;
    G1A alpha, ic_rand;
    G2A beta, gamma, delta[2];             // delta[s] pairs with the proofs' G1 point s: (C) or (pi_f, pi_r)
    std::vector<G1A> ic;
    int k() const { return ultra ? 2 : 1; }
};
struct BatchProof {
    G1A a, g[2];
    G2A b;
    Inputs in;
    u32 challenge[8];
    bool no_point = false;                 // a compressed record whose x has no y on the curve: INVALID like a point off its curve
};
enum State { DONE, SINGLE, BATCH };

bool g2_in_subgroup(const G2A& q) {
    if (q.inf) return true;
    Fq2 x, y;
    x.a = q.x.a.v; x.b = q.x.b.v; y.a = q.y.a.v; y.b = q.y.b.v;
    return is_inf(xyzz_mul_scalar(xyzz_from_affine(x, y), FrParams::q32, 254));
}
void g1_words(u32* out, const G1A& p) {                            // all zero = infinity
    if (p.inf) { memset(out, 0, G1_WORDS * sizeof(u32)); return; }
    fq_store(out, p.x.v); fq_store(out + NL, p.y.v);
}
void g2_words(u32* out, const G2A& q) {
    if (q.inf) { memset(out, 0, G2_WORDS * sizeof(u32)); return; }
    fq_store(out, q.x.a.v); fq_store(out + NL, q.x.b.v); fq_store(out + 2 * NL, q.y.a.v); fq_store(out + 3 * NL, q.y.b.v);
}
Fr fr_from_plain(const u32* w8) { return canon(from_normal<FrParams>(w8)); }

struct BatchTrace {
    std::mutex m;
    double kernel_ms[3] = {0, 0, 0};       // the last device pass of the process: Miller kernel, Fq12 tree, G1 tree
    std::vector<int> index;                // ULTRAGROTH_TEST_HOOKS=1: the last call's batched proofs, their scalars and f_i
    std::vector<u32> r, f;
    double phase_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the last call: ug_verify_batch_phase_ms
    unsigned long long in_place = 0, gathered = 0;      // ... and its passes over packed records: arrays used in place / compacted first
} g_trace;

// one pass: the proofs idx[0..m) of the call, their trees and prefix sums
struct Pass {
    const BatchKey& key;
    size_t m, cols;
    int k;
    std::vector<u32> f_tree, g_tree;
    std::vector<Fr> prefix;                // (m + 1) x cols: S, t_0 .. t_{nPublic-1}, [t_rand]
    std::vector<size_t> level_off, level_size;
    unsigned long long checks = 0;

    Pass(const BatchKey& key_, size_t m_) : key(key_), m(m_), cols(key_.ic.size() + (key_.ultra ? 1 : 0)), k(key_.k()) {
        size_t off = 0;
        for (size_t n = m;; n = (n + 1) / 2) { level_off.push_back(off); level_size.push_back(n); off += n; if (n <= 1) break; }
        f_tree.resize(off * F12_WORDS);
        g_tree.resize(off * k * XYZZ_WORDS);
    }
    // the batch equation over the proofs of node j of `level`
    bool node_ok(size_t level, size_t j) {
        checks++;
        const size_t lo = j << level, hi = std::min(m, (j + 1) << level), node = level_off[level] + j;
        std::vector<std::vector<u32>> sc(cols, std::vector<u32>(8));
        for (size_t c = 0; c < cols; c++) to_normal(sc[c].data(), sub<1>(prefix[hi * cols + c], prefix[lo * cols + c]));
        std::vector<G1A> g1;
        std::vector<G2A> g2;
        g1.push_back(g1_neg(from_xyzz(xyzz_mul_scalar_w4(to_xyzz(key.alpha), sc[0].data()))));
        g2.push_back(key.beta);
        G1XYZZ vkx = xyzz_mul_scalar_w4(to_xyzz(key.ic[0]), sc[0].data());
        for (size_t c = 1; c < key.ic.size(); c++) vkx = xyzz_add(vkx, xyzz_mul_scalar_w4(to_xyzz(key.ic[c]), sc[c].data()));
        if (key.ultra) vkx = xyzz_add(vkx, xyzz_mul_scalar_w4(to_xyzz(key.ic_rand), sc[cols - 1].data()));
        g1.push_back(g1_neg(from_xyzz(vkx)));
        g2.push_back(key.gamma);
        for (int s = 0; s < k; s++) {
            g1.push_back(g1_neg(from_xyzz(xyzz_load(&g_tree[(node * k + s) * XYZZ_WORDS]))));
            g2.push_back(key.delta[s]);
        }
        std::vector<std::future<F12>> parts;
        for (size_t i = 0; i < g1.size(); i++) {
            if (g1[i].inf || g2[i].inf) continue;
            parts.push_back(std::async(std::launch::async, [&, i] { return miller(consts(), g2[i], g1[i]); }));
        }
        F12 acc;
        f12_load(acc, &f_tree[node * F12_WORDS]);
        for (auto& p : parts) acc = f12_mul(consts(), acc, p.get());
        return final_exponentiation_is_one(acc);
    }
    // node j of `level` failed: the positions (within the pass) that the single verifier has to judge
    void walk(size_t level, size_t j, std::vector<size_t>& suspects) {
        const size_t lo = j << level, hi = std::min(m, (j + 1) << level);
        if (hi - lo <= LEAF || level == 0) { for (size_t i = lo; i < hi; i++) suspects.push_back(i); return; }
        if (2 * j + 1 >= level_size[level - 1]) { walk(level - 1, 2 * j, suspects); return; }      // copied up: the same value
        for (size_t c = 2 * j; c <= 2 * j + 1; c++)
            if (!node_ok(level - 1, c)) walk(level - 1, c, suspects);
    }
    // Node j of `level` failed, judge on: breadth first while the failing nodes still cover more than LEAF proofs each and
    // number at most `width`. Every proof under a failing node is a suspect.
    void search(size_t level, size_t j, size_t width, std::vector<size_t>& suspects) {
        std::vector<size_t> failing{j};                            // all on `level`
        auto whole = [&](size_t node) { for (size_t i = node << level, hi = std::min(m, (node + 1) << level); i < hi; i++) suspects.push_back(i); };
        for (;;) {
            std::vector<size_t> open;                              // (only the last node of a level can be smaller than the others)
            for (size_t node : failing) {
                if (level == 0 || std::min(m, (node + 1) << level) - (node << level) <= LEAF) whole(node);
                else open.push_back(node);
            }
            if (open.size() > width) { for (size_t node : open) whole(node); return; }
            if (open.empty()) return;
            failing.clear();
            for (size_t node : open) {
                if (2 * node + 1 >= level_size[level - 1]) { failing.push_back(2 * node); continue; }      // copied up: the same value
                for (size_t c = 2 * node; c <= 2 * node + 1; c++)
                    if (!node_ok(level - 1, c)) failing.push_back(c);
            }
            level--;
        }
    }
    void host_trees(const u32* a, const u32* b, const u32* g, const u32* r) {
        const PairingConsts& kc = consts();
        parallel_for(m, [&](size_t i) {
            batch_leaf(kc, a + i * G1_WORDS, b + i * G2_WORDS, g + i * k * G1_WORDS, k, r + i * 4, &f_tree[i * F12_WORDS], &g_tree[i * k * XYZZ_WORDS]);
        });
        for (size_t l = 0; l + 1 < level_size.size(); l++) {
            const size_t n_src = level_size[l];
            const u32* fs = &f_tree[level_off[l] * F12_WORDS];
            const u32* gs = &g_tree[level_off[l] * k * XYZZ_WORDS];
            u32* fd = &f_tree[level_off[l + 1] * F12_WORDS];
            u32* gd = &g_tree[level_off[l + 1] * k * XYZZ_WORDS];
            parallel_for(level_size[l + 1], [&](size_t j) {
                const bool pair = 2 * j + 1 < n_src;
                f12_node(kc, fs + 2 * j * F12_WORDS, pair ? fs + (2 * j + 1) * F12_WORDS : nullptr, fd + j * F12_WORDS);
                for (int s = 0; s < k; s++)
                    g1_node(gs + (2 * j * k + s) * XYZZ_WORDS, pair ? gs + ((2 * j + 1) * k + s) * XYZZ_WORDS : nullptr, gd + (j * k + s) * XYZZ_WORDS);
            });
        }
    }
};

struct Ctx {                               // a device context for the subgroup check of the B points
    ug_ctx* c = nullptr;
    explicit Ctx(int device) { if (ug_ctx_create(&c, device) != UG_OK) throw std::runtime_error(ug_last_error()); }
    ~Ctx() { if (c) ug_ctx_destroy(c); }
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The suspects of a call, each decided by judge_proof: on `device` in launches of at most PAIRING_PASS, on host threads for
// device < 0. valid[s] answers suspect s.
void judge_suspects(const BatchKey& key, int device, const std::vector<const BatchProof*>& sus, std::vector<char>& valid,
                    ug_verify_batch_stats_ex& stats) {
    const size_t n = sus.size(), k = (size_t)key.k(), cols = key.ic.size() + (key.ultra ? 1 : 0);
    std::vector<u32> points(cols * G1_WORDS), key_g2((1 + k) * G2_WORDS), f_ab(F12_WORDS);
    for (size_t c = 0; c < key.ic.size(); c++) g1_words(&points[c * G1_WORDS], key.ic[c]);
    if (key.ultra) g1_words(&points[(cols - 1) * G1_WORDS], key.ic_rand);
    g2_words(&key_g2[0], key.gamma);
    for (size_t s = 0; s < k; s++) g2_words(&key_g2[(1 + s) * G2_WORDS], key.delta[s]);
    const G1A nalpha = g1_neg(key.alpha);
    f12_store(f_ab.data(), pair_live(nalpha, key.beta) ? miller(consts(), key.beta, nalpha) : f12_one());
    valid.assign(n, 0);
    for (size_t first = 0; first < n; first += PAIRING_PASS) {
        const size_t m = std::min<size_t>(PAIRING_PASS, n - first);
        std::vector<u32> a(m * G1_WORDS), b(m * G2_WORDS), g(m * k * G1_WORDS), scalars(m * cols * 8, 0), verdict(m, 0);
        parallel_for(m, [&](size_t i) {
            const BatchProof& p = *sus[first + i];
            g1_words(&a[i * G1_WORDS], p.a);
            g2_words(&b[i * G2_WORDS], p.b);
            for (size_t s = 0; s < k; s++) g1_words(&g[(i * k + s) * G1_WORDS], p.g[s]);
            u32* sc = &scalars[i * cols * 8];
            sc[0] = 1;                                              // IC_0 itself
            for (size_t c = 0; c < p.in.plain.size(); c++) memcpy(sc + (1 + c) * 8, p.in.plain[c].data(), 8 * sizeof(u32));
            if (key.ultra) memcpy(sc + (cols - 1) * 8, p.challenge, 8 * sizeof(u32));
        });
        if (device < 0) {
            parallel_for(m, [&](size_t i) {
                G1XYZZ sum = xyzz_inf<Fq>();
                u32 term[XYZZ_WORDS], nvkx[G1_WORDS];
                for (size_t c = 0; c < cols; c++) {
                    vkx_term(&points[c * G1_WORDS], &scalars[(i * cols + c) * 8], term);
                    sum = xyzz_add(sum, xyzz_load(term));
                }
                vkx_finish(sum, nvkx);
                verdict[i] = judge_proof(consts(), &a[i * G1_WORDS], &b[i * G2_WORDS], nvkx, &g[i * k * G1_WORDS], (int)k, key_g2.data(), f_ab.data());
            });
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            PairingJudge pj;
            pj.n = (int)m; pj.k = (int)k; pj.cols = (int)cols; pj.a = a.data(); pj.b = b.data(); pj.g = g.data(); pj.scalars = scalars.data();
            pj.points = points.data(); pj.key_g2 = key_g2.data(); pj.f_alpha_beta = f_ab.data(); pj.verdict = verdict.data();
            pairing_judge_device(device, consts(), pj);
            const double ms = ms_since(t0);
            stats.base.device_ms += ms;
            stats.judge_ms += ms;
            stats.judge_launches++;
        }
        for (size_t i = 0; i < m; i++) valid[first + i] = verdict[i] != 0;
    }
    stats.judged += n;
}

// ---- packed proof records (include/verifier.h) --------------------------------------------------------------------------------
// A record is the proof.json whose decimal strings are its integers; these are the two directions of that sentence.
// The layouts (UG_RECORDS_*): plain little-endian coordinates, the big-endian EVM order with the imaginary half of an Fq2
// coordinate first, and compressed -- x and two flag bits per point. Every layout is read into the same points and written from
// them, so a conversion is a read and a write, and a record of any layout stands for the plain record it converts to.
constexpr bool known_format(int format) { return format == RECORDS_PLAIN || format == RECORDS_EVM || format == RECORDS_COMPRESSED; }
constexpr size_t record_bytes(bool ultra, int format = RECORDS_PLAIN) { return record_words(ultra ? 2 : 1, format) * sizeof(u32); }
constexpr size_t g1_bytes(int format) { return format == RECORDS_COMPRESSED ? 32 : 64; }      // a G2 point takes twice that
static_assert((int)UG_RECORDS_PLAIN == (int)RECORDS_PLAIN && (int)UG_RECORDS_EVM == (int)RECORDS_EVM && (int)UG_RECORDS_COMPRESSED == (int)RECORDS_COMPRESSED, "layouts");
const DecompressConsts& root_consts() { static const DecompressConsts c = decompress_consts(); return c; }

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
F1 f1_from_u256(const uint8_t* p) {                                 // any 256-bit value, reduced mod q as f1_from_decimal reduces
    u32 w[8];
    memcpy(w, p, 32);
    return F1{canon(from_normal<FqParams>(w))};
}
G1A g1_from_record(const uint8_t* p) {
    G1A a{f1_from_u256(p), f1_from_u256(p + 32), false};
    a.inf = is0(a.x) && is0(a.y);
    return a;
}
G2A g2_from_record(const uint8_t* p) {
    G2A q{F2{f1_from_u256(p), f1_from_u256(p + 32)}, F2{f1_from_u256(p + 64), f1_from_u256(p + 96)}, false};
    q.inf = is0(q.x) && is0(q.y);
    return q;
}
void reverse32(uint8_t* out, const uint8_t* in) { for (int i = 0; i < 32; i++) out[i] = in[31 - i]; }
F1 f1_from_be256(const uint8_t* p) {
    uint8_t le[32];
    reverse32(le, p);
    return f1_from_u256(le);
}
void f1_to_le256(uint8_t* p, const F1& a) {
    u32 w[8];
    f1_to_plain(w, a);
    memcpy(p, w, 32);
}
void f1_to_be256(uint8_t* p, const F1& a) {
    uint8_t le[32];
    f1_to_le256(le, a);
    reverse32(p, le);
}
// One point of a record in `format`. false: a compressed x without a y on the curve; the point is then left at infinity.
bool g1_from_layout(int format, const uint8_t* p, G1A& out) {
    if (format == RECORDS_PLAIN) { out = g1_from_record(p); return true; }
    if (format == RECORDS_EVM) {
        out = G1A{f1_from_be256(p), f1_from_be256(p + 32), false};
        out.inf = is0(out.x) && is0(out.y);
        return true;
    }
    uint8_t x[32];
    memcpy(x, p, 32);
    const bool inf = (x[31] & 0x40) != 0, larger = (x[31] & 0x80) != 0;
    x[31] &= 0x3f;
    out = G1A{f1_zero(), f1_zero(), true};
    if (inf) return true;
    const F1 xv = f1_from_u256(x);
    F1 y;
    if (!g1_decompress(root_consts(), xv, larger, y)) return false;
    out = G1A{xv, y, false};
    return true;
}
bool g2_from_layout(int format, const uint8_t* p, G2A& out) {
    if (format == RECORDS_PLAIN) { out = g2_from_record(p); return true; }
    if (format == RECORDS_EVM) {                                    // x.c1, x.c0, y.c1, y.c0
        out = G2A{F2{f1_from_be256(p + 32), f1_from_be256(p)}, F2{f1_from_be256(p + 96), f1_from_be256(p + 64)}, false};
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
    memset(p, 0, g1_bytes(format));
    if (format == RECORDS_COMPRESSED) {
        if (pt.inf) { p[31] = 0x40; return true; }
        if (!g1_on_curve(pt)) return false;
        f1_to_le256(p, pt.x);
        if (f1_larger(root_consts(), pt.y)) p[31] |= 0x80;
        return true;
    }
    if (pt.inf) return true;
    if (format == RECORDS_EVM) { f1_to_be256(p, pt.x); f1_to_be256(p + 32, pt.y); }
    else { f1_to_le256(p, pt.x); f1_to_le256(p + 32, pt.y); }
    return true;
}
bool g2_to_layout(int format, const G2A& q, uint8_t* p) {
    memset(p, 0, 2 * g1_bytes(format));
    if (format == RECORDS_COMPRESSED) {
        if (q.inf) { p[63] = 0x40; return true; }
        if (!g2_on_curve(q)) return false;
        f1_to_le256(p, q.x.a); f1_to_le256(p + 32, q.x.b);
        if (f2_larger(root_consts(), q.y)) p[63] |= 0x80;
        return true;
    }
    if (q.inf) return true;
    if (format == RECORDS_EVM) { f1_to_be256(p, q.x.b); f1_to_be256(p + 32, q.x.a); f1_to_be256(p + 64, q.y.b); f1_to_be256(p + 96, q.y.a); }
    else { f1_to_le256(p, q.x.a); f1_to_le256(p + 32, q.x.b); f1_to_le256(p + 64, q.y.a); f1_to_le256(p + 96, q.y.b); }
    return true;
}
// a whole record: pi_a | pi_b | the one or two other G1 points. ok[0..3] say which of a, b, g[0], g[1] the record held.
struct RecordPoints { G1A a, g[2]; G2A b; bool ok[4]; };
bool record_read(int format, bool ultra, const uint8_t* rec, RecordPoints& pts) {
    const size_t w = g1_bytes(format);
    pts.g[1] = G1A{f1_zero(), f1_zero(), true};
    pts.ok[0] = g1_from_layout(format, rec, pts.a);
    pts.ok[1] = g2_from_layout(format, rec + w, pts.b);
    pts.ok[2] = g1_from_layout(format, rec + 3 * w, pts.g[0]);
    pts.ok[3] = !ultra || g1_from_layout(format, rec + 4 * w, pts.g[1]);
    return pts.ok[0] && pts.ok[1] && pts.ok[2] && pts.ok[3];
}
bool record_write(int format, bool ultra, const RecordPoints& pts, uint8_t* rec) {
    const size_t w = g1_bytes(format);
    bool ok = g1_to_layout(format, pts.a, rec);
    ok = g2_to_layout(format, pts.b, rec + w) && ok;
    ok = g1_to_layout(format, pts.g[0], rec + 3 * w) && ok;
    if (ultra) ok = g1_to_layout(format, pts.g[1], rec + 4 * w) && ok;
    return ok;
}
// an input block of n_pub values in the byte order of `format` -> plain little-endian (EVM: every value byte-reversed)
void inputs_to_plain(int format, const uint8_t* in, size_t n_pub, uint8_t* out) {
    if (format != RECORDS_EVM) { memmove(out, in, n_pub * 32); return; }
    for (size_t c = 0; c < n_pub; c++) { uint8_t t[32]; reverse32(t, in + c * 32); memcpy(out + c * 32, t, 32); }
}
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

// Where the proofs of a call come from: JSON texts or packed records. parse() is step 1 of the batch for proof i and throws what the
// single call would say; single() is the single-proof verifier on the same proof.
struct Source {
    bool ultra = false;
    virtual ~Source() {}
    // points = false: only what the host needs of a proof that stays on the device -- the inputs and the challenge
    virtual void parse(size_t i, BatchProof& p, size_t ic_size, bool points) const = 0;
    virtual int single(size_t i, const char* verification_key, char* msg, unsigned long cap) const = 0;
    virtual const uint8_t* raw() const { return nullptr; }          // packed records, for the device to ingest
    virtual int raw_format() const { return RECORDS_PLAIN; }        // ... and their layout
    virtual size_t inputs_per_proof() const { return 0; }           // records: the call's n_pub, the same for every proof
};
struct JsonSource : Source {
    const char* const* proofs = nullptr;
    const char* const* inputs = nullptr;
    void parse(size_t i, BatchProof& p, size_t ic_size, bool) const override {
        if (!proofs[i] || !inputs[i]) throw std::invalid_argument("null argument");
        if (ultra) { UltraProof u = parse_ultra_proof(proofs[i]); p.a = u.a; p.b = u.b; p.g[0] = u.final_commit; p.g[1] = u.round_commit; }
        else { Groth16Proof u = parse_proof(proofs[i]); p.a = u.a; p.b = u.b; p.g[0] = u.c; p.g[1] = G1A{f1_zero(), f1_zero(), true}; }
        p.in = parse_inputs(inputs[i]);
        if (p.in.plain.size() + 1 != ic_size) throw std::invalid_argument(ultra ? "len(inputs) != len(vk.IC)" : "len(inputs)+1 != len(vk.IC)");
    }
    int single(size_t i, const char* verification_key, char* msg, unsigned long cap) const override {
        return (ultra ? ultra_groth_verify : groth16_verify)(proofs[i], inputs[i], verification_key, msg, cap);
    }
};
struct RecordSource : Source {
    const uint8_t* records = nullptr;
    const uint8_t* inputs = nullptr;
    size_t n_pub = 0;
    int format = RECORDS_PLAIN;
    // points = false reads pi_r only (the challenge); not even that of a compressed record, whose pi_r the device's ingest leaves
    void parse(size_t i, BatchProof& p, size_t, bool points) const override {
        const uint8_t* rec = records + i * record_bytes(ultra, format);
        const size_t w = g1_bytes(format);
        bool held = true;
        p.g[1] = G1A{f1_zero(), f1_zero(), true};
        if (ultra && (points || format != RECORDS_COMPRESSED)) held = g1_from_layout(format, rec + 4 * w, p.g[1]);
        if (points) {
            held = g1_from_layout(format, rec, p.a) && held;
            held = g2_from_layout(format, rec + w, p.b) && held;
            held = g1_from_layout(format, rec + 3 * w, p.g[0]) && held;
        }
        p.no_point = !held;
        p.in.plain.assign(n_pub, std::vector<u32>(8));
        for (size_t c = 0; c < n_pub; c++) {                        // reduced mod r, as fr_plain_from_decimal
            uint8_t le[32];
            inputs_to_plain(format, inputs + (i * n_pub + c) * 32, 1, le);
            u32 v[8];
            memcpy(v, le, 32);
            to_normal(p.in.plain[c].data(), from_normal<FrParams>(v));
        }
    }
    int single(size_t i, const char* verification_key, char* msg, unsigned long cap) const override {
        const uint8_t* rec = records + i * record_bytes(ultra, format);
        const uint8_t* block = inputs + i * n_pub * 32;
        uint8_t plain[320];
        std::vector<uint8_t> plain_in;
        if (format != RECORDS_PLAIN) {                              // the plain record and block this one stands for
            RecordPoints pts;
            if (!record_read(format, ultra, rec, pts)) return VERIFIER_INVALID_PROOF;
            record_write(RECORDS_PLAIN, ultra, pts, plain);
            plain_in.resize(n_pub * 32);
            inputs_to_plain(format, block, n_pub, plain_in.data());
            rec = plain; block = plain_in.data();
        }
        const std::string proof = record_to_json(ultra, rec), in = inputs_to_json(block, n_pub);
        return (ultra ? ultra_groth_verify : groth16_verify)(proof.c_str(), in.c_str(), verification_key, msg, cap);
    }
    const uint8_t* raw() const override { return records; }
    int raw_format() const override { return format; }
    size_t inputs_per_proof() const override { return n_pub; }
};

int verify_batch(const Source& src, int device, int count, const char* verification_key,
                 int* verdicts, const BatchOptions& opt, ug_verify_batch_stats_ex* stats_out, char* error_msg, unsigned long error_msg_maxsize) {
    try {
        const auto t_start = std::chrono::steady_clock::now();
        const bool ultra = src.ultra;
        if (count < 0 || !verification_key || (count > 0 && !verdicts)) throw std::invalid_argument("null argument");
        ug_verify_batch_stats_ex stats_ex = {{0, 0, 0, 0.0, 0.0}, 0, 0, 0.0};
        ug_verify_batch_stats& stats = stats_ex.base;
        BatchKey key;
        key.ultra = ultra;
        if (ultra) {
            UltraKey k = parse_ultra_key(verification_key);
            key.alpha = k.alpha; key.ic_rand = k.ic_rand; key.beta = k.beta; key.gamma = k.gamma;
            key.delta[0] = k.final_delta; key.delta[1] = k.round_delta; key.ic = k.ic;
        } else {
            Groth16Key k = parse_key(verification_key);
            key.alpha = k.alpha; key.ic_rand = G1A{f1_zero(), f1_zero(), true}; key.beta = k.beta; key.gamma = k.gamma;
            key.delta[0] = k.delta; key.delta[1] = k.delta; key.ic = k.ic;
        }
        if (src.inputs_per_proof() && src.inputs_per_proof() + 1 != key.ic.size())      // (texts: checked per proof, in parse)
            throw std::invalid_argument(ultra ? "len(inputs) != len(vk.IC)" : "len(inputs)+1 != len(vk.IC)");
        double phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // where the call's time goes (ug_verify_batch_phase_ms)
        auto t_lap = t_start;
        auto lap = [&](int k) { const auto now = std::chrono::steady_clock::now(); phase[k] += std::chrono::duration<double, std::milli>(now - t_lap).count(); t_lap = now; };
        bool key_ok = g1_on_curve(key.alpha) && g1_on_curve(key.ic_rand);
        for (const G1A& p : key.ic) key_ok = key_ok && g1_on_curve(p);
        for (const G2A* q : {&key.beta, &key.gamma, &key.delta[0], &key.delta[1]}) key_ok = key_ok && g2_on_curve(*q) && g2_in_subgroup(*q);

        const size_t n = (size_t)count;
        std::vector<int> verdict(n, VERIFIER_ERROR);
        std::vector<State> state(n, key_ok ? BATCH : SINGLE);
        std::vector<BatchProof> parsed(key_ok ? n : 0);
        std::vector<std::string> message(n);
        const bool hooks = ughost::testHooksEnabled();
        if (hooks) { std::lock_guard<std::mutex> lock(g_trace.m); g_trace.index.clear(); g_trace.r.clear(); g_trace.f.clear(); g_trace.in_place = g_trace.gathered = 0; }
        // the scalars of a pass and the prefix sums of its proofs idx[0..m)
        auto draw_scalars = [&](Pass& pass, const size_t* idx, std::vector<u32>& r) {
            const size_t m = pass.m;
            r.resize(m * 4);
            for (size_t got = 0; got < r.size() * sizeof(u32);) {
                const ssize_t w = getrandom((uint8_t*)r.data() + got, r.size() * sizeof(u32) - got, 0);
                if (w <= 0) throw std::runtime_error("getrandom failed");
                got += (size_t)w;
            }
            for (size_t i = 0; i < m; i++) if (!(r[4 * i] | r[4 * i + 1] | r[4 * i + 2] | r[4 * i + 3])) r[4 * i] = 1;       // (2^-128)
            pass.prefix.assign((m + 1) * pass.cols, fp_zero<FrParams>());
            std::vector<Fr> term(m * pass.cols);
            parallel_for(m, [&](size_t i) {
                const BatchProof& p = parsed[idx[i]];
                const u32 rw[8] = {r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], 0, 0, 0, 0};
                const Fr rf = fr_from_plain(rw);
                Fr* t = &term[i * pass.cols];
                t[0] = rf;
                for (size_t c = 0; c < p.in.plain.size(); c++) t[1 + c] = canon(mul(rf, fr_from_plain(p.in.plain[c].data())));
                if (ultra) t[pass.cols - 1] = canon(mul(rf, fr_from_plain(p.challenge)));
            });
            for (size_t i = 0; i < m; i++)
                for (size_t c = 0; c < pass.cols; c++)
                    pass.prefix[(i + 1) * pass.cols + c] = canon(add(pass.prefix[i * pass.cols + c], term[i * pass.cols + c]));
        };
        // the trees of a pass are there: the root check, the search of a rejected pass, the verdicts
        auto settle = [&](Pass& pass, const size_t* idx, const std::vector<u32>& r) {
            const size_t m = pass.m;
            if (hooks) {
                std::lock_guard<std::mutex> lock(g_trace.m);
                for (size_t i = 0; i < m; i++) g_trace.index.push_back((int)idx[i]);
                g_trace.r.insert(g_trace.r.end(), r.begin(), r.end());
                g_trace.f.insert(g_trace.f.end(), pass.f_tree.begin(), pass.f_tree.begin() + m * F12_WORDS);
            }
            const size_t top = pass.level_size.size() - 1;
            std::vector<size_t> suspects;
            if (!pass.node_ok(top, 0)) {
                if (opt.judge) pass.search(top, 0, (size_t)opt.search_width, suspects);
                else pass.walk(top, 0, suspects);
            }
            for (size_t i = 0; i < m; i++) { verdict[idx[i]] = VERIFIER_VALID_PROOF; state[idx[i]] = DONE; }
            for (size_t s : suspects) state[idx[s]] = SINGLE;
            stats.batch_checks += pass.checks;
        };
        const bool resident = key_ok && device >= 0 && src.raw();
        lap(0);
        // 1. parse; what the single call would answer before any pairing is answered here
        if (key_ok && !resident) parallel_for(n, [&](size_t i) {
            state[i] = DONE;
            try {
                BatchProof& p = parsed[i];
                src.parse(i, p, key.ic.size(), true);
                if (p.no_point || !g1_on_curve(p.a) || !g1_on_curve(p.g[0]) || !g1_on_curve(p.g[1]) || !g2_on_curve(p.b)) { verdict[i] = VERIFIER_INVALID_PROOF; return; }
                if (ultra) derive_challenge_plain(p.challenge, p.g[1]);
                state[i] = BATCH;
            } catch (std::exception& e) { message[i] = e.what(); }
        });
        lap(1);
        // 2. B outside the subgroup: out of the batch
        std::vector<size_t> cand;
        if (!resident) for (size_t i = 0; i < n; i++) if (state[i] == BATCH) cand.push_back(i);
        if (device < 0) {
            parallel_for(cand.size(), [&](size_t c) { if (!g2_in_subgroup(parsed[cand[c]].b)) state[cand[c]] = SINGLE; });
        } else if (!cand.empty()) {
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<u32> rec(cand.size() * 32, 0);             // zkey records: Montgomery R = 2^256, all zero = infinity
            parallel_for(cand.size(), [&](size_t c) {
                const G2A& q = parsed[cand[c]].b;
                if (q.inf) return;
                to_mont256(&rec[c * 32], q.x.a.v); to_mont256(&rec[c * 32 + 8], q.x.b.v);
                to_mont256(&rec[c * 32 + 16], q.y.a.v); to_mont256(&rec[c * 32 + 24], q.y.b.v);
            });
            Ctx ctx(device);
            std::vector<uint8_t> reasons(cand.size(), UG_POINT_OK);            // one call answers for every point
            if (ug_points_check_mask(ctx.c, 1, rec.data(), cand.size(), 2, reasons.data()) != UG_OK) throw std::runtime_error(ug_last_error());
            for (size_t c = 0; c < cand.size(); c++) if (reasons[c] != UG_POINT_OK) state[cand[c]] = SINGLE;
            stats.device_ms += ms_since(t0);
        }
        std::vector<size_t> idx;
        for (size_t i : cand) { if (state[i] == BATCH) idx.push_back(i); else stats.off_subgroup++; }
        lap(2);
        // 3. the batch, in passes
        for (size_t first = 0; first < idx.size(); first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, idx.size() - first);
            Pass pass(key, m);
            const int k = pass.k;
            std::vector<u32> r, a(m * G1_WORDS), b(m * G2_WORDS), g(m * k * G1_WORDS);
            draw_scalars(pass, &idx[first], r);
            lap(3);
            parallel_for(m, [&](size_t i) {
                const BatchProof& p = parsed[idx[first + i]];
                g1_words(&a[i * G1_WORDS], p.a);
                g2_words(&b[i * G2_WORDS], p.b);
                for (int s = 0; s < k; s++) g1_words(&g[(i * k + s) * G1_WORDS], p.g[s]);
            });
            lap(4);
            if (device < 0) pass.host_trees(a.data(), b.data(), g.data(), r.data());
            else {
                const auto t0 = std::chrono::steady_clock::now();
                PairingBatch pb;
                pb.n = (int)m; pb.k = k; pb.a = a.data(); pb.b = b.data(); pb.g = g.data(); pb.r = r.data();
                pb.f_tree = pass.f_tree.data(); pb.g_tree = pass.g_tree.data();
                pairing_batch_device(device, consts(), pb);
                stats.device_ms += ms_since(t0);
                { std::lock_guard<std::mutex> lock(g_trace.m); for (int t = 0; t < 3; t++) g_trace.kernel_ms[t] = pb.kernel_ms[t]; }
            }
            lap(5);
            settle(pass, &idx[first], r);
            lap(6);
        }
        // 1-3 for packed records on a device, per pass of PAIRING_PASS records: the raw records cross PCIe once, the device reduces
        // and checks them and keeps the arrays of the Miller kernel; the host reads no coordinate of a proof that stays in the
        // batch (UltraGroth: pi_r, for the challenge). Off its curve: INVALID; pi_b off the subgroup: SINGLE, as in step 2.
        for (size_t first = 0; resident && first < n; first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, n - first);
            const int k = key.k(), format = src.raw_format();
            const bool late_challenge = ultra && format == RECORDS_COMPRESSED;     // pi_r.y is the device's to find: no host root per proof
            parallel_for(m, [&](size_t i) {
                BatchProof& p = parsed[first + i];
                src.parse(first + i, p, key.ic.size(), false);
                if (ultra && !late_challenge) derive_challenge_plain(p.challenge, p.g[1]);
            });
            lap(1);
            auto t0 = std::chrono::steady_clock::now();
            ResidentBatch rb(device, (int)m, k, format);
            std::vector<uint8_t> status(m);
            rb.ingest(src.raw() + first * record_bytes(ultra, format), status.data());
            if (late_challenge) {                                   // the rows of pi_r as the ingest decompressed them
                std::vector<u32> g(m * (size_t)k * G1_WORDS);
                rb.download(nullptr, nullptr, g.data());
                parallel_for(m, [&](size_t i) {
                    if (status[i] == UG_POINT_OFF_CURVE) return;
                    BatchProof& p = parsed[first + i];
                    p.g[1] = g1_load(&g[(i * k + 1) * G1_WORDS], false);
                    derive_challenge_plain(p.challenge, p.g[1]);
                });
            }
            stats.device_ms += ms_since(t0);
            std::vector<size_t> kept;
            std::vector<u32> keep;
            for (size_t i = 0; i < m; i++) {
                if (status[i] == UG_POINT_OK) { kept.push_back(first + i); keep.push_back((u32)i); state[first + i] = BATCH; }
                else if (status[i] == UG_POINT_OFF_SUBGROUP) { state[first + i] = SINGLE; stats.off_subgroup++; }
                else { state[first + i] = DONE; verdict[first + i] = VERIFIER_INVALID_PROOF; }
            }
            lap(2);
            if (kept.empty()) continue;
            Pass pass(key, kept.size());
            std::vector<u32> r;
            draw_scalars(pass, kept.data(), r);
            lap(3);
            t0 = std::chrono::steady_clock::now();
            double kernel_ms[3];
            rb.run(consts(), kept.size() == m ? nullptr : keep.data(), (int)kept.size(), r.data(), pass.f_tree.data(), pass.g_tree.data(), kernel_ms);
            stats.device_ms += ms_since(t0);
            {
                std::lock_guard<std::mutex> lock(g_trace.m);
                for (int t = 0; t < 3; t++) g_trace.kernel_ms[t] = kernel_ms[t];
                if (hooks) (kept.size() == m ? g_trace.in_place : g_trace.gathered)++;
            }
            lap(5);
            settle(pass, kept.data(), r);
            lap(6);
        }
        // 4. whatever is left: to the judge when it is on and the suspects are many enough (never under a key the batch refused),
        //    else to the single verifier on the host threads
        std::vector<size_t> singles;
        for (size_t i = 0; i < n; i++) if (state[i] == SINGLE) singles.push_back(i);
        if (opt.judge && key_ok && !singles.empty() && singles.size() >= (size_t)opt.judge_min) {
            if (resident) parallel_for(singles.size(), [&](size_t s) { src.parse(singles[s], parsed[singles[s]], key.ic.size(), true); });   // rebuilt from the raw records
            std::vector<const BatchProof*> sus;
            for (size_t i : singles) sus.push_back(&parsed[i]);
            std::vector<char> valid;
            judge_suspects(key, device, sus, valid, stats_ex);
            for (size_t s = 0; s < singles.size(); s++) verdict[singles[s]] = valid[s] ? VERIFIER_VALID_PROOF : VERIFIER_INVALID_PROOF;
            singles.clear();
        }
        parallel_for(singles.size(), [&](size_t s) {
            const size_t i = singles[s];
            char msg[256] = {0};
            verdict[i] = src.single(i, verification_key, msg, sizeof msg - 1);
            if (verdict[i] == VERIFIER_ERROR) message[i] = msg;
        });
        stats.single_checks = singles.size();
        lap(7);
        { std::lock_guard<std::mutex> lock(g_trace.m); for (int k = 0; k < 8; k++) g_trace.phase_ms[k] = phase[k]; }
        int rc = VERIFIER_VALID_PROOF;
        for (size_t i = 0; i < n; i++) {
            verdicts[i] = verdict[i];
            if (verdict[i] != VERIFIER_VALID_PROOF && rc == VERIFIER_VALID_PROOF) {
                rc = VERIFIER_INVALID_PROOF;
                char text[320];
                snprintf(text, sizeof text, "proof %zu: %s", i, verdict[i] == VERIFIER_ERROR ? message[i].c_str() : "invalid proof");
                copy_error(error_msg, error_msg_maxsize, text);
            }
        }
        stats.host_ms = ms_since(t_start) - stats.device_ms;
        if (stats_out) *stats_out = stats_ex;
        return rc;
    } catch (std::exception& e) {
        copy_error(error_msg, error_msg_maxsize, e.what());
        return VERIFIER_ERROR;
    } catch (...) {
        copy_error(error_msg, error_msg_maxsize, "unknown error");
        return VERIFIER_ERROR;
    }
}

}  // namespace

extern "C" {

// the JSON calls: null arrays fail the call as a null key does
static int verify_batch_json(bool ultra, int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                             int* verdicts, const BatchOptions& opt, ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    if (count > 0 && (!proofs || !inputs)) { copy_error(error_msg, error_msg_maxsize, "null argument"); return VERIFIER_ERROR; }
    JsonSource src;
    src.ultra = ultra; src.proofs = proofs; src.inputs = inputs;
    return verify_batch(src, device, count, verification_key, verdicts, opt, stats, error_msg, error_msg_maxsize);
}
// the existing calls: options from the environment, the 40-byte stats
static int verify_batch_env(bool ultra, int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                            int* verdicts, ug_verify_batch_stats* stats, char* error_msg, unsigned long error_msg_maxsize) {
    BatchOptions opt;
    try { opt.judge = judge_from_environment(); }
    catch (std::exception& e) { copy_error(error_msg, error_msg_maxsize, e.what()); return VERIFIER_ERROR; }
    ug_verify_batch_stats_ex ex;
    const int rc = verify_batch_json(ultra, device, count, proofs, inputs, verification_key, verdicts, opt, stats ? &ex : nullptr, error_msg, error_msg_maxsize);
    if (stats && rc != VERIFIER_ERROR) *stats = ex.base;
    return rc;
}
static bool read_options(BatchOptions& opt, const ug_verify_batch_options* options, char* error_msg, unsigned long error_msg_maxsize) {
    try {
        if (!options) opt.judge = judge_from_environment();
        else {
            if (options->size < sizeof(ug_verify_batch_options)) throw std::invalid_argument("ug_verify_batch_options: size is smaller than the struct");
            if (options->judge != 0 && options->judge != 1) throw std::invalid_argument("ug_verify_batch_options: judge must be 0 or 1");
            opt.judge = options->judge == 1;
            if (options->search_width >= 0) opt.search_width = options->search_width;
            if (options->judge_min >= 0) opt.judge_min = options->judge_min;
        }
        return true;
    } catch (std::exception& e) { copy_error(error_msg, error_msg_maxsize, e.what()); return false; }
}
static int verify_batch_opt(bool ultra, int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                            int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                            unsigned long error_msg_maxsize) {
    BatchOptions opt;
    if (!read_options(opt, options, error_msg, error_msg_maxsize)) return VERIFIER_ERROR;
    return verify_batch_json(ultra, device, count, proofs, inputs, verification_key, verdicts, opt, stats, error_msg, error_msg_maxsize);
}
static int verify_batch_records(bool ultra, int device, int format, int count, const void* records, const void* inputs, int n_pub,
                                const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                                ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    BatchOptions opt;
    if (!read_options(opt, options, error_msg, error_msg_maxsize)) return VERIFIER_ERROR;
    if (!known_format(format)) { copy_error(error_msg, error_msg_maxsize, "format: not one of UG_RECORDS_PLAIN, UG_RECORDS_EVM, UG_RECORDS_COMPRESSED"); return VERIFIER_ERROR; }
    if (count < 0 || !verification_key || (count > 0 && (!records || !inputs || !verdicts))) { copy_error(error_msg, error_msg_maxsize, "null argument"); return VERIFIER_ERROR; }
    if (n_pub <= 0) { copy_error(error_msg, error_msg_maxsize, "invalid inputs data"); return VERIFIER_ERROR; }
    RecordSource src;
    src.ultra = ultra; src.records = static_cast<const uint8_t*>(records); src.inputs = static_cast<const uint8_t*>(inputs); src.n_pub = (size_t)n_pub;
    src.format = format;
    return verify_batch(src, device, count, verification_key, verdicts, opt, stats, error_msg, error_msg_maxsize);
}

int ug_groth16_verify_batch(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                            int* verdicts, ug_verify_batch_stats* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return verify_batch_env(false, device, count, proofs, inputs, verification_key, verdicts, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                int* verdicts, ug_verify_batch_stats* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return verify_batch_env(true, device, count, proofs, inputs, verification_key, verdicts, stats, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_opt(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                unsigned long error_msg_maxsize) {
    return verify_batch_opt(false, device, count, proofs, inputs, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_opt(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                    int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                    unsigned long error_msg_maxsize) {
    return verify_batch_opt(true, device, count, proofs, inputs, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}

int ug_groth16_verify_batch_records(int device, int count, const void* records, const void* inputs, int n_pub, const char* verification_key,
                                    int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                    unsigned long error_msg_maxsize) {
    return verify_batch_records(false, device, RECORDS_PLAIN, count, records, inputs, n_pub, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_records(int device, int count, const void* records, const void* inputs, int n_pub, const char* verification_key,
                                        int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                        unsigned long error_msg_maxsize) {
    return verify_batch_records(true, device, RECORDS_PLAIN, count, records, inputs, n_pub, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_records_fmt(int device, int format, int count, const void* records, const void* inputs, int n_pub,
                                        const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                                        ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return verify_batch_records(false, device, format, count, records, inputs, n_pub, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_records_fmt(int device, int format, int count, const void* records, const void* inputs, int n_pub,
                                            const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                                            ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return verify_batch_records(true, device, format, count, records, inputs, n_pub, verification_key, verdicts, options, stats, error_msg, error_msg_maxsize);
}

unsigned long ug_proof_record_bytes(int ultra, int format) { return known_format(format) ? (unsigned long)record_bytes(ultra != 0, format) : 0; }
int ug_proof_record_convert(int ultra, int from_format, const void* from, int to_format, void* to) {
    if (!from || !to || !known_format(from_format) || !known_format(to_format)) return 2;
    try {
        RecordPoints pts;
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
static int copy_text(const std::string& t, char* json, unsigned long maxsize) {
    if (!json || t.size() + 1 > maxsize) return 1;
    memcpy(json, t.c_str(), t.size() + 1);
    return 0;
}
int ug_proof_unpack(int ultra, const void* record, char* json, unsigned long maxsize) {
    if (!record) return 1;
    try { return copy_text(record_to_json(ultra != 0, static_cast<const uint8_t*>(record)), json, maxsize); } catch (...) { return 1; }
}
int ug_inputs_unpack(const void* in, int n_pub, char* json, unsigned long maxsize) {
    if (!in || n_pub <= 0) return 1;
    try { return copy_text(inputs_to_json(static_cast<const uint8_t*>(in), (size_t)n_pub), json, maxsize); } catch (...) { return 1; }
}

// ULTRAGROTH_TEST_HOOKS=1 only: the passes of the last records call on a device that used the resident arrays in place, and those that
// compacted them through the gather kernel first
int ug_test_verify_records_passes(unsigned long long passes[2]) {
    if (!ughost::testHooksEnabled() || !passes) return 1;
    std::lock_guard<std::mutex> lock(g_trace.m);
    passes[0] = g_trace.in_place; passes[1] = g_trace.gathered;
    return 0;
}

// ULTRAGROTH_TEST_HOOKS=1 only: upload and ingest alone. plain_out: per record the plain 256 / 320 bytes the arrays hold after the
// ingest -- coordinates reduced, infinity and a point that failed (no root, off its curve) as zeros; status: ResidentBatch::ingest's
// byte. device < 0: the host's reading of the same records.
int ug_test_records_ingest(int device, int format, int ultra_, int count, const void* records, void* plain_out, unsigned char* status) {
    if (!ughost::testHooksEnabled() || !records || !plain_out || !status || count < 0 || !known_format(format)) return 1;
    try {
        const bool ultra = ultra_ != 0;
        const int k = ultra ? 2 : 1;
        const uint8_t* rec = static_cast<const uint8_t*>(records);
        uint8_t* out = static_cast<uint8_t*>(plain_out);
        const size_t stride = record_bytes(ultra, format), plain = record_bytes(ultra);
        auto leave = [&](size_t i, RecordPoints& pts) {            // what failed is zeros
            if (!g1_on_curve(pts.a)) pts.a = G1A{f1_zero(), f1_zero(), true};
            if (!g2_on_curve(pts.b)) pts.b = g2_inf();
            for (int s = 0; s < 2; s++) if (!g1_on_curve(pts.g[s])) pts.g[s] = G1A{f1_zero(), f1_zero(), true};
            record_write(RECORDS_PLAIN, ultra, pts, out + i * plain);
        };
        for (size_t first = 0; first < (size_t)count; first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, (size_t)count - first);
            if (device < 0) {
                parallel_for(m, [&](size_t j) {
                    const size_t i = first + j;
                    RecordPoints pts;
                    bool ok = record_read(format, ultra, rec + i * stride, pts);
                    ok = ok && g1_on_curve(pts.a) && g2_on_curve(pts.b) && g1_on_curve(pts.g[0]) && g1_on_curve(pts.g[1]);
                    status[i] = !ok ? UG_POINT_OFF_CURVE : g2_in_subgroup(pts.b) ? UG_POINT_OK : UG_POINT_OFF_SUBGROUP;
                    leave(i, pts);
                });
                continue;
            }
            ResidentBatch rb(device, (int)m, k, format);
            rb.ingest(rec + first * stride, status + first);
            std::vector<u32> a(m * G1_WORDS), b(m * G2_WORDS), g(m * (size_t)k * G1_WORDS);
            rb.download(a.data(), b.data(), g.data());
            parallel_for(m, [&](size_t j) {
                RecordPoints pts;
                pts.a = g1_load(&a[j * G1_WORDS], false);
                pts.b = g2_load(&b[j * G2_WORDS]);
                pts.g[0] = g1_load(&g[j * k * G1_WORDS], false);
                pts.g[1] = ultra ? g1_load(&g[(j * k + 1) * G1_WORDS], false) : G1A{f1_zero(), f1_zero(), true};
                leave(first + j, pts);
            });
        }
        return 0;
    } catch (...) { return 1; }
}
// ULTRAGROTH_TEST_HOOKS=1 only: f2_sqrt of count values given as plain c0 | c1 (64 bytes each). out: the root that is NOT the larger
// one, in the same form (zeros when there is none); has_root: one byte each. device < 0: the host's code.
int ug_test_fq2_sqrt(int device, int count, const void* in, void* out, unsigned char* has_root) {
    if (!ughost::testHooksEnabled() || !in || !out || !has_root || count < 0) return 1;
    try {
        if (device >= 0) {
            std::vector<u32> wi((size_t)count * 16), wo((size_t)count * 16);
            memcpy(wi.data(), in, wi.size() * sizeof(u32));
            fq2_sqrt_device(device, root_consts(), count, wi.data(), wo.data(), has_root);
            memcpy(out, wo.data(), wo.size() * sizeof(u32));
            return 0;
        }
        const uint8_t* p = static_cast<const uint8_t*>(in);
        uint8_t* o = static_cast<uint8_t*>(out);
        for (size_t i = 0; i < (size_t)count; i++) {
            const F2 v{f1_from_u256(p + i * 64), f1_from_u256(p + i * 64 + 32)};
            F2 r;
            const bool ok = f2_sqrt(root_consts(), v, r);
            if (ok && f2_larger(root_consts(), r)) r = -r;
            f1_to_le256(o + i * 64, r.a); f1_to_le256(o + i * 64 + 32, r.b);
            has_root[i] = ok ? 1 : 0;
        }
        return 0;
    } catch (...) { return 1; }
}

void ug_verify_batch_phase_ms(double ms[8]) {
    std::lock_guard<std::mutex> lock(g_trace.m);
    for (int k = 0; k < 8; k++) ms[k] = g_trace.phase_ms[k];
}
void ug_verify_batch_kernel_ms(double ms[3]) {
    std::lock_guard<std::mutex> lock(g_trace.m);
    for (int t = 0; t < 3; t++) ms[t] = g_trace.kernel_ms[t];
}

// ULTRAGROTH_TEST_HOOKS=1 only (else 1 is returned and nothing is written)
int ug_test_verify_batch_trace(int index, unsigned int scalar[4], unsigned int f[108]) {
    if (!ughost::testHooksEnabled()) return 1;
    std::lock_guard<std::mutex> lock(g_trace.m);
    const auto it = std::find(g_trace.index.begin(), g_trace.index.end(), index);
    if (it == g_trace.index.end()) return 1;
    const size_t at = (size_t)(it - g_trace.index.begin());
    if (scalar) memcpy(scalar, &g_trace.r[at * 4], 4 * sizeof(u32));
    if (f) memcpy(f, &g_trace.f[at * F12_WORDS], F12_WORDS * sizeof(u32));
    return 0;
}
int ug_test_miller(const unsigned char g1[64], const unsigned char g2[128], unsigned int f[108]) {
    if (!ughost::testHooksEnabled() || !g1 || !g2 || !f) return 1;
    u32 w[48];
    memcpy(w, g1, 64); memcpy(w + 16, g2, 128);
    if (words_all_zero(w, 16) || words_all_zero(w + 16, 32)) return 1;
    auto ld = [&](int at) { return F1{canon(from_mont256<FqParams>(w + at))}; };
    const G1A pt{ld(0), ld(8), false};
    const G2A q{F2{ld(16), ld(24)}, F2{ld(32), ld(40)}, false};
    f12_store(f, miller(consts(), q, pt));
    return 0;
}

// the final exponentiation of one value: g = the value after the hard part, *is_one = the verdict; device < 0: the host
int ug_test_final_exp(int device, const unsigned int f[108], unsigned int g[108], int* is_one) {
    if (!ughost::testHooksEnabled() || !f || !g || !is_one) return 1;
    try {
        if (device < 0) {
            F12 x, hard;
            f12_load(x, f);
            *is_one = final_exp_is_one(consts(), x, hard) ? 1 : 0;
            f12_store(g, hard);
        } else {
            final_exp_device(device, consts(), f, g, is_one);
        }
        return 0;
    } catch (...) { return 1; }
}

}  // extern "C"
