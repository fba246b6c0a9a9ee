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
// The JSON parser is json_min.hpp; the packed proof records and their conversions are verifier_records.cpp.
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
#include "json_min.hpp"
#include "pairing.hpp"
#include "pairing_dev.hpp"
#include "verifier_records.hpp"
#include "../../include/ultragroth_hip.h"
#include "../../include/verifier.h"

using namespace ugv;
using ughost::keccak256;

namespace {

// ---- field wrappers, Fq12, G2 steps, the Miller loop, the final exponentiation's is-one test and their constants: pairing.hpp ----
const FinalExpConsts& consts() { static const FinalExpConsts c = final_exp_consts(); return c; }

// start * prod_i miller(g2[i], g1[i]) is one after the final exponentiation. The Miller loops are independent: one host thread each.
// Pairs with a point at infinity are skipped (src/groth16.cpp:679-681).
bool pairing_product_is_one(const F12& start, const std::vector<G1A>& g1, const std::vector<G2A>& g2) {
    std::vector<std::future<F12>> parts;
    for (size_t i = 0; i < g1.size(); i++) {
        if (!pair_live(g1[i], g2[i])) continue;
        parts.push_back(std::async(std::launch::async, [&, i] { return miller(consts(), g2[i], g1[i]); }));
    }
    F12 acc = start, hard;
    for (auto& p : parts) acc = f12_mul(consts(), acc, p.get());
    return final_exp_is_one(consts(), acc, hard);
}

// ---- G1 arithmetic for vkX (ec.hpp, host) -------------------------------------------------------------------------------
G1XYZZ to_xyzz(const G1A& p) { return p.inf ? xyzz_inf<Fq>() : xyzz_from_affine(p.x.v, p.y.v); }
G1A from_xyzz(const G1XYZZ& p) {
    if (is_inf(p)) return g1_inf();
    Fq x, y;
    xyzz_to_affine(x, y, p);
    return G1A{F1{x}, F1{y}, false};
}
G1A g1_neg(const G1A& p) { return p.inf ? p : G1A{p.x, -p.y, false}; }

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

// ---- one key and one proof for both protocols ---------------------------------------------------------------------------------
struct Inputs { std::vector<std::vector<u32>> plain; };
struct Key {
    bool ultra = false;
    G1A alpha, ic_rand;                    // ic_rand: infinity for Groth16
    G2A beta, gamma, delta[2];             // delta[s] pairs with the proofs' G1 point s: (C) or (pi_f, pi_r)
    std::vector<G1A> ic;
    int k() const { return ultra ? 2 : 1; }
    size_t cols() const { return ic.size() + (ultra ? 1 : 0); }    // columns of vkX: IC_0 .. IC_nPublic [, IC_rand]
};
struct BatchProof : Points {
    Inputs in;
    u32 challenge[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // UltraGroth, set by the batch: derive_challenge of pi_r
    bool no_point = false;                 // a compressed record whose x has no y on the curve: INVALID like a point off its curve
};

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
Points parse_proof(const char* text, bool ultra) {                  // :16-57
    try {
        JVal j = JParser(text).parse_document();
        if (j.at("protocol").string() != (ultra ? "ultragroth" : "groth16")) throw std::invalid_argument("invalid proof data");
        Points p;
        p.a = g1_from_json(j.at("pi_a"));
        p.b = g2_from_json(j.at("pi_b"));
        p.g[0] = g1_from_json(j.at(ultra ? "pi_f" : "pi_c"));
        p.g[1] = ultra ? g1_from_json(j.at("pi_r")) : g1_inf();
        return p;
    } catch (...) { throw std::invalid_argument("invalid proof data"); }
}
Key parse_key(const char* text, bool ultra) {                       // :88-146, src/ultra_groth.cpp:543-563
    try {
        JVal j = JParser(text).parse_document();
        if (j.at("nPublic").type != JVal::Number) throw std::invalid_argument("nPublic");
        if (j.at("protocol").string() != (ultra ? "ultragroth" : "groth16") || j.at("curve").string() != "bn128") throw std::invalid_argument("protocol");
        Key k;
        k.ultra = ultra;
        k.alpha = g1_from_json(j.at("vk_alpha_1"));
        k.beta = g2_from_json(j.at("vk_beta_2"));
        k.gamma = g2_from_json(j.at("vk_gamma_2"));
        k.delta[0] = g2_from_json(j.at(ultra ? "vk_delta_c2_2" : "vk_delta_2"));
        k.delta[1] = ultra ? g2_from_json(j.at("vk_delta_c1_2")) : k.delta[0];
        const JVal& a = j.at("IC");
        if (a.type == JVal::Array) for (const JVal& e : a.arr) k.ic.push_back(g1_from_json(e));
        else if (a.type == JVal::Object) for (const auto& kv : a.obj) k.ic.push_back(g1_from_json(kv.second));   // json::items()
        if (k.ic.empty()) throw std::invalid_argument("IC");
        k.ic_rand = ultra ? g1_from_json(j.at("IC_rand")) : g1_inf();
        return k;
    } catch (...) { throw std::invalid_argument("invalid verification key data"); }
}
// the proof and the inputs of one proof from their texts, with what the single call says of them
BatchProof parse_texts(const char* proof, const char* inputs, bool ultra) {
    if (!proof || !inputs) throw std::invalid_argument("null argument");
    BatchProof p;
    static_cast<Points&>(p) = parse_proof(proof, ultra);
    p.in = parse_inputs(inputs);
    return p;
}
void check_length(size_t inputs, size_t ic_size, bool ultra) {      // src/groth16.cpp:318-320, src/ultra_groth.cpp:585-587
    if (inputs + 1 != ic_size) throw std::invalid_argument(ultra ? "len(inputs) != len(vk.IC)" : "len(inputs)+1 != len(vk.IC)");
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

bool proof_on_curve(const BatchProof& p) {
    return !p.no_point && g1_on_curve(p.a) && g1_on_curve(p.g[0]) && g1_on_curve(p.g[1]) && g2_on_curve(p.b);
}
bool key_on_curve(const Key& key) {
    bool ok = g1_on_curve(key.alpha) && g1_on_curve(key.ic_rand);
    for (const G1A& p : key.ic) ok = ok && g1_on_curve(p);
    for (const G2A* q : {&key.beta, &key.gamma, &key.delta[0], &key.delta[1]}) ok = ok && g2_on_curve(*q);
    return ok;
}

// The single-proof verifier on parsed values (p.in already has the key's length): VALID or INVALID.
// Points that are not on their curve can only come from malformed data: no pairing is defined for them.
int verify_one(const Key& key, const BatchProof& p) {
    if (!proof_on_curve(p) || !key_on_curve(key)) return VERIFIER_INVALID_PROOF;
    G1XYZZ vk = to_xyzz(key.ic[0]);                                 // the loops at src/groth16.cpp:322-332, src/ultra_groth.cpp:589-612
    for (size_t i = 0; i < p.in.plain.size(); i++) vk = xyzz_add(vk, xyzz_mul_scalar(to_xyzz(key.ic[i + 1]), p.in.plain[i].data(), 256));
    if (key.ultra) {
        u32 rand[8];
        derive_challenge_plain(rand, p.g[1]);
        vk = xyzz_add(vk, xyzz_mul_scalar(to_xyzz(key.ic_rand), rand, 256));
    }
    std::vector<G1A> g1{p.a, g1_neg(key.alpha), g1_neg(from_xyzz(vk))};
    std::vector<G2A> g2{p.b, key.beta, key.gamma};
    for (int s = 0; s < key.k(); s++) { g1.push_back(g1_neg(p.g[s])); g2.push_back(key.delta[s]); }
    return pairing_product_is_one(f12_one(), g1, g2) ? VERIFIER_VALID_PROOF : VERIFIER_INVALID_PROOF;
}

void copy_error(char* dst, unsigned long cap, const char* msg) {
    if (dst && cap) strncpy(dst, msg, cap);                         // as the reference: no terminator added beyond strncpy's
}
// what a call returns; whatever it throws is VERIFIER_ERROR and its text
template <class Fn> int guarded(char* error_msg, unsigned long error_msg_maxsize, const Fn& call) {
    try {
        return call();
    } catch (std::exception& e) {
        copy_error(error_msg, error_msg_maxsize, e.what());
    } catch (...) {
        copy_error(error_msg, error_msg_maxsize, "unknown error");
    }
    return VERIFIER_ERROR;
}
int verify_texts(bool ultra, const char* proof, const char* inputs, const char* verification_key, char* error_msg, unsigned long error_msg_maxsize) {
    return guarded(error_msg, error_msg_maxsize, [&] {
        if (!verification_key) throw std::invalid_argument("null argument");
        const BatchProof p = parse_texts(proof, inputs, ultra);
        const Key key = parse_key(verification_key, ultra);
        check_length(p.in.plain.size(), key.ic.size(), ultra);
        return verify_one(key, p);
    });
}

}  // namespace

extern "C" {

int groth16_verify(const char* proof, const char* inputs, const char* verification_key, char* error_msg,
                   unsigned long error_msg_maxsize) {
    return verify_texts(false, proof, inputs, verification_key, error_msg, error_msg_maxsize);
}
int ultra_groth_verify(const char* proof, const char* inputs, const char* verification_key, char* error_msg,
                       unsigned long error_msg_maxsize) {
    return verify_texts(true, proof, inputs, verification_key, error_msg, error_msg_maxsize);
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

// The trees of one device pass: a forest with one tree per segment -- the proofs of one key, contiguous in the pass
// (pairing_dev.hpp: ForestPlan). A call under one key has one segment, and the forest is its tree.
struct Forest {
    ForestPlan plan;
    int k;
    std::vector<u32> f_tree, g_tree;
    Forest(const std::vector<u32>& sizes, int k_) : plan(sizes.data(), sizes.size()), k(k_), f_tree(plan.nodes * F12_WORDS), g_tree(plan.nodes * k_ * XYZZ_WORDS) {}
    // the leaves of the whole pass, one Miller loop each on the host threads
    void host_leaves(const u32* a, const u32* b, const u32* g, const u32* r) {
        const PairingConsts& kc = consts();
        parallel_for(plan.off.back()[0] + plan.size.back(), [&](size_t i) {
            batch_leaf(kc, a + i * G1_WORDS, b + i * G2_WORDS, g + i * k * G1_WORDS, k, r + i * 4, &f_tree[i * F12_WORDS], &g_tree[i * k * XYZZ_WORDS]);
        });
    }
};

// one segment of a pass: m proofs of one key, a view of their trees in the pass's forest, and their prefix sums
struct Pass {
    const Key& key;
    size_t m, cols, first;                 // first: the position of the segment's first proof in the pass
    int k;
    u32* f_tree;                           // the forest's arrays; node j of `level` is node level_off[level] + j of them
    u32* g_tree;
    std::vector<Fr> prefix;                // (m + 1) x cols: S, t_0 .. t_{nPublic-1}, [t_rand]
    std::vector<size_t> level_off, level_size;
    unsigned long long checks = 0;

    Pass(const Key& key_, Forest& forest, size_t s)
        : key(key_), m(forest.plan.size[s]), cols(key_.cols()), first(forest.plan.first[s]), k(key_.k()), f_tree(forest.f_tree.data()), g_tree(forest.g_tree.data()),
          level_off(forest.plan.off[s]) {
        for (size_t n = m;; n = (n + 1) / 2) { level_size.push_back(n); if (n <= 1) break; }
    }
    // node j of `level`: the product of its proofs' miller(B_i, r_i A_i) in f, and the fixed pairs of its batch equation appended
    void node_pairs(size_t level, size_t j, F12& f, std::vector<G1A>& g1, std::vector<G2A>& g2) const {
        const size_t lo = j << level, hi = std::min(m, (j + 1) << level), node = level_off[level] + j;
        std::vector<std::vector<u32>> sc(cols, std::vector<u32>(8));
        for (size_t c = 0; c < cols; c++) to_normal(sc[c].data(), sub<1>(prefix[hi * cols + c], prefix[lo * cols + c]));
        G1XYZZ vkx = xyzz_mul_scalar_w4(to_xyzz(key.ic[0]), sc[0].data());
        for (size_t c = 1; c < key.ic.size(); c++) vkx = xyzz_add(vkx, xyzz_mul_scalar_w4(to_xyzz(key.ic[c]), sc[c].data()));
        if (key.ultra) vkx = xyzz_add(vkx, xyzz_mul_scalar_w4(to_xyzz(key.ic_rand), sc[cols - 1].data()));
        g1.push_back(g1_neg(from_xyzz(xyzz_mul_scalar_w4(to_xyzz(key.alpha), sc[0].data())))); g2.push_back(key.beta);
        g1.push_back(g1_neg(from_xyzz(vkx))); g2.push_back(key.gamma);
        for (int s = 0; s < k; s++) {
            g1.push_back(g1_neg(from_xyzz(xyzz_load(&g_tree[(node * k + s) * XYZZ_WORDS]))));
            g2.push_back(key.delta[s]);
        }
        f12_load(f, &f_tree[node * F12_WORDS]);
    }
    // the batch equation over the proofs of node j of `level`
    bool node_ok(size_t level, size_t j) {
        checks++;
        F12 f;
        std::vector<G1A> g1;
        std::vector<G2A> g2;
        node_pairs(level, j, f, g1, g2);
        return pairing_product_is_one(f, g1, g2);
    }
    // The segment's value in the pass's one equation: its root times the Miller loops of its fixed pairs, on the calling thread
    // (the segments of a pass are spread over the host threads). The pass holds when the product of these is one after ONE final
    // exponentiation.
    F12 root_value() const {
        F12 f;
        std::vector<G1A> g1;
        std::vector<G2A> g2;
        node_pairs(level_size.size() - 1, 0, f, g1, g2);
        for (size_t i = 0; i < g1.size(); i++)
            if (pair_live(g1[i], g2[i])) f = f12_mul(consts(), f, miller(consts(), g2[i], g1[i]));
        return f;
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
    // the segment's tree above its leaves (Forest::host_leaves), on the host; spread: over the host threads, level by level
    void host_trees(bool spread) {
        const PairingConsts& kc = consts();
        for (size_t l = 0; l + 1 < level_size.size(); l++) {
            const size_t n_src = level_size[l];
            const u32* fs = &f_tree[level_off[l] * F12_WORDS];
            const u32* gs = &g_tree[level_off[l] * k * XYZZ_WORDS];
            u32* fd = &f_tree[level_off[l + 1] * F12_WORDS];
            u32* gd = &g_tree[level_off[l + 1] * k * XYZZ_WORDS];
            auto node = [&](size_t j) {
                const bool pair = 2 * j + 1 < n_src;
                f12_node(kc, fs + 2 * j * F12_WORDS, pair ? fs + (2 * j + 1) * F12_WORDS : nullptr, fd + j * F12_WORDS);
                for (int s = 0; s < k; s++)
                    g1_node(gs + (2 * j * k + s) * XYZZ_WORDS, pair ? gs + ((2 * j + 1) * k + s) * XYZZ_WORDS : nullptr, gd + (j * k + s) * XYZZ_WORDS);
            };
            if (spread) parallel_for(level_size[l + 1], node);
            else for (size_t j = 0; j < level_size[l + 1]; j++) node(j);
        }
    }
};
// The host forest of a pass (device < 0): the leaves are there; every segment's tree by the loop above. Few segments: each level
// over the host threads; many: a segment per thread.
void host_forest(std::vector<Pass>& segs) {
    if (segs.size() < 16) { for (Pass& p : segs) p.host_trees(true); return; }
    parallel_for(segs.size(), [&](size_t s) { segs[s].host_trees(false); });
}

struct Ctx {                               // a device context for the subgroup check of the B points
    ug_ctx* c = nullptr;
    explicit Ctx(int device) { if (ug_ctx_create(&c, device) != UG_OK) throw std::runtime_error(ug_last_error()); }
    ~Ctx() { if (c) ug_ctx_destroy(c); }
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The arrays of a pass or of a launch of the judge (pairing_dev.hpp) from the proofs idx[0..m) of `proofs`; idx == nullptr: its first m.
void pack_points(const std::vector<BatchProof>& proofs, const size_t* idx, size_t m, int k, u32* a, u32* b, u32* g) {
    parallel_for(m, [&](size_t i) {
        const Points& p = proofs[idx ? idx[i] : i];
        g1_words(a + i * G1_WORDS, p.a);
        g2_words(b + i * G2_WORDS, p.b);
        for (int s = 0; s < k; s++) g1_words(g + (i * k + s) * G1_WORDS, p.g[s]);
    });
}

// The suspects sus[] of a call (positions in `proofs`), each decided by judge_proof: on `device` in launches of at most PAIRING_PASS,
// on host threads for device < 0. valid[s] answers suspect s.
// key_of: the key of every proof of the call (empty: keys[0]); sus is ordered by key, so the suspects of a key are contiguous in every
// launch, and a launch takes the keys it meets as a table (one key: the table is that key, the launch the one-key kernel).
void judge_suspects(const std::vector<Key>& keys, const std::vector<int>& key_of, int device, const std::vector<BatchProof>& proofs, const std::vector<size_t>& sus,
                    std::vector<char>& valid, ug_verify_batch_stats_ex& stats) {
    const size_t n = sus.size(), k = (size_t)keys[0].k();
    auto key_at = [&](size_t s) { return key_of.empty() ? (size_t)0 : (size_t)key_of[sus[s]]; };
    valid.assign(n, 0);
    for (size_t first = 0; first < n; first += PAIRING_PASS) {
        const size_t m = std::min<size_t>(PAIRING_PASS, n - first);
        // the keys of this launch, in order: their suspects, columns, points, G2 points and miller(beta, -alpha)
        std::vector<size_t> which;
        std::vector<int> key_first, key_cols;
        std::vector<size_t> slot(m), sc_at(m + 1, 0), point_at;
        for (size_t i = 0; i < m; i++) {
            if (which.empty() || which.back() != key_at(first + i)) { which.push_back(key_at(first + i)); key_first.push_back((int)i); }
            slot[i] = which.size() - 1;
            sc_at[i + 1] = sc_at[i] + keys[which.back()].cols() * 8;
        }
        key_first.push_back((int)m);
        const size_t n_keys = which.size();
        size_t all_cols = 0;
        for (size_t q : which) { point_at.push_back(all_cols); key_cols.push_back((int)keys[q].cols()); all_cols += keys[q].cols(); }
        std::vector<u32> points(all_cols * G1_WORDS), key_g2(n_keys * (1 + k) * G2_WORDS), f_ab(n_keys * F12_WORDS);
        parallel_for(n_keys, [&](size_t q) {
            const Key& key = keys[which[q]];
            u32* pt = &points[point_at[q] * G1_WORDS];
            for (size_t c = 0; c < key.ic.size(); c++) g1_words(pt + c * G1_WORDS, key.ic[c]);
            if (key.ultra) g1_words(pt + (key.cols() - 1) * G1_WORDS, key.ic_rand);
            u32* g2 = &key_g2[q * (1 + k) * G2_WORDS];
            g2_words(g2, key.gamma);
            for (size_t s = 0; s < k; s++) g2_words(g2 + (1 + s) * G2_WORDS, key.delta[s]);
            const G1A nalpha = g1_neg(key.alpha);
            f12_store(&f_ab[q * F12_WORDS], pair_live(nalpha, key.beta) ? miller(consts(), key.beta, nalpha) : f12_one());
        });
        std::vector<u32> a(m * G1_WORDS), b(m * G2_WORDS), g(m * k * G1_WORDS), scalars(sc_at[m], 0), verdict(m, 0);
        pack_points(proofs, &sus[first], m, (int)k, a.data(), b.data(), g.data());
        parallel_for(m, [&](size_t i) {
            const BatchProof& p = proofs[sus[first + i]];
            const Key& key = keys[which[slot[i]]];
            u32* sc = &scalars[sc_at[i]];
            sc[0] = 1;                                              // IC_0 itself
            for (size_t c = 0; c < p.in.plain.size(); c++) memcpy(sc + (1 + c) * 8, p.in.plain[c].data(), 8 * sizeof(u32));
            if (key.ultra) memcpy(sc + (key.cols() - 1) * 8, p.challenge, 8 * sizeof(u32));
        });
        if (device < 0) {
            parallel_for(m, [&](size_t i) {
                const size_t q = slot[i], cols = (size_t)key_cols[q];
                G1XYZZ sum = xyzz_inf<Fq>();
                u32 term[XYZZ_WORDS], nvkx[G1_WORDS];
                for (size_t c = 0; c < cols; c++) {
                    vkx_term(&points[(point_at[q] + c) * G1_WORDS], &scalars[sc_at[i] + c * 8], term);
                    sum = xyzz_add(sum, xyzz_load(term));
                }
                vkx_finish(sum, nvkx);
                verdict[i] = judge_proof(consts(), &a[i * G1_WORDS], &b[i * G2_WORDS], nvkx, &g[i * k * G1_WORDS], (int)k, &key_g2[q * (1 + k) * G2_WORDS],
                                         &f_ab[q * F12_WORDS]);
            });
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            PairingJudge pj;
            pj.n = (int)m; pj.k = (int)k; pj.cols = key_cols[0]; pj.a = a.data(); pj.b = b.data(); pj.g = g.data(); pj.scalars = scalars.data();
            pj.points = points.data(); pj.key_g2 = key_g2.data(); pj.f_alpha_beta = f_ab.data(); pj.verdict = verdict.data();
            pj.n_keys = (int)n_keys; pj.key_first = key_first.data(); pj.key_cols = key_cols.data();
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

// Where the proofs of a call come from: JSON texts or packed records (verifier_records.cpp). check() is the call's test of its
// arguments; parse() is step 1 of the batch for proof i and throws what the single call would say.
struct Source {
    bool ultra = false;
    virtual ~Source() {}
    // null_argument: count, key or verdicts already are one. The order of the tests is the order of the messages.
    virtual void check(int count, bool null_argument) const = 0;
    // points = false: only what the host needs of a proof that stays on the device -- the inputs and the challenge
    virtual void parse(size_t i, BatchProof& p, size_t ic_size, bool points) const = 0;
    const uint8_t* records = nullptr;      // packed records, for the device to ingest (texts: none)
    int format = RECORDS_PLAIN;            // ... their layout
    size_t n_pub = 0;                      // ... and their inputs per proof, the same for every proof of a call under one key
    // several keys: the inputs per proof of every key, and where proof i's begin in the ragged input block (bytes); set by ragged()
    std::vector<size_t> n_pub_of_key, inputs_at;
    const int* key_of = nullptr;
    bool records_call = false, keyed = false;      // the call takes packed records; it is a call under several keys
    void ragged(const int* key_of_, const int* n_pub_, size_t n_keys, size_t count) {
        key_of = key_of_;
        for (size_t q = 0; q < n_keys; q++) n_pub_of_key.push_back((size_t)n_pub_[q]);
        inputs_at.assign(count + 1, 0);
        for (size_t i = 0; i < count; i++) inputs_at[i + 1] = inputs_at[i] + n_pub_of_key[(size_t)key_of[i]] * 32;
    }
};
struct JsonSource : Source {
    const char* const* proofs;
    const char* const* inputs;
    JsonSource(bool ultra_, const char* const* proofs_, const char* const* inputs_) : proofs(proofs_), inputs(inputs_) { ultra = ultra_; }
    void check(int count, bool null_argument) const override {     // null arrays fail the call as a null key does
        if (null_argument || (count > 0 && (!proofs || !inputs))) throw std::invalid_argument("null argument");
    }
    void parse(size_t i, BatchProof& p, size_t ic_size, bool) const override {
        p = parse_texts(proofs[i], inputs[i], ultra);
        check_length(p.in.plain.size(), ic_size, ultra);
    }
};
struct RecordSource : Source {
    const uint8_t* inputs;
    RecordSource(bool ultra_, int format_, const void* records_, const void* inputs_, int n_pub_) : inputs(static_cast<const uint8_t*>(inputs_)) {
        ultra = ultra_; format = format_; records = static_cast<const uint8_t*>(records_); n_pub = (size_t)std::max(n_pub_, 0); records_call = true;
    }
    void check(int count, bool null_argument) const override {
        if (!known_format(format)) throw std::invalid_argument("format: not one of UG_RECORDS_PLAIN, UG_RECORDS_EVM, UG_RECORDS_COMPRESSED");
        if (null_argument || (count > 0 && (!records || !inputs))) throw std::invalid_argument("null argument");
        if (!n_pub && !keyed) throw std::invalid_argument("invalid inputs data");
    }
    // points = false reads pi_r only (the challenge); not even that of a compressed record, whose pi_r the device's ingest leaves
    void parse(size_t i, BatchProof& p, size_t, bool points) const override {
        const uint8_t* rec = records + i * record_bytes(ultra, format);
        p.g[1] = g1_inf();
        p.no_point = points && !record_read(format, ultra, rec, p);
        if (!points && ultra && format != RECORDS_COMPRESSED) record_read_pi_r(format, rec, p.g[1]);
        const size_t n_in = keyed ? n_pub_of_key[(size_t)key_of[i]] : n_pub;
        const uint8_t* in = inputs + (keyed ? inputs_at[i] : i * n_pub * 32);
        p.in.plain.assign(n_in, std::vector<u32>(8));
        for (size_t c = 0; c < n_in; c++) {                         // reduced mod r, as fr_plain_from_decimal
            uint8_t le[32];
            inputs_to_plain(format, in + c * 32, 1, le);
            u32 v[8];
            memcpy(v, le, 32);
            to_normal(p.in.plain[c].data(), from_normal<FrParams>(v));
        }
    }
};

// where a call's time goes: the indices of ug_verify_batch_phase_ms
enum Phase { PHASE_KEY, PHASE_PARSE, PHASE_SUBGROUP, PHASE_SCALARS, PHASE_PACKING, PHASE_PASS, PHASE_SEARCH, PHASE_SINGLES, PHASES };
static_assert(PHASES == 8, "ug_verify_batch_phase_ms writes 8 values");

// One call of the batch verifier. Proofs that are not packed records on a device are gathered: (1) parsed on the host, (2) those with
// B outside the subgroup set aside, (3) the rest packed into the arrays of a pass. Packed records on a device are resident: 1-3 happen
// there, per pass. Either way a pass ends in run_pass, and (4) what the passes left undecided goes to the judge or to verify_one.
struct BatchCall {
    const Source& src;
    const int device;
    const BatchOptions opt;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    // The keys of the call and the key of every proof. A call under one key: one key, key_of empty. A call under several
    // (the _keys entry points): key_of[i] indexes keys, checked by the entry point; the proofs of a pass are taken in key order
    // (a stable sort), so that those of one key form a segment, and the verdicts are the caller's order again.
    std::vector<Key> keys;
    std::vector<char> key_ok;              // per key; else no batching under it: every proof of it that parses is verify_one's
    const std::vector<int> key_of;
    const size_t n;
    bool resident = false;
    const bool hooks;
    std::vector<State> state;
    std::vector<int> verdict;
    std::vector<BatchProof> parsed;
    std::vector<std::string> message;      // of the proofs whose verdict stays VERIFIER_ERROR
    ug_verify_batch_stats_ex stats = {{0, 0, 0, 0.0, 0.0}, 0, 0, 0.0};
    unsigned long long segments = 0, tree_launches = 0, key_checks = 0;        // ug_verify_batch_stats_keys
    double phase[PHASES] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t_lap = t_start;

    // key_texts: n_keys texts. keyed: the call names its keys by index, and says so in what it reports of one ("key <k>: ...").
    // The keys are parsed and checked -- the subgroup tests are the 8.7 ms of the one-key call -- across the host threads.
    BatchCall(const Source& src_, int device_, size_t count, const char* const* key_texts, size_t n_keys, bool keyed, const int* key_of_,
              const BatchOptions& opt_)
        : src(src_), device(device_), opt(opt_), keys(n_keys), key_ok(n_keys, 0), key_of(key_of_ ? key_of_ : nullptr, key_of_ ? key_of_ + count : nullptr), n(count),
          hooks(ughost::testHooksEnabled()), state(count, SINGLE), verdict(count, VERIFIER_ERROR), parsed(count), message(count) {
        std::vector<std::string> failure(n_keys);
        parallel_for(n_keys, [&](size_t q) {
            try {
                keys[q] = parse_key(key_texts[q], src.ultra);
                if (keyed ? src.records_call : src.records != nullptr) check_length(keyed ? src.n_pub_of_key[q] : src.n_pub, keys[q].ic.size(), src.ultra);      // (texts: checked per proof, in parse)
                key_ok[q] = batchable(keys[q]);
            } catch (std::exception& e) { failure[q] = e.what(); }
        });
        for (size_t q = 0; q < n_keys; q++)
            if (!failure[q].empty()) throw std::invalid_argument(keyed ? "key " + std::to_string(q) + ": " + failure[q] : failure[q]);
        bool any_ok = false;
        for (char ok : key_ok) any_ok = any_ok || ok;
        resident = any_ok && device >= 0 && src.records;
        if (hooks) { std::lock_guard<std::mutex> lock(g_trace.m); g_trace.index.clear(); g_trace.r.clear(); g_trace.f.clear(); g_trace.in_place = g_trace.gathered = 0; }
        lap(PHASE_KEY);
    }
    size_t key_index(size_t i) const { return key_of.empty() ? 0 : (size_t)key_of[i]; }
    const Key& key_for(size_t i) const { return keys[key_index(i)]; }
    // idx (proofs of the call) in key order, the caller's order within a key
    void group_by_key(std::vector<size_t>& idx) const {
        if (!key_of.empty()) std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return key_of[x] < key_of[y]; });
    }
    static bool batchable(const Key& key) {                         // every point on its curve, every G2 point in the subgroup
        bool ok = key_on_curve(key);
        for (const G2A* q : {&key.beta, &key.gamma, &key.delta[0], &key.delta[1]}) ok = ok && g2_in_subgroup(*q);
        return ok;
    }
    void lap(Phase p) {
        const auto now = std::chrono::steady_clock::now();
        phase[p] += std::chrono::duration<double, std::milli>(now - t_lap).count();
        t_lap = now;
    }

    int run(int* verdicts, char* error_msg, unsigned long error_msg_maxsize) {
        if (resident) resident_passes();
        else {
            parse_all();
            std::vector<size_t> idx = set_aside_off_subgroup();
            group_by_key(idx);
            gathered_passes(idx);
        }
        decide_singles();
        return finish(verdicts, error_msg, error_msg_maxsize);
    }

    // 1. parse; what the single call would answer before any pairing is answered here. Under a key the batch refuses the parse is
    //    the first step of the single verifier, which every proof is then handed to.
    void parse_all() {
        parallel_for(n, [&](size_t i) {
            const bool ok = key_ok[key_index(i)];
            state[i] = ok ? DONE : SINGLE;
            try {
                BatchProof& p = parsed[i];
                src.parse(i, p, key_for(i).ic.size(), true);
                if (!ok) return;
                if (!proof_on_curve(p)) { verdict[i] = VERIFIER_INVALID_PROOF; return; }
                if (src.ultra) derive_challenge_plain(p.challenge, p.g[1]);
                state[i] = BATCH;
            } catch (std::exception& e) { message[i] = e.what(); }
        });
        lap(PHASE_PARSE);
    }
    // 2. B outside the subgroup: out of the batch. Returns the proofs that stay in it.
    std::vector<size_t> set_aside_off_subgroup() {
        std::vector<size_t> cand, idx;
        for (size_t i = 0; i < n; i++) if (state[i] == BATCH) cand.push_back(i);
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
            stats.base.device_ms += ms_since(t0);
        }
        for (size_t i : cand) { if (state[i] == BATCH) idx.push_back(i); else stats.base.off_subgroup++; }
        lap(PHASE_SUBGROUP);
        return idx;
    }
    // the scalars of a pass of m proofs
    void draw_scalars(size_t m, std::vector<u32>& r) {
        r.resize(m * 4);
        for (size_t got = 0; got < r.size() * sizeof(u32);) {
            const ssize_t w = getrandom((uint8_t*)r.data() + got, r.size() * sizeof(u32) - got, 0);
            if (w <= 0) throw std::runtime_error("getrandom failed");
            got += (size_t)w;
        }
        for (size_t i = 0; i < m; i++) if (!(r[4 * i] | r[4 * i + 1] | r[4 * i + 2] | r[4 * i + 3])) r[4 * i] = 1;       // (2^-128)
    }
    // the prefix sums of a segment: its proofs idx[0..m) and their scalars r
    void prefix_sums(Pass& pass, const size_t* idx, const u32* r) {
        const size_t m = pass.m;
        pass.prefix.assign((m + 1) * pass.cols, fp_zero<FrParams>());
        std::vector<Fr> term(m * pass.cols);
        parallel_for(m, [&](size_t i) {
            const BatchProof& p = parsed[idx[i]];
            const u32 rw[8] = {r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], 0, 0, 0, 0};
            const Fr rf = fr_from_plain(rw);
            Fr* t = &term[i * pass.cols];
            t[0] = rf;
            for (size_t c = 0; c < p.in.plain.size(); c++) t[1 + c] = canon(mul(rf, fr_from_plain(p.in.plain[c].data())));
            if (src.ultra) t[pass.cols - 1] = canon(mul(rf, fr_from_plain(p.challenge)));
        });
        for (size_t i = 0; i < m; i++)
            for (size_t c = 0; c < pass.cols; c++)
                pass.prefix[(i + 1) * pass.cols + c] = canon(add(pass.prefix[i * pass.cols + c], term[i * pass.cols + c]));
    }
    // The trees of a pass are there: the pass's check, the search of a rejected pass, the verdicts. suspects: positions in the pass.
    // One segment: its root check, then its tree. Several: ONE equation for the pass -- the product of the segments' values
    // (Pass::root_value, made across the host threads), one final exponentiation. A pass that fails is searched down a binary
    // tree over the segments, a node's value the product of its segments' values: both children of a failing node are checked and
    // the failing ones entered (an odd last node copied up has its child's value: no check), and a failing segment is searched as
    // under one key, its root not checked again. Judge on: the segments' level follows the rule of Pass::search -- breadth first
    // while the failing nodes number at most search_width, then every proof under a failing node is a suspect.
    void settle(std::vector<Pass>& segs, const size_t* idx, size_t m) {
        std::vector<size_t> suspects;
        auto enter = [&](Pass& seg) {                               // a segment whose root is known to fail
            std::vector<size_t> local;
            if (opt.judge) seg.search(seg.level_size.size() - 1, 0, (size_t)opt.search_width, local);
            else seg.walk(seg.level_size.size() - 1, 0, local);
            for (size_t s : local) suspects.push_back(seg.first + s);
        };
        if (segs.size() == 1) {
            key_checks++;
            if (!segs[0].node_ok(segs[0].level_size.size() - 1, 0)) enter(segs[0]);
        } else {
            std::vector<std::vector<F12>> value(1, std::vector<F12>(segs.size()));     // value[l][j]: segments j << l .. (j + 1) << l
            parallel_for(segs.size(), [&](size_t s) { value[0][s] = segs[s].root_value(); });
            while (value.back().size() > 1) {
                const std::vector<F12>& below = value.back();
                std::vector<F12> above((below.size() + 1) / 2);
                for (size_t j = 0; j < above.size(); j++) above[j] = 2 * j + 1 < below.size() ? f12_mul(consts(), below[2 * j], below[2 * j + 1]) : below[2 * j];
                value.push_back(std::move(above));
            }
            unsigned long long checks = 0;
            auto ok = [&](size_t level, size_t j) { checks++; F12 hard; return final_exp_is_one(consts(), value[level][j], hard); };
            auto whole = [&](size_t level, size_t j) {
                for (size_t s = j << level; s < std::min(segs.size(), (j + 1) << level); s++)
                    for (size_t i = 0; i < segs[s].m; i++) suspects.push_back(segs[s].first + i);
            };
            size_t level = value.size() - 1;
            std::vector<size_t> failing;
            if (!ok(level, 0)) failing.push_back(0);
            while (!failing.empty() && level > 0) {                 // all of `failing` on `level`
                if (opt.judge && failing.size() > (size_t)opt.search_width) { for (size_t j : failing) whole(level, j); failing.clear(); break; }
                std::vector<size_t> next;
                for (size_t j : failing) {
                    if (2 * j + 1 >= value[level - 1].size()) { next.push_back(2 * j); continue; }        // copied up: the same value
                    for (size_t c = 2 * j; c <= 2 * j + 1; c++) if (!ok(level - 1, c)) next.push_back(c);
                }
                failing.swap(next);
                level--;
            }
            for (size_t s : failing) enter(segs[s]);                // level 0: the failing segments
            key_checks += checks;
            stats.base.batch_checks += checks;
        }
        for (size_t i = 0; i < m; i++) { verdict[idx[i]] = VERIFIER_VALID_PROOF; state[idx[i]] = DONE; }
        for (size_t s : suspects) state[idx[s]] = SINGLE;
        for (const Pass& seg : segs) stats.base.batch_checks += seg.checks;
    }
    // the segments of a pass over the proofs idx[0..m), which are in key order: the sizes of the runs of one key
    std::vector<u32> segment_sizes(const size_t* idx, size_t m) const {
        std::vector<u32> sizes;
        for (size_t i = 0; i < m; i++) {
            if (i && key_index(idx[i]) == key_index(idx[i - 1])) sizes.back()++;
            else sizes.push_back(1);
        }
        return sizes;
    }
    // One pass over the proofs idx[0..m) of the call, in key order: the forest of its segments, scalars and prefix sums, the trees from
    // make_trees(forest, r, kernel_ms) -- the host forest, pairing_batch_device or ResidentBatch::run; it returns its tree launches --,
    // then the checks. The one place that accounts a pass's device time and leaves its kernel times and, for the test hooks, its
    // scalars and leaves (hook_counter: which kind of resident pass it was).
    template <class MakeTrees> void run_pass(const size_t* idx, size_t m, unsigned long long* hook_counter, const MakeTrees& make_trees) {
        Forest forest(segment_sizes(idx, m), src.ultra ? 2 : 1);
        std::vector<Pass> segs;
        segs.reserve(forest.plan.size.size());
        for (size_t s = 0; s < forest.plan.size.size(); s++) segs.emplace_back(key_for(idx[forest.plan.first[s]]), forest, s);
        segments += segs.size();
        std::vector<u32> r;
        draw_scalars(m, r);
        for (Pass& seg : segs) prefix_sums(seg, idx + seg.first, &r[seg.first * 4]);
        lap(PHASE_SCALARS);
        const auto t0 = std::chrono::steady_clock::now();
        double kernel_ms[3] = {0, 0, 0};
        tree_launches += (unsigned long long)make_trees(forest, segs, r.data(), kernel_ms);
        if (device >= 0) stats.base.device_ms += ms_since(t0);
        {
            std::lock_guard<std::mutex> lock(g_trace.m);
            if (device >= 0) for (int t = 0; t < 3; t++) g_trace.kernel_ms[t] = kernel_ms[t];
            if (hooks) {
                for (size_t i = 0; i < m; i++) g_trace.index.push_back((int)idx[i]);
                g_trace.r.insert(g_trace.r.end(), r.begin(), r.end());
                g_trace.f.insert(g_trace.f.end(), forest.f_tree.begin(), forest.f_tree.begin() + m * F12_WORDS);
                if (hook_counter) ++*hook_counter;
            }
        }
        lap(PHASE_PASS);
        settle(segs, idx, m);
        lap(PHASE_SEARCH);
    }
    // the plan a device pass is given: none for one segment, which keeps the one-key tree kernels and their layout
    static const ForestPlan* device_plan(const Forest& forest) { return forest.plan.size.size() > 1 ? &forest.plan : nullptr; }
    // 3. the batch, in passes; idx: the proofs that stay in it, in key order
    void gathered_passes(const std::vector<size_t>& idx) {
        for (size_t first = 0; first < idx.size(); first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, idx.size() - first);
            const int k = src.ultra ? 2 : 1;
            std::vector<u32> a(m * G1_WORDS), b(m * G2_WORDS), g(m * k * G1_WORDS);
            pack_points(parsed, &idx[first], m, k, a.data(), b.data(), g.data());
            lap(PHASE_PACKING);
            run_pass(&idx[first], m, nullptr, [&](Forest& forest, std::vector<Pass>& segs, const u32* r, double kernel_ms[3]) {
                if (device < 0) { forest.host_leaves(a.data(), b.data(), g.data(), r); host_forest(segs); return 0; }
                PairingBatch pb;
                pb.n = (int)m; pb.k = k; pb.a = a.data(); pb.b = b.data(); pb.g = g.data(); pb.r = r;
                pb.f_tree = forest.f_tree.data(); pb.g_tree = forest.g_tree.data(); pb.plan = device_plan(forest);
                pairing_batch_device(device, consts(), pb);
                for (int t = 0; t < 3; t++) kernel_ms[t] = pb.kernel_ms[t];
                return pb.tree_launches;
            });
        }
    }
    // 1-3 for packed records on a device, per pass of PAIRING_PASS records: the raw records cross PCIe once, the device reduces
    // and checks them and keeps the arrays of the Miller kernel; the host reads no coordinate of a proof that stays in the
    // batch (UltraGroth: pi_r, for the challenge). Off its curve: INVALID; pi_b off the subgroup: SINGLE, as in step 2.
    // Several keys: the records of a pass are uploaded grouped by key -- reordered on the host before the copy, 16 MB a pass at most
    // (none when they lie in that order already, as under one key) --, so that ingest, ladder and gather work as they are and what
    // they keep is in key order. The records of a key the batch refuses are not uploaded: the single verifier's (step 4).
    void resident_passes() {
        const int k = src.ultra ? 2 : 1, format = src.format;
        const bool late_challenge = src.ultra && format == RECORDS_COMPRESSED;     // pi_r.y is the device's to find: no host root per proof
        const size_t stride = record_bytes(src.ultra, format);
        std::vector<size_t> order;
        for (size_t i = 0; i < n; i++) if (key_ok[key_index(i)]) order.push_back(i);
        group_by_key(order);
        for (size_t first = 0; first < order.size(); first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, order.size() - first);
            const size_t* ids = &order[first];
            parallel_for(m, [&](size_t i) {
                BatchProof& p = parsed[ids[i]];
                src.parse(ids[i], p, key_for(ids[i]).ic.size(), false);
                if (src.ultra && !late_challenge) derive_challenge_plain(p.challenge, p.g[1]);
            });
            const uint8_t* records = src.records + ids[0] * stride;
            std::vector<uint8_t> grouped;
            bool in_order = true;
            for (size_t i = 1; i < m && in_order; i++) in_order = ids[i] == ids[i - 1] + 1;
            if (!in_order) {
                grouped.resize(m * stride);
                parallel_for((m + 1023) / 1024, [&](size_t c) {
                    for (size_t i = c * 1024; i < std::min(m, (c + 1) * 1024); i++) memcpy(&grouped[i * stride], src.records + ids[i] * stride, stride);
                });
                records = grouped.data();
            }
            lap(PHASE_PARSE);
            const auto t0 = std::chrono::steady_clock::now();
            ResidentBatch rb(device, (int)m, k, format);
            std::vector<uint8_t> status(m);
            rb.ingest(records, status.data());
            if (late_challenge) {                                   // the rows of pi_r as the ingest decompressed them
                std::vector<u32> g(m * (size_t)k * G1_WORDS);
                rb.download(nullptr, nullptr, g.data());
                parallel_for(m, [&](size_t i) {
                    if (status[i] == UG_POINT_OFF_CURVE) return;
                    BatchProof& p = parsed[ids[i]];
                    p.g[1] = g1_load(&g[(i * k + 1) * G1_WORDS], false);
                    derive_challenge_plain(p.challenge, p.g[1]);
                });
            }
            stats.base.device_ms += ms_since(t0);
            std::vector<size_t> kept;
            std::vector<u32> keep;
            for (size_t i = 0; i < m; i++) {
                if (status[i] == UG_POINT_OK) { kept.push_back(ids[i]); keep.push_back((u32)i); state[ids[i]] = BATCH; }
                else if (status[i] == UG_POINT_OFF_SUBGROUP) { state[ids[i]] = SINGLE; stats.base.off_subgroup++; }
                else { state[ids[i]] = DONE; verdict[ids[i]] = VERIFIER_INVALID_PROOF; }
            }
            lap(PHASE_SUBGROUP);
            if (kept.empty()) continue;
            const bool in_place = kept.size() == m;
            run_pass(kept.data(), kept.size(), in_place ? &g_trace.in_place : &g_trace.gathered,
                     [&](Forest& forest, std::vector<Pass>&, const u32* r, double kernel_ms[3]) {
                rb.plan = device_plan(forest);
                rb.run(consts(), in_place ? nullptr : keep.data(), (int)kept.size(), r, forest.f_tree.data(), forest.g_tree.data(), kernel_ms);
                return rb.tree_launches;
            });
        }
    }
    // 4. whatever is left: to the judge when it is on and the suspects are many enough (never under a key the batch refused),
    //    else to verify_one on the host threads. Proofs that stayed on the device are rebuilt from the raw records first.
    void decide_singles() {
        std::vector<size_t> singles;
        for (size_t i = 0; i < n; i++) if (state[i] == SINGLE) singles.push_back(i);
        if (resident) parallel_for(singles.size(), [&](size_t s) { src.parse(singles[s], parsed[singles[s]], key_for(singles[s]).ic.size(), true); });
        std::vector<size_t> suspects, rest;                         // suspects: under a key the batch takes; the judge's, all keys in one launch
        for (size_t i : singles) (key_ok[key_index(i)] ? suspects : rest).push_back(i);
        if (opt.judge && !suspects.empty() && suspects.size() >= (size_t)opt.judge_min) {
            group_by_key(suspects);
            std::vector<char> valid;
            judge_suspects(keys, key_of, device, parsed, suspects, valid, stats);
            for (size_t s = 0; s < suspects.size(); s++) verdict[suspects[s]] = valid[s] ? VERIFIER_VALID_PROOF : VERIFIER_INVALID_PROOF;
            singles.swap(rest);
        }
        parallel_for(singles.size(), [&](size_t s) {
            const size_t i = singles[s];
            if (!message[i].empty()) return;                        // (it did not parse)
            try { verdict[i] = verify_one(key_for(i), parsed[i]); }
            catch (std::exception& e) { message[i] = e.what(); }
        });
        stats.base.single_checks = singles.size();
        lap(PHASE_SINGLES);
    }
    int finish(int* verdicts, char* error_msg, unsigned long error_msg_maxsize) {
        { std::lock_guard<std::mutex> lock(g_trace.m); for (int k = 0; k < PHASES; k++) g_trace.phase_ms[k] = phase[k]; }
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
        stats.base.host_ms = ms_since(t_start) - stats.base.device_ms;
        return rc;
    }
};

// ULTRAGROTH_VERIFY_JUDGE when the caller gives no options (the calls without an options argument never do)
BatchOptions read_options(const ug_verify_batch_options* options) {
    BatchOptions opt;
    if (!options) { opt.judge = judge_from_environment(); return opt; }
    if (options->size < sizeof(ug_verify_batch_options)) throw std::invalid_argument("ug_verify_batch_options: size is smaller than the struct");
    if (options->judge != 0 && options->judge != 1) throw std::invalid_argument("ug_verify_batch_options: judge must be 0 or 1");
    opt.judge = options->judge == 1;
    if (options->search_width >= 0) opt.search_width = options->search_width;
    if (options->judge_min >= 0) opt.judge_min = options->judge_min;
    return opt;
}
// The one route of the exported batch calls. stats / legacy_stats: the call's statistics and their first 40 bytes, the struct of the
// calls without options; either may be null, and neither is written by a call that fails.
int batch_entry(int device, const Source& src, int count, const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                ug_verify_batch_stats_ex* stats, ug_verify_batch_stats* legacy_stats, char* error_msg, unsigned long error_msg_maxsize) {
    return guarded(error_msg, error_msg_maxsize, [&] {
        const BatchOptions opt = read_options(options);
        src.check(count, count < 0 || !verification_key || (count > 0 && !verdicts));
        BatchCall call(src, device, (size_t)count, &verification_key, 1, false, nullptr, opt);
        const int rc = call.run(verdicts, error_msg, error_msg_maxsize);
        if (stats) *stats = call.stats;
        if (legacy_stats) *legacy_stats = call.stats.base;
        return rc;
    });
}
// The route of the _keys calls: the same call under n_keys keys. n_pub: the records calls' inputs per proof of every key (texts: null).
// The order of the tests is the order of the messages (include/verifier.h).
int keys_entry(int device, Source& src, int count, int n_keys, const char* const* keys, const int* key_of, const int* n_pub, int* verdicts,
               const ug_verify_batch_options* options, ug_verify_batch_stats_keys* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return guarded(error_msg, error_msg_maxsize, [&] {
        const BatchOptions opt = read_options(options);
        src.keyed = true;                                           // (RecordSource::check then asks no n_pub of its own)
        bool null_argument = count < 0 || n_keys < 0 || (count > 0 && (!verdicts || !key_of)) || (n_keys > 0 && (!keys || (src.records_call && !n_pub)));
        for (int q = 0; !null_argument && q < n_keys; q++) null_argument = !keys[q];
        src.check(count, null_argument);
        if (count > 0 && n_keys <= 0) throw std::invalid_argument("n_keys: a call with proofs needs at least one key");
        for (int i = 0; i < count; i++)
            if (key_of[i] < 0 || key_of[i] >= n_keys) throw std::invalid_argument("proof " + std::to_string(i) + ": key index " + std::to_string(key_of[i]) + " out of range");
        if (src.records_call) {
            for (int q = 0; q < n_keys; q++) if (n_pub[q] <= 0) throw std::invalid_argument("key " + std::to_string(q) + ": invalid inputs data");
            src.ragged(key_of, n_pub, (size_t)n_keys, (size_t)count);
        }
        BatchCall call(src, device, (size_t)count, keys, (size_t)n_keys, true, count > 0 ? key_of : nullptr, opt);
        const int rc = call.run(verdicts, error_msg, error_msg_maxsize);
        if (stats) {
            stats->ex = call.stats;
            stats->segments = call.segments; stats->tree_launches = call.tree_launches; stats->key_checks = call.key_checks;
        }
        return rc;
    });
}

}  // namespace

extern "C" {

int ug_groth16_verify_batch(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                            int* verdicts, ug_verify_batch_stats* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return batch_entry(device, JsonSource(false, proofs, inputs), count, verification_key, verdicts, nullptr, nullptr, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                int* verdicts, ug_verify_batch_stats* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return batch_entry(device, JsonSource(true, proofs, inputs), count, verification_key, verdicts, nullptr, nullptr, stats, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_opt(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                unsigned long error_msg_maxsize) {
    return batch_entry(device, JsonSource(false, proofs, inputs), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_opt(int device, int count, const char* const* proofs, const char* const* inputs, const char* verification_key,
                                    int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                    unsigned long error_msg_maxsize) {
    return batch_entry(device, JsonSource(true, proofs, inputs), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_records(int device, int count, const void* records, const void* inputs, int n_pub, const char* verification_key,
                                    int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                    unsigned long error_msg_maxsize) {
    return batch_entry(device, RecordSource(false, RECORDS_PLAIN, records, inputs, n_pub), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_records(int device, int count, const void* records, const void* inputs, int n_pub, const char* verification_key,
                                        int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_ex* stats, char* error_msg,
                                        unsigned long error_msg_maxsize) {
    return batch_entry(device, RecordSource(true, RECORDS_PLAIN, records, inputs, n_pub), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_records_fmt(int device, int format, int count, const void* records, const void* inputs, int n_pub,
                                        const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                                        ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return batch_entry(device, RecordSource(false, format, records, inputs, n_pub), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_records_fmt(int device, int format, int count, const void* records, const void* inputs, int n_pub,
                                            const char* verification_key, int* verdicts, const ug_verify_batch_options* options,
                                            ug_verify_batch_stats_ex* stats, char* error_msg, unsigned long error_msg_maxsize) {
    return batch_entry(device, RecordSource(true, format, records, inputs, n_pub), count, verification_key, verdicts, options, stats, nullptr, error_msg, error_msg_maxsize);
}

int ug_groth16_verify_batch_keys(int device, int count, const char* const* proofs, const char* const* inputs, int n_keys, const char* const* keys,
                                 const int* key_of, int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_keys* stats, char* error_msg,
                                 unsigned long error_msg_maxsize) {
    JsonSource src(false, proofs, inputs);
    return keys_entry(device, src, count, n_keys, keys, key_of, nullptr, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_keys(int device, int count, const char* const* proofs, const char* const* inputs, int n_keys, const char* const* keys,
                                     const int* key_of, int* verdicts, const ug_verify_batch_options* options, ug_verify_batch_stats_keys* stats,
                                     char* error_msg, unsigned long error_msg_maxsize) {
    JsonSource src(true, proofs, inputs);
    return keys_entry(device, src, count, n_keys, keys, key_of, nullptr, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_groth16_verify_batch_records_keys(int device, int format, int count, const void* records, const void* inputs, int n_keys, const char* const* keys,
                                         const int* key_of, const int* n_pub, int* verdicts, const ug_verify_batch_options* options,
                                         ug_verify_batch_stats_keys* stats, char* error_msg, unsigned long error_msg_maxsize) {
    RecordSource src(false, format, records, inputs, 0);
    return keys_entry(device, src, count, n_keys, keys, key_of, n_pub, verdicts, options, stats, error_msg, error_msg_maxsize);
}
int ug_ultra_groth_verify_batch_records_keys(int device, int format, int count, const void* records, const void* inputs, int n_keys,
                                             const char* const* keys, const int* key_of, const int* n_pub, int* verdicts,
                                             const ug_verify_batch_options* options, ug_verify_batch_stats_keys* stats, char* error_msg,
                                             unsigned long error_msg_maxsize) {
    RecordSource src(true, format, records, inputs, 0);
    return keys_entry(device, src, count, n_keys, keys, key_of, n_pub, verdicts, options, stats, error_msg, error_msg_maxsize);
}

// ULTRAGROTH_TEST_HOOKS=1 only: the forest over given leaves -- n_segments segments of sizes[] leaves, leaves_f n x 108 words and
// leaves_g n x k x 36 (canonical values, as the Miller kernel leaves them) -- by the forest kernels alone on `device`, by the host
// forest for device < 0. f_tree_out / g_tree_out: the whole forest in ForestPlan's layout, nodes x 108 and nodes x k x 36 words.
int ug_test_tree_forest(int device, int k, int n_segments, const int* sizes, const unsigned int* leaves_f, const unsigned int* leaves_g,
                        unsigned int* f_tree_out, unsigned int* g_tree_out) {
    if (!ughost::testHooksEnabled() || !sizes || !leaves_f || !leaves_g || !f_tree_out || !g_tree_out || n_segments <= 0 || (k != 1 && k != 2)) return 1;
    try {
        std::vector<u32> sz;
        size_t n = 0;
        for (int s = 0; s < n_segments; s++) {
            if (sizes[s] <= 0) return 1;
            sz.push_back((u32)sizes[s]);
            n += (size_t)sizes[s];
        }
        if (n > (size_t)PAIRING_PASS) return 1;
        Forest forest(sz, k);
        if (device < 0) {
            memcpy(forest.f_tree.data(), leaves_f, n * F12_WORDS * sizeof(u32));
            memcpy(forest.g_tree.data(), leaves_g, n * (size_t)k * XYZZ_WORDS * sizeof(u32));
            Key none;                                               // (the trees ask nothing of a key)
            none.ultra = k == 2;
            std::vector<Pass> segs;
            segs.reserve(sz.size());
            for (size_t s = 0; s < sz.size(); s++) segs.emplace_back(none, forest, s);
            host_forest(segs);
        } else {
            PairingBatch pb;
            pb.n = (int)n; pb.k = k; pb.plan = &forest.plan; pb.leaf_f = leaves_f; pb.leaf_g = leaves_g;
            pb.f_tree = forest.f_tree.data(); pb.g_tree = forest.g_tree.data();
            pairing_batch_device(device, consts(), pb);
        }
        memcpy(f_tree_out, forest.f_tree.data(), forest.f_tree.size() * sizeof(u32));
        memcpy(g_tree_out, forest.g_tree.data(), forest.g_tree.size() * sizeof(u32));
        return 0;
    } catch (...) { return 1; }
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
        for (size_t first = 0; first < (size_t)count; first += PAIRING_PASS) {
            const size_t m = std::min<size_t>(PAIRING_PASS, (size_t)count - first);
            std::vector<u32> a(m * G1_WORDS), b(m * G2_WORDS), g(m * (size_t)k * G1_WORDS);
            if (device < 0) {
                std::vector<BatchProof> read(m);
                parallel_for(m, [&](size_t j) {
                    BatchProof& p = read[j];
                    p.no_point = !record_read(format, ultra, rec + (first + j) * stride, p);
                    status[first + j] = !proof_on_curve(p) ? UG_POINT_OFF_CURVE : g2_in_subgroup(p.b) ? UG_POINT_OK : UG_POINT_OFF_SUBGROUP;
                });
                pack_points(read, nullptr, m, k, a.data(), b.data(), g.data());
            } else {
                ResidentBatch rb(device, (int)m, k, format);
                rb.ingest(rec + first * stride, status + first);
                rb.download(a.data(), b.data(), g.data());
            }
            parallel_for(m, [&](size_t j) {                         // the arrays as plain records; what failed is zeros
                Points pts;
                pts.a = g1_load(&a[j * G1_WORDS], false);
                pts.b = g2_load(&b[j * G2_WORDS]);
                for (int s = 0; s < 2; s++) pts.g[s] = s < k ? g1_load(&g[(j * k + s) * G1_WORDS], false) : g1_inf();
                if (!g1_on_curve(pts.a)) pts.a = g1_inf();
                if (!g2_on_curve(pts.b)) pts.b = g2_inf();
                for (int s = 0; s < 2; s++) if (!g1_on_curve(pts.g[s])) pts.g[s] = g1_inf();
                record_write(RECORDS_PLAIN, ultra, pts, out + (first + j) * plain);
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
