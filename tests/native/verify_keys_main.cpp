// verify_keys_main.cpp -- CPU-only harness for the calls under several keys (include/verifier.h: ug_*_verify_batch_records_keys,
// ug_*_verify_batch_keys) with device = -1, built with -fsanitize=address,undefined by tests/test_verify_keys_sanitized.py together
// with verifier_api.cpp, verifier_records.cpp and host_util.cpp. Records, inputs, key indices and input counts are a service's
// untrusted values: whatever arrives, a call must end in verdicts or in a clean VERIFIER_ERROR with the verdicts untouched -- never
// in an out-of-bounds access or undefined arithmetic.
//
// usage: verify_keys_main <seed> <count> <ultra_key.json> <ultra n_pub> <groth16_key.json> <n_pub> [<groth16_key.json> <n_pub> ...]
// Random compressed records, three in four with pi_b = infinity and G1 points wherever the random x has a y: about a quarter of them
// are on their curves and enter the batch, where they fail -- so the forest, the search over the keys and inside the segments, the
// judge and the single verifier all run. The input block is ragged and allocated to the byte. The device entry points
// verifier_api.cpp links against are stubs that throw: nothing here may reach them.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "fuzz_kit.hpp"
#include "pairing_dev.hpp"
#include "../../include/ultragroth_hip.h"
#include "../../include/verifier.h"

namespace ug {
void pairing_batch_device(int, const pr::PairingConsts&, PairingBatch&) { throw std::runtime_error("no device in this build"); }
ResidentBatch::ResidentBatch(int, int, int, int) { throw std::runtime_error("no device in this build"); }
ResidentBatch::~ResidentBatch() {}
void ResidentBatch::ingest(const void*, unsigned char*) { throw std::runtime_error("no device in this build"); }
void ResidentBatch::download(u32*, u32*, u32*) { throw std::runtime_error("no device in this build"); }
void ResidentBatch::run(const pr::PairingConsts&, const u32*, int, const u32*, u32*, u32*, double*) { throw std::runtime_error("no device in this build"); }
void pairing_judge_device(int, const pr::FinalExpConsts&, PairingJudge&) { throw std::runtime_error("no device in this build"); }
void final_exp_device(int, const pr::FinalExpConsts&, const u32*, u32*, int*) { throw std::runtime_error("no device in this build"); }
void fq2_sqrt_device(int, const pr::DecompressConsts&, int, const u32*, u32*, unsigned char*) { throw std::runtime_error("no device in this build"); }
}  // namespace ug
extern "C" {
const char* ug_last_error(void) { return "no device in this build"; }
int ug_ctx_create(ug_ctx**, int) { return UG_ERROR; }
void ug_ctx_destroy(ug_ctx*) {}
int ug_points_check_mask(ug_ctx*, int, const void*, uint64_t, int, uint8_t*) { return UG_ERROR; }
}

using fuzz::rnd;
using fuzz::rng_state;
static void fill(uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) p[i] = (uint8_t)rnd(); }
static void fail(const char* what, const char* more = "") { fprintf(stderr, "verify_keys_main: %s %s\n", what, more); exit(1); }
static std::string slurp(const char* path) {
    std::ifstream f(path);
    if (!f) fail("cannot read", path);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static unsigned long calls = 0, errors = 0, verdicts_seen = 0, batched_calls = 0;
static const int SENTINEL = -7;

struct Batch {                                                      // one call's arguments, every buffer of its exact size
    int ultra, format, count;
    std::vector<uint8_t> records, inputs;
    std::vector<int> key_of, n_pub;
    std::vector<const char*> keys;
};

// the call; expect_error: it must be refused with the verdicts untouched, and its message begin with `prefix`
static void call(const Batch& b, const ug_verify_batch_options* opt, bool expect_error, const char* prefix = "") {
    std::vector<int> verdicts((size_t)b.count, SENTINEL);
    ug_verify_batch_stats_keys stats;
    memset(&stats, 0, sizeof stats);
    char err[256] = {0};
    auto fn = b.ultra ? ug_ultra_groth_verify_batch_records_keys : ug_groth16_verify_batch_records_keys;
    const int rc = fn(-1, b.format, b.count, b.records.data(), b.inputs.data(), (int)b.keys.size(), b.keys.data(), b.key_of.data(), b.n_pub.data(),
                      verdicts.data(), opt, &stats, err, 255);
    calls++;
    if (expect_error) {
        if (rc != VERIFIER_ERROR) fail("a call that had to be refused was not:", prefix);
        if (strncmp(err, prefix, strlen(prefix)) != 0) fail("unexpected message:", err);
        for (int v : verdicts) if (v != SENTINEL) fail("a refused call wrote a verdict");
        errors++;
        return;
    }
    if (rc == VERIFIER_ERROR) fail("a well-formed call was refused:", err);
    for (int v : verdicts) {
        if (v != VERIFIER_INVALID_PROOF && v != VERIFIER_VALID_PROOF) fail("a verdict is neither VALID nor INVALID");
        verdicts_seen++;
    }
    if (stats.ex.base.batch_checks) batched_calls++;
    if (stats.ex.base.batch_checks < stats.key_checks || stats.tree_launches != 0) fail("statistics");
}

static Batch make(int ultra, int format, int count, const std::vector<const char*>& keys, const std::vector<int>& n_pub) {
    Batch b;
    b.ultra = ultra; b.format = format; b.count = count; b.keys = keys; b.n_pub = n_pub;
    const size_t stride = ug_proof_record_bytes(ultra, format);
    b.records.resize((size_t)count * stride);
    fill(b.records.data(), b.records.size());
    if (format == UG_RECORDS_COMPRESSED) {
        const size_t ends[4] = {31, 95, 127, 159};
        for (int i = 0; i < count; i++) {
            uint8_t* rec = &b.records[(size_t)i * stride];
            for (int p = 0; p < 3 + ultra; p++) rec[ends[p]] &= 0xbf;
            if (rnd() % 4) rec[ends[1]] |= 0x40;                    // pi_b = infinity: in the subgroup, so the record can be batched
        }
    }
    size_t bytes = 0;
    for (int i = 0; i < count; i++) {                               // interleaved keys, ragged inputs
        b.key_of.push_back((int)(rnd() % keys.size()));
        bytes += (size_t)n_pub[(size_t)b.key_of.back()] * 32;
    }
    b.inputs.resize(bytes);
    fill(b.inputs.data(), b.inputs.size());
    return b;
}

int main(int argc, char** argv) {
    if (argc < 7 || argc % 2 == 0) { fprintf(stderr, "usage: %s <seed> <count> <ultra_key.json> <n_pub> <groth16_key.json> <n_pub> ...\n", argv[0]); return 2; }
    setenv("ULTRAGROTH_TEST_HOOKS", "1", 1);
    rng_state = strtoull(argv[1], nullptr, 10);
    const int count = atoi(argv[2]);
    std::vector<std::string> texts;
    for (int a = 3; a < argc; a += 2) texts.push_back(slurp(argv[a]));
    std::vector<const char*> ultra_keys{texts[0].c_str(), texts[0].c_str()}, keys;
    std::vector<int> ultra_pub{atoi(argv[4]), atoi(argv[4])}, n_pub;
    for (size_t t = 1; t < texts.size(); t++) { keys.push_back(texts[t].c_str()); n_pub.push_back(atoi(argv[4 + 2 * t])); }
    ug_verify_batch_options judge = {sizeof(ug_verify_batch_options), 1, 1, 1};

    for (int format = 0; format < 3; format++)
        for (int ultra = 0; ultra < 2; ultra++) {
            const Batch b = ultra ? make(1, format, count, ultra_keys, ultra_pub) : make(0, format, count, keys, n_pub);
            call(b, nullptr, false);
            call(b, &judge, false);
            Batch one = b;                                          // every proof under the last key alone: one segment
            one.keys.resize(1); one.n_pub.resize(1);
            one.key_of.assign((size_t)count, 0);
            one.inputs.resize((size_t)count * (size_t)one.n_pub[0] * 32);
            fill(one.inputs.data(), one.inputs.size());
            call(one, nullptr, false);
        }
    const Batch good = make(0, UG_RECORDS_COMPRESSED, count, keys, n_pub);
    const int outside[4] = {-1, (int)keys.size(), INT_MAX, INT_MIN};
    for (int v : outside) {                                         // key indices out of range, first, last and in the middle
        for (int at : {0, count / 2, count - 1}) {
            Batch b = good;
            b.key_of[(size_t)at] = v;
            call(b, nullptr, true, "proof ");
        }
    }
    for (size_t q = 0; q < keys.size(); q++) {                      // input counts that do not fit the key
        for (int v : {n_pub[q] + 1, n_pub[q] - 1, 0, -3, INT_MAX, INT_MIN}) {
            if (v == n_pub[q]) continue;
            Batch b = good;
            b.n_pub[q] = v;
            call(b, nullptr, true, "key ");
        }
    }
    {
        Batch b = good;                                             // a key that does not parse; no key at all; an unknown format
        b.keys[keys.size() - 1] = "{\"protocol\": \"groth16\"";
        call(b, nullptr, true, "key ");
        b = good; b.keys.clear(); b.n_pub.clear();
        call(b, nullptr, true, "n_keys");
        b = good; b.format = 7;
        call(b, nullptr, true, "format");
        b = good; b.count = 0; b.records.clear(); b.inputs.clear(); b.key_of.clear();
        b.records.resize(1); b.inputs.resize(1);
        call(b, nullptr, false);
    }
    {
        char err[256] = {0};                                        // null arguments, and texts that are no JSON under two keys
        int v[2] = {SENTINEL, SENTINEL};
        const int ko[2] = {1, 0};
        if (ug_groth16_verify_batch_records_keys(-1, 0, 2, nullptr, nullptr, (int)keys.size(), keys.data(), ko, n_pub.data(), v, nullptr, nullptr, err, 255) != VERIFIER_ERROR)
            fail("null records were not refused");
        const char* proofs[2] = {"{", "[1, 2"};
        const char* pubs[2] = {"[\"1\"]", ""};
        const int rc = ug_groth16_verify_batch_keys(-1, 2, proofs, pubs, (int)keys.size(), keys.data(), ko, v, nullptr, nullptr, err, 255);
        if (rc != VERIFIER_INVALID_PROOF || v[0] != VERIFIER_ERROR || v[1] != VERIFIER_ERROR) fail("texts that do not parse:", err);
        calls += 2;
    }
    printf("%lu calls, %lu refused, %lu verdicts, %lu calls with a batch check\n", calls, errors, verdicts_seen, batched_calls);
    return 0;
}
