// record_formats_main.cpp -- CPU-only harness for the host code of the record layouts (include/verifier.h): the square roots and
// decompression of pairing.hpp and the conversions of verifier_api.cpp, built with -fsanitize=address,undefined by
// tests/test_formats_sanitized.py together with verifier_api.cpp and host_util.cpp. Records are untrusted bytes of a service: whatever
// arrives, a conversion must end in one of its three return codes and a batch call in verdicts -- never in an out-of-bounds access or
// undefined arithmetic.
//
// usage: record_formats_main <verification_key.json> <iterations> <seed>
// Random compressed records (most x have a y for about half of the points), their round trips through all three layouts, random
// bytes in every layout, input blocks, f2_sqrt of random and degenerate values, and a batch call with device = -1 over the lot.
// The device entry points verifier_api.cpp links against are stubs that throw: nothing here may reach them.
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
static void fail(const char* what) { fprintf(stderr, "record_formats_main: %s\n", what); exit(1); }

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s <verification_key.json> <iterations> <seed>\n", argv[0]); return 2; }
    setenv("ULTRAGROTH_TEST_HOOKS", "1", 1);
    std::ifstream f(argv[1]);
    std::stringstream key;
    key << f.rdbuf();
    const int iterations = atoi(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10);
    unsigned long converted = 0, refused = 0;
    std::vector<uint8_t> batch;                                     // compressed Groth16 records for the batch call
    for (int it = 0; it < iterations; it++) {
        for (int ultra = 0; ultra < 2; ultra++) {
            // exact-size heap buffers: a byte past a record is the sanitizer's to see
            std::vector<uint8_t> comp(ug_proof_record_bytes(ultra, UG_RECORDS_COMPRESSED));
            fill(comp.data(), comp.size());
            const size_t ends[4] = {31, 95, 127, 159};
            for (int p = 0; p < 3 + ultra; p++) {                   // flags: mostly a sign, sometimes infinity
                comp[ends[p]] &= 0xbf;
                if (rnd() % 16 == 0) comp[ends[p]] |= 0x40;
            }
            if (!ultra) batch.insert(batch.end(), comp.begin(), comp.end());
            std::vector<uint8_t> plain(ug_proof_record_bytes(ultra, UG_RECORDS_PLAIN)), evm(plain.size()), back(comp.size()), again(plain.size());
            const int rc = ug_proof_record_convert(ultra, UG_RECORDS_COMPRESSED, comp.data(), UG_RECORDS_PLAIN, plain.data());
            if (rc == 1) { refused++; continue; }
            if (rc != 0) fail("COMPRESSED -> PLAIN: unexpected return code");
            converted++;
            if (ug_proof_record_convert(ultra, UG_RECORDS_PLAIN, plain.data(), UG_RECORDS_COMPRESSED, back.data()) != 0) fail("PLAIN -> COMPRESSED refused a decompressed record");
            if (ug_proof_record_convert(ultra, UG_RECORDS_COMPRESSED, back.data(), UG_RECORDS_PLAIN, again.data()) != 0 || again != plain) fail("round trip through COMPRESSED");
            if (ug_proof_record_convert(ultra, UG_RECORDS_PLAIN, plain.data(), UG_RECORDS_EVM, evm.data()) != 0) fail("PLAIN -> EVM");
            if (ug_proof_record_convert(ultra, UG_RECORDS_EVM, evm.data(), UG_RECORDS_PLAIN, again.data()) != 0 || again != plain) fail("round trip through EVM");
            if (ug_proof_record_convert(ultra, UG_RECORDS_EVM, evm.data(), UG_RECORDS_COMPRESSED, evm.data()) != 0) fail("EVM -> COMPRESSED in place");
            if (memcmp(evm.data(), back.data(), back.size()) != 0) fail("EVM -> COMPRESSED differs from PLAIN -> COMPRESSED");
        }
        for (int from = 0; from < 3; from++)                        // random bytes in every layout: any of the three codes, no more
            for (int to = 0; to < 3; to++) {
                std::vector<uint8_t> a(ug_proof_record_bytes(it & 1, from)), b(ug_proof_record_bytes(it & 1, to));
                fill(a.data(), a.size());
                const int rc = ug_proof_record_convert(it & 1, from, a.data(), to, b.data());
                if (rc < 0 || rc > 1) fail("random record: unexpected return code");
            }
        std::vector<uint8_t> in(32 * (1 + it % 3)), out(in.size());
        fill(in.data(), in.size());
        if (ug_inputs_convert(UG_RECORDS_PLAIN, in.data(), (int)(in.size() / 32), UG_RECORDS_EVM, out.data()) != 0) fail("inputs");
        if (ug_inputs_convert(UG_RECORDS_EVM, out.data(), (int)(in.size() / 32), UG_RECORDS_COMPRESSED, out.data()) != 0 || out != in) fail("inputs round trip");
    }
    // f2_sqrt: degenerate values first (zero, real, purely imaginary, values at and above q), then random ones and their squares' kin
    std::vector<uint8_t> vals(64 * (8 + (size_t)iterations), 0), roots(vals.size()), has(vals.size() / 64);
    vals[64 * 1] = 4; vals[64 * 2] = 5; vals[64 * 3 + 32] = 1; vals[64 * 4 + 32] = 7;
    memset(&vals[64 * 5], 0xff, 64); memset(&vals[64 * 6], 0xff, 32); memset(&vals[64 * 7 + 32], 0xff, 32);
    fill(&vals[64 * 8], 64 * (size_t)iterations);
    if (ug_test_fq2_sqrt(-1, (int)has.size(), vals.data(), roots.data(), has.data()) != 0) fail("ug_test_fq2_sqrt");
    unsigned long with_root = 0;
    for (uint8_t h : has) with_root += h;
    // a batch call on the host threads over the compressed records gathered above, and the ingest hook's host reading of them
    const int count = (int)(batch.size() / 128), n_pub = 2;
    std::vector<uint8_t> inputs((size_t)count * n_pub * 32), plain_out((size_t)count * 256), status(count);
    fill(inputs.data(), inputs.size());
    std::vector<int> verdicts(count, -7);
    char err[256] = {0};
    const int rc = ug_groth16_verify_batch_records_fmt(-1, UG_RECORDS_COMPRESSED, count, batch.data(), inputs.data(), n_pub, key.str().c_str(), verdicts.data(),
                                                       nullptr, nullptr, err, 255);
    if (rc == VERIFIER_ERROR) { fprintf(stderr, "batch call: %s\n", err); return 1; }
    for (int v : verdicts) if (v != VERIFIER_INVALID_PROOF && v != VERIFIER_VALID_PROOF) fail("a verdict is neither VALID nor INVALID");
    if (ug_test_records_ingest(-1, UG_RECORDS_COMPRESSED, 0, count, batch.data(), plain_out.data(), status.data()) != 0) fail("ug_test_records_ingest");
    printf("%lu converted, %lu refused, %lu of %zu values with a root, %d verdicts\n", converted, refused, with_root, has.size(), count);
    return 0;
}
