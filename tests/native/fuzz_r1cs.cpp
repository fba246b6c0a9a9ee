// fuzz_r1cs.cpp -- CPU-only robustness harness for the .r1cs reader of the product (ultragroth_amd/csrc/host_util.cpp: BinFile,
// loadR1csHeader, countR1csTerms, loadR1cs), built with -fsanitize=address,undefined by tests/test_r1cs_parser_sanitized.py.
// An .r1cs handed to a proving service is untrusted input: whatever bytes arrive, parsing must end in a normal return or a
// C++ exception -- never in an out-of-bounds access.
//
// usage: fuzz_r1cs <file> <iterations> <seed>
// Mutations of the given file: bit flips in the header section and anywhere in the constraints, term counts and wire ids
// replaced by extreme values, truncations, section sizes replaced by extreme values. After a successful parse every offset
// and every term of the three CSR triples is read, which is what trips the sanitizer if a count lies.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include "fuzz_kit.hpp"
#include "host_util.hpp"

using namespace ughost;
using namespace fuzz;

static volatile uint64_t sink;

static int parse(const std::vector<uint8_t>& buf) {
    try {
        BinFile f(buf.data(), buf.size(), "r1cs", 1);
        R1cs cs;
        loadR1cs(f, cs);
        uint64_t sum = 0;
        for (int m = 0; m < 3; m++) {
            const R1csMatrix& M = cs.m[m];
            if (M.rowPtr.size() != (size_t)cs.hdr.nConstraints + 1 || M.rowPtr.back() != cs.terms[m]) abort();
            for (uint32_t k = 0; k < cs.hdr.nConstraints; k++) {
                if (M.rowPtr[k] > M.rowPtr[k + 1]) abort();
                for (uint32_t p = M.rowPtr[k]; p < M.rowPtr[k + 1]; p++) {
                    if (M.sig[p] >= cs.hdr.nWires) abort();
                    sum += M.sig[p] + M.val[(size_t)p * 32] + M.val[(size_t)p * 32 + 31];
                }
            }
        }
        sink = sum;
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_r1cs <file> <iterations> <seed>\n"); return 2; }
    const std::vector<uint8_t> orig = readFile(argv[1]);
    const long iters = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10);
    if (parse(orig) != 0) { fprintf(stderr, "the unmodified file does not parse\n"); return 3; }
    // the section headers of the original file and the payload of sections 1 and 2
    const std::vector<SectionAt> secs = walkSections(orig);
    const std::vector<size_t> hdrs = headerOffsets(secs);
    const SectionAt *sec1 = findSection(secs, 1), *sec2 = findSection(secs, 2);
    if (!sec1 || !sec2 || sec2->size < 16) { fprintf(stderr, "sections 1 and 2 not found\n"); return 3; }
    const size_t s1 = sec1->header + 12, s2 = sec2->header + 12, s2len = (size_t)sec2->size;
    const uint64_t extremes[] = {0, 1, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffe8ull};
    const uint32_t extremes32[] = {0, 1, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x071c71c7u, 0x071c71c8u};      // (2^32 / 36 and its neighbour)
    mutateAndParse(orig, iters, [&](std::vector<uint8_t>& buf) {
        switch (rnd() % 6) {
            case 0: flipBits(buf, s1, 64, 3); break;               // in the header section (n8, prime, counts)
            case 1: flipBits(buf, s2, s2len, 4); break;            // anywhere in the constraints (term counts, wire ids, coefficients)
            case 2: truncate(buf); break;
            case 3: replaceSectionSize(buf, hdrs, extremes); break;
            case 4: {                                  // a header count (nWires .. nConstraints) replaced by an extreme value
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])] + (uint32_t)(rnd() % 3) - 1;
                const size_t field[] = {36, 40, 44, 48, 60};
                memcpy(buf.data() + s1 + field[rnd() % 5], &v, 4);
                break;
            }
            default: {                                 // a word somewhere in the constraints replaced by an extreme value (on a
                                                       // 4-byte grid from the section's start: the first word is a term count)
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])] + (uint32_t)(rnd() % 3) - 1;
                size_t o = (rnd() % 8 == 0) ? 0 : (rnd() % (s2len / 4)) * 4;
                memcpy(buf.data() + s2 + o, &v, 4);
                break;
            }
        }
    }, [](const std::vector<uint8_t>& buf) { return parse(buf); });
    return 0;
}
