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
#include <fstream>
#include <string>
#include <vector>
#include "host_util.hpp"

using namespace ughost;

static uint64_t rng_state;
static uint64_t rnd() {                       // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

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
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<uint8_t> orig((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const long iters = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10);
    if (parse(orig) != 0) { fprintf(stderr, "the unmodified file does not parse\n"); return 3; }
    // offsets of the section headers of the original file (type u32, size u64 at +4) and the payload of sections 1 and 2
    std::vector<size_t> hdrs;
    size_t s1 = 0, s2 = 0, s2len = 0;
    {
        uint32_t n; memcpy(&n, orig.data() + 8, 4);
        size_t pos = 12;
        for (uint32_t i = 0; i < n && pos + 12 <= orig.size(); i++) {
            hdrs.push_back(pos);
            uint32_t id; memcpy(&id, orig.data() + pos, 4);
            uint64_t sz; memcpy(&sz, orig.data() + pos + 4, 8);
            if (id == 1) s1 = pos + 12;
            if (id == 2) { s2 = pos + 12; s2len = (size_t)sz; }
            pos += 12 + sz;
        }
    }
    if (!s1 || !s2 || s2len < 16) { fprintf(stderr, "sections 1 and 2 not found\n"); return 3; }
    const uint64_t extremes[] = {0, 1, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffe8ull};
    const uint32_t extremes32[] = {0, 1, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x071c71c7u, 0x071c71c8u};      // (2^32 / 36 and its neighbour)
    long ok = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> buf = orig;
        switch (rnd() % 6) {
            case 0: {                                  // bit flips in the header section (n8, prime, counts)
                int k = 1 + (int)(rnd() % 3);
                for (int j = 0; j < k; j++) buf[s1 + rnd() % 64] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 1: {                                  // bit flips anywhere in the constraints (term counts, wire ids, coefficients)
                int k = 1 + (int)(rnd() % 4);
                for (int j = 0; j < k; j++) buf[s2 + rnd() % s2len] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 2: buf.resize(rnd() % (buf.size() + 1)); break;           // truncation
            case 3: {                                  // a section size replaced by an extreme value (+- a small offset)
                size_t h = hdrs[rnd() % hdrs.size()];
                uint64_t v = extremes[rnd() % (sizeof extremes / sizeof extremes[0])] + (rnd() % 3) - 1;
                memcpy(buf.data() + h + 4, &v, 8);
                break;
            }
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
        if (parse(buf) == 0) ok++; else rejected++;
    }
    printf("%ld parsed, %ld rejected, 0 crashed\n", ok, rejected);
    return 0;
}
