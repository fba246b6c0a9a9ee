// fuzz_ptau_prepare.cpp -- CPU-only robustness harness for what the powers-of-tau preparation reads of a file
// (ultragroth_amd/csrc/host_util.cpp: BinFile and its section order, loadPtauHeader, loadPtauPowers, loadPtauLagrange), built with
// -fsanitize=address,undefined by tests/test_ptau_prepare_host.py.
// A .ptau is a download: whatever bytes arrive, parsing must end in a normal return or a C++ exception -- never in an
// out-of-bounds access.
//
// usage: fuzz_ptau_prepare <unprepared file> <iterations> <seed>
// Mutations of the given file: bit flips in the header section and in the point data, the power replaced by extreme values,
// truncations, section sizes, ids and the section count replaced by extreme values. After a successful parse every byte of every
// slice the reader hands out is read -- the powers of every cut the file allows, every section in file order (what a prepared
// file copies), the Lagrange sections when a mutation makes some appear -- which is what trips the sanitizer if a size lies. The
// buffer is an exact-size heap block, so one byte past the end is caught.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <memory>
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

static uint64_t touch(const uint8_t* p, uint64_t n) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; i++) s += p[i];
    return s;
}

// 0: the header parsed and the powers of at least one cut were handed out and read; 1: refused
static int parse(const uint8_t* data, size_t size) {
    try {
        BinFile f(data, size, "ptau", 1);
        uint64_t sum = 0;
        for (const auto& s : f.inOrder()) sum += touch(s.second.start, s.second.size);
        const PtauHeader h = loadPtauHeader(f);
        if (h.n8 != 32 || h.power > 28) abort();
        int served = 0;
        for (uint32_t p = 0; p <= h.power + 1 && p <= 12; p++) {      // (a mutated power may claim 2^28: the file never holds it)
            try {
                const PtauPowers s = loadPtauPowers(f, h, p);
                if (s.power != (p ? p : h.power) || s.n != (1ull << s.power)) abort();
                sum += touch(s.tau1, (2 * s.n - 1) * 64) + touch(s.tau2, s.n * 128) + touch(s.alphaTau1, s.n * 64) + touch(s.betaTau1, s.n * 64);
                served++;
            } catch (const std::exception&) {
            }
        }
        if (h.power <= 12) {
            try {
                const PtauLagrange l = loadPtauLagrange(f, h);
                const uint64_t n = 1ull << h.power;
                sum += touch(l.sec[0], (4 * n - 1) * 64) + touch(l.sec[1], (2 * n - 1) * 128) + touch(l.sec[2], (2 * n - 1) * 64) + touch(l.sec[3], (2 * n - 1) * 64);
            } catch (const std::exception&) {
            }
        }
        sink = sum;
        return served ? 0 : 1;
    } catch (const std::exception&) {
        return 1;
    }
}

static int parse(const std::vector<uint8_t>& buf) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[buf.size() ? buf.size() : 1]);
    if (!buf.empty()) memcpy(exact.get(), buf.data(), buf.size());
    return parse(exact.get(), buf.size());
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_ptau_prepare <file> <iterations> <seed>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<uint8_t> orig((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const long iters = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10);
    if (orig.size() < 12 || parse(orig) != 0) { fprintf(stderr, "the unmodified file does not parse\n"); return 3; }
    std::vector<size_t> hdrs;                   // offsets of the section headers (id u32, size u64 at +4)
    size_t s1 = 0;
    {
        uint32_t n; memcpy(&n, orig.data() + 8, 4);
        size_t pos = 12;
        for (uint32_t i = 0; i < n && pos + 12 <= orig.size(); i++) {
            hdrs.push_back(pos);
            uint32_t id; memcpy(&id, orig.data() + pos, 4);
            uint64_t sz; memcpy(&sz, orig.data() + pos + 4, 8);
            if (id == 1) s1 = pos + 12;
            pos += 12 + sz;
        }
    }
    if (!s1 || hdrs.empty()) { fprintf(stderr, "section 1 not found\n"); return 3; }
    const uint64_t extremes[] = {0, 1, 63, 64, 127, 128, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffc0ull};
    const uint32_t extremes32[] = {0, 1, 5, 6, 7, 27, 28, 29, 31, 32, 63, 64, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    long ok = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> buf = orig;
        switch (rnd() % 7) {
            case 0: {                                  // bit flips in the header section (n8, prime, power, ceremonyPower)
                int k = 1 + (int)(rnd() % 3);
                for (int j = 0; j < k; j++) buf[s1 + rnd() % 44] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 1: {                                  // bit flips anywhere (the reader never looks inside a point)
                int k = 1 + (int)(rnd() % 4);
                for (int j = 0; j < k; j++) buf[12 + rnd() % (buf.size() - 12)] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 2: buf.resize(rnd() % (buf.size() + 1)); break;           // truncation
            case 3: {                                  // a section size replaced by an extreme value (+- a small offset)
                size_t h = hdrs[rnd() % hdrs.size()];
                uint64_t v = extremes[rnd() % (sizeof extremes / sizeof extremes[0])] + (rnd() % 3) - 1;
                memcpy(buf.data() + h + 4, &v, 8);
                break;
            }
            case 4: {                                  // the power or the ceremony power replaced
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])];
                memcpy(buf.data() + s1 + (rnd() % 2 ? 36 : 40), &v, 4);
                break;
            }
            case 5: {                                  // a section id replaced: a section goes missing, another appears twice or as 12 - 15
                size_t h = hdrs[rnd() % hdrs.size()];
                uint32_t v = (uint32_t)(rnd() % 18);
                memcpy(buf.data() + h, &v, 4);
                break;
            }
            default: {                                 // the section count replaced
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])];
                memcpy(buf.data() + 8, &v, 4);
                break;
            }
        }
        if (parse(buf) == 0) ok++; else rejected++;
    }
    printf("%ld parsed, %ld rejected, 0 crashed\n", ok, rejected);
    return 0;
}
