// fuzz_ptau.cpp -- CPU-only robustness harness for the .ptau reader of the product (ultragroth_amd/csrc/host_util.cpp: BinFile,
// loadPtauHeader, loadPtauSlices), built with -fsanitize=address,undefined by tests/test_setup_ptau_host.py.
// A .ptau is a download: whatever bytes arrive, parsing must end in a normal return or a C++ exception -- never in an
// out-of-bounds access.
//
// usage: fuzz_ptau <file> <iterations> <seed>
// Mutations of the given file: bit flips in the header section and in the point data, the power replaced by extreme values,
// truncations, section sizes and ids replaced by extreme values. After a successful parse every byte of every slice the reader
// hands out, for every domain the file claims to serve, is read, which is what trips the sanitizer if a size lies. The buffer
// is an exact-size heap block, so one byte past the end is caught.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>
#include "fuzz_kit.hpp"
#include "host_util.hpp"

using namespace ughost;
using namespace fuzz;

static volatile uint64_t sink;

static uint64_t touch(const uint8_t* p, uint64_t n) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; i++) s += p[i];
    return s;
}

// 0: the header parsed and at least one domain's slices were handed out and read; 1: refused
static int parse(const uint8_t* data, size_t size) {
    try {
        BinFile f(data, size, "ptau", 1);
        const PtauHeader h = loadPtauHeader(f);
        if (h.n8 != 32 || h.power > 28) abort();
        uint64_t sum = 0;
        int served = 0;
        for (uint32_t n = 0; n <= h.power + 1 && n <= 12; n++) {      // (a mutated power may claim 2^28: the file never holds it)
            try {
                const PtauSlices s = loadPtauSlices(f, h, n);
                if (s.n != (1ull << n)) abort();
                sum += touch(s.tau1, s.n * 64) + touch(s.tau2, s.n * 128) + touch(s.alphaTau1, s.n * 64) + touch(s.betaTau1, s.n * 64);
                sum += touch(s.top, 2 * s.n * 64) + touch(s.alpha1, 64) + touch(s.beta1, 64) + touch(s.beta2, 128);
                served++;
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
    const Exact exact(buf);
    return parse(exact.p.get(), exact.n);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_ptau <file> <iterations> <seed>\n"); return 2; }
    const std::vector<uint8_t> orig = readFile(argv[1]);
    const long iters = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10);
    if (orig.size() < 12 || parse(orig) != 0) { fprintf(stderr, "the unmodified file does not parse\n"); return 3; }
    const std::vector<SectionAt> secs = walkSections(orig);
    const std::vector<size_t> hdrs = headerOffsets(secs);
    const SectionAt* sec1 = findSection(secs, 1);
    if (!sec1) { fprintf(stderr, "section 1 not found\n"); return 3; }
    const size_t s1 = sec1->header + 12;
    const uint64_t extremes[] = {0, 1, 63, 64, 127, 128, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffc0ull};
    const uint32_t extremes32[] = {0, 1, 5, 6, 7, 27, 28, 29, 31, 32, 63, 64, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    mutateAndParse(orig, iters, [&](std::vector<uint8_t>& buf) {
        switch (rnd() % 7) {
            case 0: flipBits(buf, s1, 44, 3); break;                       // in the header section (n8, prime, power, ceremonyPower)
            case 1: flipBits(buf, 12, buf.size() - 12, 4); break;          // anywhere (the reader never looks inside a point)
            case 2: truncate(buf); break;
            case 3: replaceSectionSize(buf, hdrs, extremes); break;
            case 4: {                                  // the power or the ceremony power replaced
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])];
                memcpy(buf.data() + s1 + (rnd() % 2 ? 36 : 40), &v, 4);
                break;
            }
            case 5: replaceSectionId(buf, hdrs); break;                    // a section goes missing, another appears twice
            default: replaceWord(buf, 8, extremes32); break;               // the section count
        }
    }, [](const std::vector<uint8_t>& buf) { return parse(buf); });
    return 0;
}
