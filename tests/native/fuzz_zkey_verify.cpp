// fuzz_zkey_verify.cpp -- CPU-only robustness harness for the key check on host threads (ultragroth_amd/csrc/zkey_verify_host.cpp with
// setup_ptau.cpp, point_check.cpp, setup_host.cpp and host_util.cpp: ug_zkey_verify_run, device = -1), built with -fsanitize=address,undefined by
// tests/test_zkey_verify_host.py. No HIP code is linked: the four device calls the point check names are stubs that abort.
// A key, a .ptau and an .r1cs are downloads: whatever bytes arrive, the call must end with one of its three answers -- valid,
// invalid, refused -- never in an out-of-bounds access.
//
// usage: fuzz_zkey_verify <circuit.r1cs> <prepared.ptau> <key.zkey> <iterations> <seed>
// Each turn mutates ONE of the three files: bit flips anywhere, bit flips in a header section, a truncation, a section size, a
// section id or the section count replaced by an extreme value. The buffers are exact-size heap blocks, so one byte past an end
// is caught. The unmodified triple must be valid.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fuzz_kit.hpp"
#include "../../include/ultragroth_hip.h"

using namespace fuzz;

extern "C" {
// (point_check.cpp reaches these for device >= 0 only)
int ug_ctx_create(ug_ctx**, int) { abort(); }
void ug_ctx_destroy(ug_ctx*) { abort(); }
int ug_points_check(ug_ctx*, int, const void*, uint64_t, int, ug_point_fault*) { abort(); }
const char* ug_last_error(void) { abort(); }
}

// UG_OK, UG_ZKEY_INVALID or UG_ERROR
static int verify(const std::vector<uint8_t> file[3]) {
    const Exact r1cs(file[0]), ptau(file[1]), zkey(file[2]);
    ug_zkey_verify_options opt;
    memset(&opt, 0, sizeof opt);
    opt.size = sizeof opt;
    opt.validate = 2;
    ug_zkey_verify_report rep;
    double ms[UG_ZKEY_VERIFY_PHASES];
    char message[256];
    const int rc = ug_zkey_verify_run(&opt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, zkey.p.get(), zkey.n, -1, &rep, ms, message, sizeof message);
    if (rc != UG_OK && rc != UG_ZKEY_INVALID && rc != UG_ERROR) abort();
    if ((rc == UG_ZKEY_INVALID) != (rep.failed_sections != 0)) abort();
    if (rc != UG_OK && !message[0]) abort();
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: fuzz_zkey_verify <r1cs> <ptau> <zkey> <iterations> <seed>\n"); return 2; }
    const std::vector<uint8_t> orig[3] = {readFile(argv[1]), readFile(argv[2]), readFile(argv[3])};
    const long iters = atol(argv[4]);
    rng_state = strtoull(argv[5], nullptr, 10);
    for (const auto& f : orig)
        if (f.size() < 24) { fprintf(stderr, "a file is missing or too short\n"); return 3; }
    if (verify(orig) != UG_OK) { fprintf(stderr, "the unmodified triple is not valid\n"); return 3; }
    // .r1cs: sections 1, 2; .ptau: 1, 4, 5, 6, 12 - 15; .zkey: 1 - 9
    const uint32_t readIds[3] = {0x6u, 0xf072u, 0x3feu};
    std::vector<size_t> hdrs[3];
    for (int i = 0; i < 3; i++) {
        hdrs[i] = headerOffsets(walkSections(orig[i]), readIds[i]);
        if (hdrs[i].empty()) { fprintf(stderr, "no sections found\n"); return 3; }
    }
    const uint64_t extremes[] = {0, 1, 43, 44, 63, 64, 127, 128, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffc0ull};
    const uint32_t extremes32[] = {0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 64, 1337, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    long count[3] = {0, 0, 0};
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> file[3] = {orig[0], orig[1], orig[2]};
        const int which = (int)(rnd() % 3);
        std::vector<uint8_t>& buf = file[which];
        const std::vector<size_t>& hd = hdrs[which];
        // (a turn that reaches the pairings costs a hundred times one that is refused by a size rule, and most bytes of a .ptau are
        // never read: the mutations aimed at the sections the check reads get most of the turns)
        static const int kinds[16] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6};
        switch (kinds[rnd() % 16]) {
            case 0: flipBits(buf, 12, buf.size() - 12, 3); break;          // anywhere: mostly inside a point or a coefficient
            case 1: {                                  // a bit flip at the start of a section: the headers' fields, the counts
                size_t h = hd[rnd() % hd.size()];
                uint64_t sz;
                memcpy(&sz, buf.data() + h + 4, 8);
                if (sz) flipBit(buf, h + 12, sz < 96 ? sz : 96);
                break;
            }
            case 2: truncate(buf); break;
            case 3: replaceSectionSize(buf, hd, extremes); break;
            case 4: {                                  // a u32 among the first words of a section replaced (n8, nVars, nPublic, domain, power, counts)
                size_t h = hd[rnd() % hd.size()];
                uint64_t sz;
                memcpy(&sz, buf.data() + h + 4, 8);
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])];
                if (sz >= 4) memcpy(buf.data() + h + 12 + 4 * (rnd() % (sz / 4 < 24 ? sz / 4 : 24)), &v, 4);
                break;
            }
            case 5: replaceSectionId(buf, hd); break;                      // a section goes missing, another appears twice
            default: replaceWord(buf, 8, extremes32); break;               // the section count
        }
        count[verify(file)]++;
    }
    printf("%ld valid, %ld invalid, %ld refused, 0 crashed\n", count[UG_OK], count[UG_ZKEY_INVALID], count[UG_ERROR]);
    return 0;
}
