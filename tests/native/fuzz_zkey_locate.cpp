// fuzz_zkey_locate.cpp -- CPU-only robustness harness for locating the wrong records of a key on host threads
// (ultragroth_amd/csrc/zkey_verify_host.cpp with setup_ptau.cpp, point_check.cpp, setup_host.cpp and host_util.cpp:
// ug_zkey_locate_run, device = -1), built with -fsanitize=address,undefined by tests/test_zkey_locate_host.py. No HIP code is
// linked: the four device calls the point check names are stubs that abort.
//
// usage: fuzz_zkey_locate <circuit.r1cs> <prepared.ptau> <key.zkey> <iterations> <seed>
// Each turn mutates ONE of the three files. Three turns in sixteen aim at what locating reads -- a record of a point section
// replaced by another valid record or by infinity, two B2 records swapped (a flipped bit inside a point is refused by the point
// check and never gets that far), a byte of the .r1cs' constraints; such a turn runs some twenty pairings under the sanitizers, a
// hundred times the cost of a refusal, so the rest are the cheap ones of fuzz_zkey_verify: truncations, section sizes, ids and the
// section count. The buffers are exact-size heap blocks. Every turn must end in one of the three answers; the verify part of the answer --
// return code, failing sections, first section, message -- must equal ug_zkey_verify_run's on the same bytes; a refusal reports no
// section; every entry names a failing point section, counts within its records, and lists ascending indices below its count.
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

static long located_sections = 0;
static ug_zkey_locate_report located;           // (57 KiB: not on the stack)

// UG_OK, UG_ZKEY_INVALID or UG_ERROR
static int locate(const std::vector<uint8_t> file[3]) {
    const Exact r1cs(file[0]), ptau(file[1]), zkey(file[2]);
    ug_zkey_verify_options vopt;
    memset(&vopt, 0, sizeof vopt);
    vopt.size = sizeof vopt;
    vopt.validate = 2;
    ug_zkey_locate_options opt;
    memset(&opt, 0, sizeof opt);
    opt.size = sizeof opt;
    opt.validate = 2;
    opt.max_listed = (uint32_t)(rnd() % 4);      // 0: the default
    opt.max_blocks = (uint32_t)(rnd() % 3);
    ug_zkey_verify_report vrep, rep;
    double ms[UG_ZKEY_VERIFY_PHASES];
    char vmessage[256] = {0}, message[256] = {0};
    const int vrc = ug_zkey_verify_run(&vopt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, zkey.p.get(), zkey.n, -1, &vrep, ms, vmessage, sizeof vmessage);
    memset(&located, 0xff, sizeof located);
    const int rc = ug_zkey_locate_run(&opt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, zkey.p.get(), zkey.n, -1, &rep, &located, ms, message, sizeof message);
    if (rc != UG_OK && rc != UG_ZKEY_INVALID && rc != UG_ERROR) abort();
    if (rc != vrc || rep.failed_sections != vrep.failed_sections || rep.first_failed != vrep.first_failed || strcmp(message, vmessage)) abort();
    if (rc != UG_ZKEY_INVALID && located.n_sections) abort();
    if (located.n_sections > UG_ZKEY_LOCATE_SECTIONS) abort();
    const uint32_t listed = opt.max_listed ? opt.max_listed : 16;
    uint32_t before = 0;
    for (uint32_t s = 0; s < located.n_sections; s++) {
        const ug_zkey_locate_section& e = located.section[s];
        const uint32_t points = (1u << 3) | (1u << 5) | (1u << 6) | (1u << 7) | (1u << 8) | (1u << 9);
        if (e.section >= 32 || !(points >> e.section & 1) || !(rep.failed_sections >> e.section & 1) || (before >> e.section & 1)) abort();
        before |= 1u << e.section;
        if (e.method != UG_LOCATE_BYTES && e.method != UG_LOCATE_RATIO) abort();
        if (e.blocks != (e.records + 255) / 256 || e.bad_blocks > e.blocks || e.resolved_blocks > e.bad_blocks || e.bad_records > e.records) abort();
        if (e.exact != (e.resolved_blocks == e.bad_blocks ? 1u : 0u)) abort();
        if (e.n_listed > listed || e.n_listed > e.bad_records) abort();
        for (uint32_t i = 0; i < e.n_listed; i++)
            if (e.index[i] >= e.records || (i && e.index[i] <= e.index[i - 1])) abort();
        located_sections++;
    }
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: fuzz_zkey_locate <r1cs> <ptau> <zkey> <iterations> <seed>\n"); return 2; }
    const std::vector<uint8_t> orig[3] = {readFile(argv[1]), readFile(argv[2]), readFile(argv[3])};
    const long iters = atol(argv[4]);
    rng_state = strtoull(argv[5], nullptr, 10);
    for (const auto& f : orig)
        if (f.size() < 24) { fprintf(stderr, "a file is missing or too short\n"); return 3; }
    if (locate(orig) != UG_OK) { fprintf(stderr, "the unmodified triple is not valid\n"); return 3; }
    // .r1cs: sections 1, 2; .ptau: 1, 4, 5, 6, 12 - 15; .zkey: 1 - 9
    const uint32_t readIds[3] = {0x6u, 0xf072u, 0x3feu};
    std::vector<size_t> hdrs[3];
    for (int i = 0; i < 3; i++) {
        hdrs[i] = headerOffsets(walkSections(orig[i]), readIds[i]);
        if (hdrs[i].empty()) { fprintf(stderr, "no sections found\n"); return 3; }
    }
    const std::vector<SectionAt> zsecs = walkSections(orig[2]);
    const std::vector<SectionAt> rsecs = walkSections(orig[0]);
    const SectionAt* constraints = findSection(rsecs, 2);
    const uint32_t g1Ids[5] = {3, 5, 6, 8, 9};
    const uint64_t extremes[] = {0, 1, 63, 64, 127, 128, 0xffffffffull, 0x7fffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffc0ull};
    const uint32_t extremes32[] = {0, 1, 2, 3, 7, 8, 31, 32, 64, 1337, 0x7fffffffu, 0xffffffffu};
    long count[3] = {0, 0, 0};
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> file[3] = {orig[0], orig[1], orig[2]};
        std::vector<uint8_t>& key = file[2];
        int kind = (int)(rnd() % 16);
        kind = kind == 0 ? (int)(rnd() % 9) : kind == 1 ? 9 + (int)(rnd() % 2) : kind == 2 ? 11 : 13;
        if (kind < 9) {                          // a G1 record of a point section replaced by a G1 record of any of them, or by infinity
            const SectionAt* to = findSection(zsecs, g1Ids[rnd() % 5]);
            const SectionAt* from = findSection(zsecs, g1Ids[rnd() % 5]);
            if (to && from && to->size >= 64 && from->size >= 64) {
                uint8_t* dst = key.data() + to->header + 12 + 64 * (rnd() % (to->size / 64));
                if (kind < 2) memset(dst, 0, 64);
                else memcpy(dst, orig[2].data() + from->header + 12 + 64 * (rnd() % (from->size / 64)), 64);
                if (kind == 8) {                 // ... and a second one, in another section perhaps
                    const SectionAt* two = findSection(zsecs, g1Ids[rnd() % 5]);
                    if (two && two->size >= 64) memcpy(key.data() + two->header + 12 + 64 * (rnd() % (two->size / 64)), dst, 64);
                }
            }
        } else if (kind < 11) {                  // two B2 records swapped, or one set to infinity
            const SectionAt* b2 = findSection(zsecs, 7);
            if (b2 && b2->size >= 256) {
                uint8_t* a = key.data() + b2->header + 12 + 128 * (rnd() % (b2->size / 128));
                uint8_t* b = key.data() + b2->header + 12 + 128 * (rnd() % (b2->size / 128));
                uint8_t t[128];
                memcpy(t, a, 128);
                if (kind == 9) { memcpy(a, b, 128); memcpy(b, t, 128); }
                else memset(a, 0, 128);
            }
        } else if (kind < 13) {                  // a low byte of the .r1cs' constraints: a coefficient, a wire or a count
            if (constraints && constraints->size) flipBit(file[0], constraints->header + 12, constraints->size);
        } else {                                 // fuzz_zkey_verify's mutations of any of the three files
            const int which = (int)(rnd() % 3);
            std::vector<uint8_t>& buf = file[which];
            switch (rnd() % 4) {
                case 0: replaceWord(buf, 8, extremes32); break;                // the section count
                case 1: truncate(buf); break;
                case 2: replaceSectionSize(buf, hdrs[which], extremes); break;
                default: replaceSectionId(buf, hdrs[which]); break;
            }
        }
        count[locate(file)]++;
    }
    printf("%ld valid, %ld invalid, %ld refused, %ld sections located, 0 crashed\n", count[UG_OK], count[UG_ZKEY_INVALID], count[UG_ERROR], located_sections);
    return 0;
}
