// fuzz_ultra_keys.cpp -- CPU-only robustness harness for the UltraGroth phase-2 setup and key check on host threads
// (ultragroth_amd/csrc/setup_ptau.cpp and zkey_verify_host.cpp with point_check.cpp, setup_host.cpp and host_util.cpp:
// ug_ultra_setup_ptau_size / _run and ug_ultra_zkey_verify_run, device = -1), built with -fsanitize=address,undefined by
// tests/test_ultra_keys_host.py. No HIP code is linked: the four device calls the point check names
// are stubs that abort. An .r1cs and a .ptau are downloads and the signal lists come from a caller: whatever arrives, the call
// must end with a key of exactly the size the size query gave, or with a refusal -- never in an out-of-bounds access (the lists
// index the K records and size sections 8 - 11).
//
// usage: fuzz_ultra_keys <circuit.r1cs> <prepared.ptau> <n_public> <n_wires> <iterations> <seed>
// The unmodified lists are the private wires alternating between the rounds, rand_indx = 1. Each turn mutates ONE of: the .r1cs,
// the .ptau (bit flips, a truncation, a section size, id or the section count replaced by an extreme value), the lists (an entry
// replaced by an extreme or a public or a repeated signal, an entry dropped or added, a list emptied, rand_indx replaced, the
// lists swapped), or the deltas (0, r, all ones) -- each through the setup --, or the KEY the unmodified inputs give (the same file
// mutations over its sections 1 - 12, or the spec it is checked against) through the check, which must answer valid, invalid or
// refused: the key's own lists index the weights and size its sections. The buffers are exact-size heap blocks, the output included.
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

struct Spec {
    uint32_t randIndx;
    std::vector<uint32_t> round, final;
    uint8_t delta[2][32];
    uint32_t contribute;
};

// UG_OK, UG_ZKEY_INVALID or UG_ERROR
static int verify(const std::vector<uint8_t> file[2], const std::vector<uint8_t>& key, const Spec& s, bool withSpec) {
    const Exact r1cs(file[0]), ptau(file[1]), zkey(key);
    const std::vector<uint8_t> rb((const uint8_t*)s.round.data(), (const uint8_t*)s.round.data() + 4 * s.round.size());
    const std::vector<uint8_t> fb((const uint8_t*)s.final.data(), (const uint8_t*)s.final.data() + 4 * s.final.size());
    const Exact round(rb), final(fb);
    ug_ultra_zkey_verify_options opt;
    memset(&opt, 0, sizeof opt);
    opt.size = sizeof opt;
    opt.validate = 2;
    opt.check_spec = withSpec ? 1 : 0;
    opt.rand_indx = s.randIndx;
    opt.round_signals = (const uint32_t*)round.p.get(); opt.n_round = s.round.size();
    opt.final_signals = (const uint32_t*)final.p.get(); opt.n_final = s.final.size();
    ug_zkey_verify_report rep;
    double ms[UG_ZKEY_VERIFY_PHASES];
    char message[256] = {0};
    const int rc = ug_ultra_zkey_verify_run(&opt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, zkey.p.get(), zkey.n, -1, &rep, ms, message, sizeof message);
    if (rc != UG_OK && rc != UG_ZKEY_INVALID && rc != UG_ERROR) abort();
    if ((rc == UG_ZKEY_INVALID) != (rep.failed_sections != 0)) abort();
    if (rc != UG_OK && !message[0]) abort();
    return rc;
}

// UG_OK or UG_ERROR; keyOut (may be null) receives the key
static int setup(const std::vector<uint8_t> file[2], const Spec& s, std::vector<uint8_t>* keyOut = nullptr) {
    const Exact r1cs(file[0]), ptau(file[1]);
    // exact-size copies of the lists: an index one past a list's end is the sanitizer's
    const std::vector<uint8_t> rb((const uint8_t*)s.round.data(), (const uint8_t*)s.round.data() + 4 * s.round.size());
    const std::vector<uint8_t> fb((const uint8_t*)s.final.data(), (const uint8_t*)s.final.data() + 4 * s.final.size());
    const Exact round(rb), final(fb);
    ug_ultra_setup_ptau_options opt;
    memset(&opt, 0, sizeof opt);
    opt.size = sizeof opt;
    opt.validate = 2;
    opt.contribute = s.contribute;
    memcpy(opt.delta_round, s.delta[0], 32);
    memcpy(opt.delta_final, s.delta[1], 32);
    opt.rand_indx = s.randIndx;
    opt.round_signals = (const uint32_t*)round.p.get(); opt.n_round = s.round.size();
    opt.final_signals = (const uint32_t*)final.p.get(); opt.n_final = s.final.size();
    char message[256] = {0};
    uint64_t zbytes = 0, vmax = 0, wrote = 0, vlen = 0;
    int rc = ug_ultra_setup_ptau_size(&opt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, &zbytes, &vmax, message, sizeof message);
    if (rc != UG_OK && rc != UG_ERROR) abort();
    if (rc != UG_OK) { if (!message[0]) abort(); return rc; }
    if (zbytes > (1u << 26) || vmax > (1u << 26)) abort();          // (a circuit of a handful of wires)
    const std::unique_ptr<uint8_t[]> zkey(new uint8_t[zbytes]);
    const std::unique_ptr<char[]> vkey(new char[vmax]);
    double ms[UG_SETUP_PTAU_PHASES];
    rc = ug_ultra_setup_ptau_run(&opt, r1cs.p.get(), r1cs.n, ptau.p.get(), ptau.n, -1, zkey.get(), zbytes, &wrote, vkey.get(), vmax, &vlen, ms,
                                 message, sizeof message);
    if (rc != UG_OK && rc != UG_ERROR) abort();
    if (rc == UG_OK && (wrote != zbytes || vlen >= vmax)) abort();
    if (rc != UG_OK && !message[0]) abort();
    if (rc == UG_OK && keyOut) keyOut->assign(zkey.get(), zkey.get() + wrote);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: fuzz_ultra_keys <r1cs> <ptau> <n_public> <n_wires> <iterations> <seed>\n"); return 2; }
    const std::vector<uint8_t> orig[2] = {readFile(argv[1]), readFile(argv[2])};
    const uint32_t nPublic = (uint32_t)atol(argv[3]), nWires = (uint32_t)atol(argv[4]);
    const long iters = atol(argv[5]);
    rng_state = strtoull(argv[6], nullptr, 10);
    for (const auto& f : orig)
        if (f.size() < 24) { fprintf(stderr, "a file is missing or too short\n"); return 3; }
    Spec base;
    memset(base.delta, 0, sizeof base.delta);
    base.delta[0][0] = 3; base.delta[1][0] = 5;
    base.contribute = 1;
    base.randIndx = 1;
    for (uint32_t s = nPublic + 1; s < nWires; s++) ((s & 1) ? base.round : base.final).push_back(s);
    std::vector<uint8_t> key;
    if (setup(orig, base, &key) != UG_OK) { fprintf(stderr, "the unmodified inputs are refused\n"); return 3; }
    if (verify(orig, key, base, true) != UG_OK) { fprintf(stderr, "the unmodified key is not valid\n"); return 3; }
    const std::vector<size_t> keyHdrs = headerOffsets(walkSections(key), 0x1ffeu);
    // .r1cs: sections 1, 2; .ptau: 1, 4, 5, 6, 12 - 15
    const uint32_t readIds[2] = {0x6u, 0xf072u};
    std::vector<size_t> hdrs[2];
    for (int i = 0; i < 2; i++) {
        hdrs[i] = headerOffsets(walkSections(orig[i]), readIds[i]);
        if (hdrs[i].empty()) { fprintf(stderr, "no sections found\n"); return 3; }
    }
    const uint64_t extremes[] = {0, 1, 43, 44, 63, 64, 127, 128, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                                 0xffffffffffffffffull, 0xfffffffffffffff4ull, 0xffffffffffffffc0ull};
    const uint32_t extremes32[] = {0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 64, 1337, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    const uint32_t signals[] = {0, 1, nPublic, nPublic + 1, nWires - 1, nWires, nWires + 1, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    const size_t nSignals = sizeof signals / sizeof signals[0];
    static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                     0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
    long count[2] = {0, 0}, verdicts[3] = {0, 0, 0};
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> file[2] = {orig[0], orig[1]};
        Spec s = base;
        const int which = (int)(rnd() % 5);
        if (which == 4) {                          // the key, or the spec it is checked against, through the check
            std::vector<uint8_t> buf = key;
            bool withSpec = (rnd() & 1) != 0;
            switch (rnd() % 8) {
                case 0: flipBits(buf, 12, buf.size() - 12, 3); break;
                case 1: case 2: {                  // a bit flip at the start of a section: the header's counts, a list's first entries
                    size_t h = keyHdrs[rnd() % keyHdrs.size()];
                    uint64_t sz;
                    memcpy(&sz, buf.data() + h + 4, 8);
                    if (sz) flipBit(buf, h + 12, sz < 112 ? sz : 112);
                    break;
                }
                case 3: truncate(buf); break;
                case 4: replaceSectionSize(buf, keyHdrs, extremes); break;
                case 5: replaceSectionId(buf, keyHdrs); break;
                case 6: {                          // an entry of section 10 or 11 replaced by a signal of the table
                    const std::vector<SectionAt> walked = walkSections(buf);
                    const SectionAt* sec = findSection(walked, (rnd() & 1) ? 10 : 11);
                    if (sec && sec->size >= 4) {
                        const uint32_t v = signals[rnd() % nSignals];
                        memcpy(buf.data() + sec->header + 12 + 4 * (rnd() % (sec->size / 4)), &v, 4);
                    }
                    break;
                }
                default: withSpec = true; if (!s.round.empty()) s.round[rnd() % s.round.size()] = signals[rnd() % nSignals]; break;
            }
            verdicts[verify(file, buf, s, withSpec)]++;
            continue;
        }
        if (which < 2) {
            std::vector<uint8_t>& buf = file[which];
            const std::vector<size_t>& hd = hdrs[which];
            switch (rnd() % 6) {
                case 0: flipBits(buf, 12, buf.size() - 12, 3); break;
                case 1: {                              // a bit flip at the start of a section: the headers' fields, the counts
                    size_t h = hd[rnd() % hd.size()];
                    uint64_t sz;
                    memcpy(&sz, buf.data() + h + 4, 8);
                    if (sz) flipBit(buf, h + 12, sz < 96 ? sz : 96);
                    break;
                }
                case 2: truncate(buf); break;
                case 3: replaceSectionSize(buf, hd, extremes); break;
                case 4: replaceSectionId(buf, hd); break;
                default: replaceWord(buf, 8, extremes32); break;
            }
        } else if (which == 2) {
            std::vector<uint32_t>& lst = (rnd() & 1) ? s.round : s.final;
            switch (rnd() % 7) {
                case 0: if (!lst.empty()) lst[rnd() % lst.size()] = signals[rnd() % nSignals]; break;
                case 1: if (!lst.empty()) lst[rnd() % lst.size()] = lst[rnd() % lst.size()]; break;
                case 2: if (!lst.empty()) lst.erase(lst.begin() + (long)(rnd() % lst.size())); break;
                case 3: lst.push_back(signals[rnd() % nSignals]); break;
                case 4: lst.clear(); break;
                case 5: s.randIndx = signals[rnd() % nSignals]; break;
                default: s.round.swap(s.final); break;                     // (still a partition: a key)
            }
        } else {
            uint8_t* d = s.delta[rnd() & 1];
            switch (rnd() % 4) {
                case 0: memset(d, 0, 32); break;
                case 1: memcpy(d, R_LE, 32); break;
                case 2: memset(d, 0xff, 32); break;
                default: s.contribute = (uint32_t)(rnd() % 5); break;      // (0, 2: the deltas are not read; 3, 4: refused)
            }
        }
        count[setup(file, s) == UG_OK ? 0 : 1]++;
    }
    printf("%ld keys, %ld refused, %ld valid, %ld invalid, %ld refused by the check, 0 crashed\n", count[0], count[1], verdicts[UG_OK],
           verdicts[UG_ZKEY_INVALID], verdicts[UG_ERROR]);
    return 0;
}
