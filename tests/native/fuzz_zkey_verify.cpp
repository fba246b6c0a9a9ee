// fuzz_zkey_verify.cpp -- CPU-only robustness harness for the key check on host threads (ultragroth_amd/csrc/zkey_verify.cpp with
// setup_ptau.cpp, setup_host.cpp and host_util.cpp: ug_zkey_verify_run, device = -1), built with -fsanitize=address,undefined by
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
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>
#include "../../include/ultragroth_hip.h"

extern "C" {
// (setup_ptau.cpp's point check reaches these for device >= 0 only)
int ug_ctx_create(ug_ctx**, int) { abort(); }
void ug_ctx_destroy(ug_ctx*) { abort(); }
int ug_points_check(ug_ctx*, int, const void*, uint64_t, int, ug_point_fault*) { abort(); }
const char* ug_last_error(void) { abort(); }
}

static uint64_t rng_state;
static uint64_t rnd() {                       // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static std::vector<uint8_t> readFile(const char* path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

struct Exact {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Exact(const std::vector<uint8_t>& v) : p(new uint8_t[v.size() ? v.size() : 1]), n(v.size()) {
        if (n) memcpy(p.get(), v.data(), n);
    }
};

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

// offsets of the section headers (id u32, size u64 at +4) of a binfile's sections whose bit is set in `ids`: the ones the check reads
static std::vector<size_t> sectionHeaders(const std::vector<uint8_t>& f, uint32_t ids) {
    std::vector<size_t> out;
    uint32_t n;
    memcpy(&n, f.data() + 8, 4);
    size_t pos = 12;
    for (uint32_t i = 0; i < n && pos + 12 <= f.size(); i++) {
        uint32_t id;
        memcpy(&id, f.data() + pos, 4);
        if (id < 32 && (ids >> id & 1)) out.push_back(pos);
        uint64_t sz;
        memcpy(&sz, f.data() + pos + 4, 8);
        pos += 12 + sz;
    }
    return out;
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
        hdrs[i] = sectionHeaders(orig[i], readIds[i]);
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
            case 0: {                                  // bit flips anywhere: mostly inside a point or a coefficient
                int k = 1 + (int)(rnd() % 3);
                for (int j = 0; j < k; j++) buf[12 + rnd() % (buf.size() - 12)] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 1: {                                  // bit flips at the start of a section: the headers' fields, the counts
                size_t h = hd[rnd() % hd.size()];
                uint64_t sz;
                memcpy(&sz, buf.data() + h + 4, 8);
                if (sz) buf[h + 12 + rnd() % (sz < 96 ? sz : 96)] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 2: buf.resize(rnd() % (buf.size() + 1)); break;           // truncation
            case 3: {                                  // a section size replaced by an extreme value (+- a small offset)
                size_t h = hd[rnd() % hd.size()];
                uint64_t v = extremes[rnd() % (sizeof extremes / sizeof extremes[0])] + (rnd() % 3) - 1;
                memcpy(buf.data() + h + 4, &v, 8);
                break;
            }
            case 4: {                                  // a u32 among the first words of a section replaced (n8, nVars, nPublic, domain, power, counts)
                size_t h = hd[rnd() % hd.size()];
                uint64_t sz;
                memcpy(&sz, buf.data() + h + 4, 8);
                uint32_t v = extremes32[rnd() % (sizeof extremes32 / sizeof extremes32[0])];
                if (sz >= 4) memcpy(buf.data() + h + 12 + 4 * (rnd() % (sz / 4 < 24 ? sz / 4 : 24)), &v, 4);
                break;
            }
            case 5: {                                  // a section id replaced: a section goes missing, another appears twice
                size_t h = hd[rnd() % hd.size()];
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
        count[verify(file)]++;
    }
    printf("%ld valid, %ld invalid, %ld refused, 0 crashed\n", count[UG_OK], count[UG_ZKEY_INVALID], count[UG_ERROR]);
    return 0;
}
