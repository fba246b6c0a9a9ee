// fuzz_kit.hpp -- what the binfile harnesses of this directory share (fuzz_parsers.cpp, fuzz_r1cs.cpp, fuzz_ptau.cpp,
// fuzz_ptau_prepare.cpp, fuzz_zkey_verify.cpp): the generator, an exact-size buffer, a file read whole, the walk over a binfile's
// section headers, and the mutations that differ only in a harness's tables. A harness keeps its parse / verify body, its tables
// and the order in which it draws: the same seed gives the same mutations as before the harnesses shared this.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

namespace fuzz {

inline uint64_t rng_state;
inline uint64_t rnd() {                       // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

inline std::vector<uint8_t> readFile(const char* path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

// a heap block of exactly the buffer's size: one byte past its end is the sanitizer's
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Exact(const std::vector<uint8_t>& v) : p(new uint8_t[v.size() ? v.size() : 1]), n(v.size()) {
        if (n) memcpy(p.get(), v.data(), n);
    }
};

// the sections of a binfile of at least 12 bytes, in its order: `header` is the offset of (id u32, size u64), the payload
// starts 12 bytes later. The walk stops where a header would leave the file.
struct SectionAt { size_t header; uint32_t id; uint64_t size; };
inline std::vector<SectionAt> walkSections(const std::vector<uint8_t>& f) {
    std::vector<SectionAt> out;
    uint32_t n;
    memcpy(&n, f.data() + 8, 4);
    size_t pos = 12;
    for (uint32_t i = 0; i < n && pos + 12 <= f.size(); i++) {
        SectionAt s;
        s.header = pos;
        memcpy(&s.id, f.data() + pos, 4);
        memcpy(&s.size, f.data() + pos + 4, 8);
        out.push_back(s);
        pos += 12 + s.size;
    }
    return out;
}
// the header offsets of every section
inline std::vector<size_t> headerOffsets(const std::vector<SectionAt>& secs) {
    std::vector<size_t> out;
    for (const SectionAt& s : secs) out.push_back(s.header);
    return out;
}
// ... of the sections whose id's bit is set in `ids`
inline std::vector<size_t> headerOffsets(const std::vector<SectionAt>& secs, uint32_t ids) {
    std::vector<size_t> out;
    for (const SectionAt& s : secs)
        if (s.id < 32 && (ids >> s.id & 1)) out.push_back(s.header);
    return out;
}
// the last section with this id (null: none)
inline const SectionAt* findSection(const std::vector<SectionAt>& secs, uint32_t id) {
    const SectionAt* at = nullptr;
    for (const SectionAt& s : secs)
        if (s.id == id) at = &s;
    return at;
}

// ---- mutations; each draws what it needs, in the order written ----
// one bit of a byte in [base, base + span)
inline void flipBit(std::vector<uint8_t>& buf, size_t base, uint64_t span) { buf[base + rnd() % span] ^= (uint8_t)(1u << (rnd() % 8)); }
// 1 .. most of them
inline void flipBits(std::vector<uint8_t>& buf, size_t base, uint64_t span, int most) {
    int k = 1 + (int)(rnd() % most);
    for (int j = 0; j < k; j++) flipBit(buf, base, span);
}
inline void truncate(std::vector<uint8_t>& buf) { buf.resize(rnd() % (buf.size() + 1)); }
// a section size replaced by an extreme value (+- a small offset)
template <size_t N> void replaceSectionSize(std::vector<uint8_t>& buf, const std::vector<size_t>& hdrs, const uint64_t (&extremes)[N]) {
    size_t h = hdrs[rnd() % hdrs.size()];
    uint64_t v = extremes[rnd() % N] + (rnd() % 3) - 1;
    memcpy(buf.data() + h + 4, &v, 8);
}
// a section id replaced: a section goes missing, another appears twice
inline void replaceSectionId(std::vector<uint8_t>& buf, const std::vector<size_t>& hdrs) {
    size_t h = hdrs[rnd() % hdrs.size()];
    uint32_t v = (uint32_t)(rnd() % 18);
    memcpy(buf.data() + h, &v, 4);
}
// the u32 at `at` replaced by an extreme value: the section count sits at 8
template <size_t N> void replaceWord(std::vector<uint8_t>& buf, size_t at, const uint32_t (&extremes32)[N]) {
    uint32_t v = extremes32[rnd() % N];
    memcpy(buf.data() + at, &v, 4);
}

// `iters` turns of a one-file harness: a fresh copy, one mutation, parse (0: parsed); then the line the tests read
template <class Mutate, class Parse> void mutateAndParse(const std::vector<uint8_t>& orig, long iters, Mutate&& mutate, Parse&& parse) {
    long ok = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> buf = orig;
        mutate(buf);
        if (parse(buf) == 0) ok++; else rejected++;
    }
    printf("%ld parsed, %ld rejected, 0 crashed\n", ok, rejected);
}

}  // namespace fuzz
