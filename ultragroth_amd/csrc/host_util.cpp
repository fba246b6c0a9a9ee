// host_util.cpp -- see host_util.hpp.
#include "host_util.hpp"
#include <cstdlib>
#include <fcntl.h>
#include <mutex>
#include <sys/mman.h>
#include <sys/random.h>
#include <sys/stat.h>
#include <system_error>
#include <unistd.h>

namespace ughost {

namespace {
uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

const uint8_t BN254_R_LE[32] = {
    0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
    0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
}  // namespace

// ---- BinFile: magic[4] | u32 version | u32 nSections | { u32 type, u64 size, bytes }* ----------------
BinFile::BinFile(const void* data, uint64_t size, const std::string& type, uint32_t maxVersion) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    if (size < 12) throw std::range_error("File is too short.");
    std::string got(reinterpret_cast<const char*>(p), 4);
    if (got != type) throw std::invalid_argument("Invalid file type. It should be " + type + " and it is " + got);
    uint32_t version = rd32(p + 4);
    if (version > maxVersion)
        throw std::invalid_argument("Invalid version. It should be <=" + std::to_string(maxVersion) + " and it is " + std::to_string(version));
    uint32_t nSections = rd32(p + 8);
    if (size < 12 + (uint64_t)nSections * 12)
        throw std::range_error("File is too short to contain " + std::to_string(nSections) + " sections.");
    uint64_t pos = 12;
    for (uint32_t i = 0; i < nSections; i++) {
        if (pos + 12 > size)
            throw std::range_error("File pos is too big. There are " + std::to_string(size) + " bytes and it's trying to access byte " + std::to_string(pos + 12));
        uint32_t sType = rd32(p + pos);
        uint64_t sSize = rd64(p + pos + 4);
        pos += 12;
        // checked before the add: a crafted size near 2^64 must not wrap `pos` back into the buffer (the reference adds
        // first, binfile_utils.cpp:60-66, and would accept it)
        if (sSize > size - pos)
            throw std::range_error("Section #" + std::to_string(i) + " is invalid.. It ends at pos " +
                                   (sSize > UINT64_MAX - pos ? "beyond 2^64" : std::to_string(pos + sSize)) +
                                   " but should end before " + std::to_string(size) + ".");
        sections_[sType].push_back(Section{p + pos, sSize});
        order_.emplace_back(sType, Section{p + pos, sSize});
        pos += sSize;
    }
}
const Section& BinFile::find(uint32_t id, uint32_t pos) const {
    auto it = sections_.find(id);
    if (it == sections_.end()) throw std::range_error("Section does not exist: " + std::to_string(id));
    if (pos >= it->second.size())
        throw std::range_error("Section pos too big. There are " + std::to_string(it->second.size()) +
                               " and it's trying to access section: " + std::to_string(pos));
    return it->second[pos];
}
const uint8_t* BinFile::sectionData(uint32_t id, uint32_t pos) const { return find(id, pos).start; }
uint64_t BinFile::sectionSize(uint32_t id, uint32_t pos) const { return find(id, pos).size; }

std::unique_ptr<BinFile> openBinFile(const void* data, uint64_t size, const char* type, const std::string& prefix, const char* nullMessage) {
    if (!data) throw std::invalid_argument(prefix + nullMessage);
    try {
        return std::unique_ptr<BinFile>(new BinFile(data, size, type, 1));
    } catch (const std::exception& e) {
        throw std::invalid_argument(prefix + e.what());
    }
}

// ---- FileMap ---------------------------------------------------------------------------------------------
FileMap::FileMap(const std::string& path) {
    fd_ = open(path.c_str(), O_RDONLY);
    if (fd_ == -1) throw std::system_error(errno, std::generic_category(), "open");
    struct stat sb;
    if (fstat(fd_, &sb) == -1) { int e = errno; close(fd_); fd_ = -1; throw std::system_error(e, std::generic_category(), "fstat"); }
    size_ = (uint64_t)sb.st_size;
    addr_ = mmap(nullptr, size_ ? size_ : 1, PROT_READ, MAP_PRIVATE, fd_, 0);
    if (addr_ == MAP_FAILED) { int e = errno; close(fd_); fd_ = -1; addr_ = nullptr; throw std::system_error(e, std::generic_category(), "mmap failed"); }
    madvise(addr_, size_, MADV_SEQUENTIAL);
}
FileMap::~FileMap() {
    if (addr_) munmap(addr_, size_ ? size_ : 1);
    if (fd_ != -1) close(fd_);
}

// ---- headers ---------------------------------------------------------------------------------------------
namespace {
struct Reader {           // bounds-checked cursor over one section
    const uint8_t* p; uint64_t left;
    const uint8_t* take(uint64_t n) {
        if (n > left) throw std::range_error("Invalid section size");
        const uint8_t* r = p; p += n; left -= n; return r;
    }
    uint32_t u32() { return rd32(take(4)); }
};
}  // namespace

ZkeyHeader loadZkeyHeader(const BinFile& f, bool ultra) {
    ZkeyHeader h;
    Reader s1{f.sectionData(1), f.sectionSize(1)};
    uint32_t protocol = s1.u32();
    if (!ultra && protocol != 1) throw std::invalid_argument("zkey file is not groth16");
    if (ultra && protocol != 1337) throw std::invalid_argument("zkey file is not ultragroth");
    Reader s{f.sectionData(2), f.sectionSize(2)};
    h.n8q = s.u32();
    s.take(h.n8q);
    h.n8r = s.u32();
    const uint8_t* rPrime = s.take(h.n8r);
    h.rIsBn254 = (h.n8r == 32 && h.n8q == 32 && memcmp(rPrime, BN254_R_LE, 32) == 0);
    h.nVars = s.u32();
    h.nPublic = s.u32();
    h.domainSize = s.u32();
    if (ultra) { h.numIndexesC1 = s.u32(); h.numIndexesC2 = s.u32(); h.randIndx = s.u32(); }
    if (!h.rIsBn254) return h;                     // caller reports "zkey curve not supported"
    h.alpha1 = s.take(64);
    h.beta1 = s.take(64);
    h.beta2 = s.take(128);
    h.gamma2 = s.take(128);
    if (ultra) { h.roundDelta1 = s.take(64); h.roundDelta2 = s.take(128); }
    h.delta1 = s.take(64);
    h.delta2 = s.take(128);
    h.nCoefs = f.sectionSize(4) / (12 + h.n8r);
    return h;
}

WtnsHeader loadWtnsHeader(const BinFile& f) {
    WtnsHeader h;
    Reader s{f.sectionData(1), f.sectionSize(1)};
    h.n8 = s.u32();
    const uint8_t* prime = s.take(h.n8);
    h.primeIsBn254 = (h.n8 == 32 && memcmp(prime, BN254_R_LE, 32) == 0);
    h.nVars = s.u32();
    return h;
}

// ---- .r1cs --------------------------------------------------------------------------------------------------
const uint8_t BN254_R_BYTES[32] = {
    0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
    0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

namespace {
struct R1csError : public std::invalid_argument {
    explicit R1csError(const std::string& m) : std::invalid_argument("r1cs: " + m) {}
};
bool belowModulus(const uint8_t* le) {
    for (int i = 31; i >= 0; i--) {
        if (le[i] < BN254_R_LE[i]) return true;
        if (le[i] > BN254_R_LE[i]) return false;
    }
    return false;
}
// One walk of section 2. fill == nullptr: the validating pass (terms[] counted). Otherwise the triples are written; the first
// pass has then vouched for every bound, which are checked again all the same (the cursor never leaves the section).
void walkR1cs(const uint8_t* p, uint64_t left, const R1csHeader& h, uint64_t terms[3], R1csMatrix* fill) {
    uint64_t at[3] = {0, 0, 0};
    for (uint32_t k = 0; k < h.nConstraints; k++) {
        for (int m = 0; m < 3; m++) {
            if (left < 4) throw R1csError("constraint " + std::to_string(k) + ": record runs past the section");
            const uint32_t n = rd32(p);
            p += 4; left -= 4;
            if (n > left / 36) throw R1csError("constraint " + std::to_string(k) + ": record runs past the section");
            if (at[m] + n > 0xffffffffull) throw R1csError(std::string("more than 2^32 - 1 terms in matrix ") + "ABC"[m]);
            if (fill) fill[m].rowPtr[k] = (uint32_t)at[m];
            for (uint32_t t = 0; t < n; t++, p += 36) {
                const uint32_t wire = rd32(p);
                if (wire >= h.nWires) throw R1csError("constraint " + std::to_string(k) + ": wire " + std::to_string(wire) + " out of range");
                if (!belowModulus(p + 4)) throw R1csError("constraint " + std::to_string(k) + ": coefficient not below the field modulus");
                if (fill) {
                    fill[m].sig[at[m] + t] = wire;
                    memcpy(&fill[m].val[(at[m] + t) * 32], p + 4, 32);
                }
            }
            left -= (uint64_t)n * 36;
            at[m] += n;
        }
    }
    if (left) throw R1csError("trailing bytes in section 2");
    for (int m = 0; m < 3; m++) {
        terms[m] = at[m];
        if (fill) fill[m].rowPtr[h.nConstraints] = (uint32_t)at[m];
    }
}
}  // namespace

R1csHeader loadR1csHeader(const BinFile& f) {
    if (!f.hasSection(1)) throw R1csError("section 1 (header) is missing");
    const uint8_t* p = f.sectionData(1);
    const uint64_t size = f.sectionSize(1);
    R1csHeader h;
    if (size < 4) throw R1csError("section 1 (header) is too short");
    h.n8 = rd32(p);
    if (h.n8 != 32) throw R1csError("n8 is " + std::to_string(h.n8) + ", not 32");
    if (size < 4 + 32 + 16 + 8 + 4) throw R1csError("section 1 (header) is too short");
    if (memcmp(p + 4, BN254_R_LE, 32) != 0) throw R1csError("not over the BN254 scalar field");
    h.nWires = rd32(p + 36); h.nPubOut = rd32(p + 40); h.nPubIn = rd32(p + 44); h.nPrvIn = rd32(p + 48);
    h.nLabels = rd64(p + 52);
    h.nConstraints = rd32(p + 60);
    if (h.nWires == 0) throw R1csError("nWires is 0");
    return h;
}
void countR1csTerms(const BinFile& f, const R1csHeader& h, uint64_t terms[3]) {
    if (!f.hasSection(2)) throw R1csError("section 2 (constraints) is missing");
    walkR1cs(f.sectionData(2), f.sectionSize(2), h, terms, nullptr);
}
void loadR1cs(const BinFile& f, R1cs& out) {
    out.hdr = loadR1csHeader(f);
    countR1csTerms(f, out.hdr, out.terms);
    for (int m = 0; m < 3; m++) {
        out.m[m].rowPtr.assign((size_t)out.hdr.nConstraints + 1, 0);
        out.m[m].sig.assign((size_t)out.terms[m], 0);
        out.m[m].val.assign((size_t)out.terms[m] * 32, 0);
    }
    uint64_t again[3];
    walkR1cs(f.sectionData(2), f.sectionSize(2), out.hdr, again, out.m);
}

// ---- .ptau --------------------------------------------------------------------------------------------------
const uint8_t BN254_Q_LE[32] = {
    0x47, 0xfd, 0x7c, 0xd8, 0x16, 0x8c, 0x20, 0x3c, 0x8d, 0xca, 0x71, 0x68, 0x91, 0x6a, 0x81, 0x97,
    0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

namespace {
struct PtauError : public std::invalid_argument {
    explicit PtauError(const std::string& m) : std::invalid_argument("ptau: " + m) {}
};
constexpr uint32_t PTAU_MAX_POWER = 28;        // the two-adicity of r: no ceremony over BN254 is larger
// the first `records` records of `rec` bytes of section id; the count is compared with the section's own, never multiplied up
const uint8_t* ptauRecords(const BinFile& f, uint32_t id, uint64_t records, uint64_t rec) {
    if (!f.hasSection(id)) throw PtauError("section " + std::to_string(id) + " is missing");
    if (f.sectionSize(id) / rec < records)
        throw PtauError("section " + std::to_string(id) + " is too short: " + std::to_string(records) + " records of " + std::to_string(rec) +
                        " bytes are needed, it has " + std::to_string(f.sectionSize(id)) + " bytes");
    return f.sectionData(id);
}
}  // namespace

PtauHeader loadPtauHeader(const BinFile& f) {
    if (!f.hasSection(1)) throw PtauError("section 1 (header) is missing");
    const uint8_t* p = f.sectionData(1);
    const uint64_t size = f.sectionSize(1);
    PtauHeader h;
    if (size < 4) throw PtauError("section 1 (header) is too short");
    h.n8 = rd32(p);
    if (h.n8 != 32) throw PtauError("n8 is " + std::to_string(h.n8) + ", not 32");
    if (size < 4 + 32 + 8) throw PtauError("section 1 (header) is too short");
    if (memcmp(p + 4, BN254_Q_LE, 32) != 0) throw PtauError("not over the BN254 base field");
    h.power = rd32(p + 36);
    h.ceremonyPower = rd32(p + 40);
    if (h.power > PTAU_MAX_POWER) throw PtauError("sizes that cannot be represented: power " + std::to_string(h.power) + " is above " + std::to_string(PTAU_MAX_POWER));
    h.prepared = f.hasSection(12) && f.hasSection(13) && f.hasSection(14) && f.hasSection(15);
    return h;
}

PtauSlices loadPtauSlices(const BinFile& f, const PtauHeader& h, uint32_t logN) {
    if (!h.prepared) throw PtauError("not prepared for phase 2 (sections 12 - 15, the Lagrange forms, are absent)");
    if (h.power < logN) throw PtauError("power " + std::to_string(h.power) + " is below the circuit's " + std::to_string(logN));
    // (logN <= power <= 28: no count below passes 2^30, no byte offset 2^37)
    PtauSlices s;
    s.n = 1ull << logN;
    s.first = s.n - 1;
    s.firstTop = 2 * s.n - 1;
    const uint8_t* s12 = ptauRecords(f, 12, 4 * s.n - 1, 64);         // levels 0 .. logN + 1
    s.tau1 = s12 + s.first * 64;
    s.top = s12 + s.firstTop * 64;
    s.tau2 = ptauRecords(f, 13, 2 * s.n - 1, 128) + s.first * 128;     // levels 0 .. logN
    s.alphaTau1 = ptauRecords(f, 14, 2 * s.n - 1, 64) + s.first * 64;
    s.betaTau1 = ptauRecords(f, 15, 2 * s.n - 1, 64) + s.first * 64;
    s.alpha1 = ptauRecords(f, 4, 1, 64);
    s.beta1 = ptauRecords(f, 5, 1, 64);
    s.beta2 = ptauRecords(f, 6, 1, 128);
    return s;
}

PtauPowers loadPtauPowers(const BinFile& f, const PtauHeader& h, uint32_t power) {
    if (power > h.power) throw PtauError("power " + std::to_string(power) + " is above the file's " + std::to_string(h.power));
    // (power <= 28: no count below passes 2^29, no byte offset 2^36)
    PtauPowers s;
    s.power = power ? power : h.power;
    s.n = 1ull << s.power;
    s.tau1 = ptauRecords(f, 2, 2 * s.n - 1, 64);
    s.tau2 = ptauRecords(f, 3, s.n, 128);
    s.alphaTau1 = ptauRecords(f, 4, s.n, 64);
    s.betaTau1 = ptauRecords(f, 5, s.n, 64);
    return s;
}

PtauLagrange loadPtauLagrange(const BinFile& f, const PtauHeader& h) {
    if (!h.prepared) throw PtauError("not prepared for phase 2 (sections 12 - 15, the Lagrange forms, are absent)");
    const uint64_t n = 1ull << h.power;
    PtauLagrange s;
    s.sec[0] = ptauRecords(f, 12, 4 * n - 1, 64);
    s.sec[1] = ptauRecords(f, 13, 2 * n - 1, 128);
    s.sec[2] = ptauRecords(f, 14, 2 * n - 1, 64);
    s.sec[3] = ptauRecords(f, 15, 2 * n - 1, 64);
    return s;
}

// ---- decimal ---------------------------------------------------------------------------------------------
std::string toDecimal(const uint8_t le[32]) {
    uint32_t w[8];
    memcpy(w, le, 32);
    std::string out;
    bool nonzero = false;
    for (int i = 0; i < 8; i++) nonzero |= (w[i] != 0);
    if (!nonzero) return "0";
    while (true) {
        nonzero = false;
        uint64_t rem = 0;
        for (int i = 7; i >= 0; i--) {               // divide by 10^9
            uint64_t cur = (rem << 32) | w[i];
            w[i] = (uint32_t)(cur / 1000000000u);
            rem = cur % 1000000000u;
            nonzero |= (w[i] != 0);
        }
        char buf[16];
        if (nonzero) { snprintf(buf, sizeof buf, "%09u", (unsigned)rem); out.insert(0, buf); }
        else { snprintf(buf, sizeof buf, "%u", (unsigned)rem); out.insert(0, buf); break; }
    }
    return out;
}

// ---- randomness ------------------------------------------------------------------------------------------
namespace {
std::mutex g_rand_mutex;
std::vector<uint8_t> g_override;
size_t g_override_pos = 0;
}  // namespace

// The override makes r, s and the round randomness deterministic for every prover of the process, i.e. it removes zero
// knowledge: it only exists in processes started with ULTRAGROTH_TEST_HOOKS=1 (tests, bench.py --check, smoke()).
bool testHooksEnabled() {
    static const bool on = [] { const char* e = getenv("ULTRAGROTH_TEST_HOOKS"); return e && e[0] == '1' && !e[1]; }();
    return on;
}
bool setRandomOverride(const void* bytes, size_t n) {
    if (n && !testHooksEnabled()) return false;               // clearing is always allowed
    std::lock_guard<std::mutex> lock(g_rand_mutex);
    g_override.assign(static_cast<const uint8_t*>(bytes), static_cast<const uint8_t*>(bytes) + n);
    g_override_pos = 0;
    return true;
}
// For the CLIs, which have no call to make: under ULTRAGROTH_TEST_HOOKS=1 the environment variable ULTRAGROTH_TEST_BLINDING
// (hex) sets the override once, before the first draw (tests compare the files `prover` writes byte for byte).
static void overrideFromEnvOnce() {
    static const bool done = [] {
        const char* hex = testHooksEnabled() ? getenv("ULTRAGROTH_TEST_BLINDING") : nullptr;
        if (!hex) return true;
        std::vector<uint8_t> bytes;
        auto nib = [](char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
        for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) {
            const int hi = nib(hex[i]), lo = nib(hex[i + 1]);
            if (hi < 0 || lo < 0) break;
            bytes.push_back((uint8_t)(hi * 16 + lo));
        }
        if (!bytes.empty()) setRandomOverride(bytes.data(), bytes.size());
        return true;
    }();
    (void)done;
}
void randomBytes(void* buf, size_t n) {
    overrideFromEnvOnce();
    {
        std::lock_guard<std::mutex> lock(g_rand_mutex);
        if (!g_override.empty()) {
            uint8_t* o = static_cast<uint8_t*>(buf);
            for (size_t i = 0; i < n; i++) { o[i] = g_override[g_override_pos]; g_override_pos = (g_override_pos + 1) % g_override.size(); }
            return;
        }
    }
    uint8_t* o = static_cast<uint8_t*>(buf);
    size_t done = 0;
    while (done < n) {
        ssize_t r = getrandom(o + done, n - done, 0);
        if (r < 0) { if (errno == EINTR) continue; throw std::system_error(errno, std::generic_category(), "getrandom"); }
        done += (size_t)r;
    }
}

// ---- Keccak-256 ------------------------------------------------------------------------------------------
namespace {
const uint64_t RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
    0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
    0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
inline uint64_t rotl(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }
void permute(uint64_t a[25]) {
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], d[5];
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
        for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
        // rho + pi
        uint64_t b[25];
        int x = 1, y = 0;
        b[0] = a[0];
        uint64_t cur = a[1];
        for (int t = 0; t < 24; t++) {
            int r = ((t + 1) * (t + 2) / 2) % 64;
            int nx = y, ny = (2 * x + 3 * y) % 5;
            uint64_t next = a[nx + 5 * ny];
            b[nx + 5 * ny] = r ? rotl(cur, r) : cur;
            cur = next; x = nx; y = ny;
        }
        // chi
        for (int yy = 0; yy < 25; yy += 5)
            for (int xx = 0; xx < 5; xx++) a[yy + xx] = b[yy + xx] ^ (~b[yy + (xx + 1) % 5] & b[yy + (xx + 2) % 5]);
        a[0] ^= RC[round];
    }
}
}  // namespace

void keccak256(uint8_t out[32], const uint8_t* in, uint64_t len) {
    uint64_t st[25];
    memset(st, 0, sizeof st);
    uint8_t* sb = reinterpret_cast<uint8_t*>(st);
    const uint64_t rate = 136;
    while (len >= rate) {
        for (uint64_t i = 0; i < rate; i++) sb[i] ^= in[i];
        permute(st);
        in += rate; len -= rate;
    }
    for (uint64_t i = 0; i < len; i++) sb[i] ^= in[i];
    sb[len] ^= 0x01;
    sb[rate - 1] ^= 0x80;
    permute(st);
    memcpy(out, sb, 32);
}

}  // namespace ughost
