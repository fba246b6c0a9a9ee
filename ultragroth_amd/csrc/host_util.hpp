// host_util.hpp -- host-side pieces shared by the prover classes: iden3 binfile container, zkey / wtns
// headers, decimal printing, blinding randomness, Keccak-256.
//
// Mirrors, with its own code, the behaviour of the reference's
//   BinFileUtils::BinFile          src/binfile_utils.cpp:24-176 (error strings included)
//   ZKeyUtils::loadHeader          src/zkey_utils.cpp:42-76, ultra_groth_loadHeader :123-163
//   WtnsUtils::loadHeader          src/wtns_utils.cpp:13-26
//   BinFileUtils::FileLoader       src/fileloader.cpp:23-59 (mmap, MADV_SEQUENTIAL)
//   randombytes_buf                src/random_generator.hpp:4-25
//   FIPS202_KECCAK_256             src/keccak256.cpp:8 (Keccak-f[1600], rate 1088, padding 0x01)
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace ughost {

struct Section { const uint8_t* start; uint64_t size; };

class BinFile {
public:
    BinFile(const void* data, uint64_t size, const std::string& type, uint32_t maxVersion);
    const uint8_t* sectionData(uint32_t id, uint32_t pos = 0) const;
    uint64_t sectionSize(uint32_t id, uint32_t pos = 0) const;
    bool hasSection(uint32_t id) const { return sections_.count(id) != 0; }
    // every section as the file has them, in its order: (id, payload)
    const std::vector<std::pair<uint32_t, Section>>& inOrder() const { return order_; }
private:
    const Section& find(uint32_t id, uint32_t pos) const;
    std::map<uint32_t, std::vector<Section>> sections_;
    std::vector<std::pair<uint32_t, Section>> order_;
};

// A version-1 BinFile of `type` over (data, size) for an interface whose messages carry the prefix of the file they are about:
// a null buffer is refused as prefix + nullMessage, the container's own errors are rethrown as prefix + their text.
std::unique_ptr<BinFile> openBinFile(const void* data, uint64_t size, const char* type, const std::string& prefix, const char* nullMessage);

class FileMap {           // read-only mmap of a whole file
public:
    explicit FileMap(const std::string& path);
    ~FileMap();
    const void* data() const { return addr_; }
    uint64_t size() const { return size_; }
    FileMap(const FileMap&) = delete;
    FileMap& operator=(const FileMap&) = delete;
private:
    void* addr_ = nullptr; uint64_t size_ = 0; int fd_ = -1;
};

struct ZkeyHeader {
    uint32_t n8q = 0, n8r = 0, nVars = 0, nPublic = 0, domainSize = 0;
    uint64_t nCoefs = 0;
    bool rIsBn254 = false;
    const uint8_t *alpha1 = nullptr, *beta1 = nullptr, *beta2 = nullptr, *gamma2 = nullptr, *delta1 = nullptr, *delta2 = nullptr;
    // UltraGroth (protocol 1337): delta1/delta2 above hold the FINAL-round deltas
    uint32_t numIndexesC1 = 0, numIndexesC2 = 0, randIndx = 0;
    const uint8_t *roundDelta1 = nullptr, *roundDelta2 = nullptr;
};
ZkeyHeader loadZkeyHeader(const BinFile& f, bool ultra);

struct WtnsHeader { uint32_t n8 = 0, nVars = 0; bool primeIsBn254 = false; };
WtnsHeader loadWtnsHeader(const BinFile& f);

// ---- .r1cs (iden3 binfile, magic "r1cs", version 1; the layout is restated in include/ultragroth_hip.h) ----
// Every failure is a C++ exception whose message starts with "r1cs: ".
struct R1csHeader {
    uint32_t n8 = 0, nWires = 0, nPubOut = 0, nPubIn = 0, nPrvIn = 0, nConstraints = 0;
    uint64_t nLabels = 0;
};
R1csHeader loadR1csHeader(const BinFile& f);
// one of the matrices A, B, C in CSR form: row k holds the terms [rowPtr[k], rowPtr[k + 1]), term p is coefficient
// val[32 p, 32 p + 32) (plain little-endian integer below r, as the file has it) of wire sig[p]; the file's order is kept
struct R1csMatrix {
    std::vector<uint32_t> rowPtr, sig;
    std::vector<uint8_t> val;
};
struct R1cs {
    R1csHeader hdr;
    uint64_t terms[3] = {0, 0, 0};
    R1csMatrix m[3];
};
// first pass over section 2: bounds, wire ids and coefficients checked, the terms of each matrix counted
void countR1csTerms(const BinFile& f, const R1csHeader& h, uint64_t terms[3]);
// both passes: the header, the first pass, then the three CSR triples
void loadR1cs(const BinFile& f, R1cs& out);
extern const uint8_t BN254_R_BYTES[32];      // the scalar modulus r, little-endian

// ---- .ptau (iden3 binfile, magic "ptau", version 1; the layout is restated in include/ultragroth_hip.h -- from memory of
// snarkjs' format: no file of a real ceremony has been read yet) ----
// Every failure is a C++ exception whose message starts with "ptau: ". Nothing here walks a section: a 2^28 file is hundreds of GB.
struct PtauHeader {
    uint32_t n8 = 0, power = 0, ceremonyPower = 0;
    bool prepared = false;                    // sections 12 - 15 (the Lagrange forms) are all there
};
PtauHeader loadPtauHeader(const BinFile& f);
// what a phase-2 setup of domain 2^logN reads: level logN of sections 12 (tauG1), 13 (tauG2), 14 (alphaTauG1), 15 (betaTauG1),
// level logN + 1 of section 12, record 0 of sections 4 and 5, section 6. first12 / firstTop: the index of a slice's first record
// in its section. Every size is checked (compared before it is added or multiplied) before a pointer is formed.
struct PtauSlices {
    uint64_t n = 0;                           // 2^logN
    const uint8_t *tau1 = nullptr, *tau2 = nullptr, *alphaTau1 = nullptr, *betaTau1 = nullptr;      // n records each
    const uint8_t* top = nullptr;             // 2 n records of section 12: level logN + 1
    const uint8_t *alpha1 = nullptr, *beta1 = nullptr, *beta2 = nullptr;
    uint64_t first = 0, firstTop = 0;         // n - 1 and 2 n - 1
};
PtauSlices loadPtauSlices(const BinFile& f, const PtauHeader& h, uint32_t logN);
// what preparing the file for phase 2 at `power` reads (power = 0: the file's own; below the file's: the file cut to it): the
// first 2^(power+1) - 1 records of section 2 (tauG1) and the first 2^power of sections 3 (tauG2), 4 (alphaTauG1), 5 (betaTauG1).
// Counts are compared with the sections' own sizes before anything is multiplied.
struct PtauPowers {
    uint32_t power = 0;
    uint64_t n = 0;                           // 2^power
    const uint8_t *tau1 = nullptr, *tau2 = nullptr, *alphaTau1 = nullptr, *betaTau1 = nullptr;      // 2 n - 1, n, n, n records
};
PtauPowers loadPtauPowers(const BinFile& f, const PtauHeader& h, uint32_t power);
// sections 12 - 15 whole, for a comparison with recomputed ones: 4 n - 1 records of section 12 (levels 0 .. power + 1), 2 n - 1 of
// sections 13, 14, 15 (levels 0 .. power), n = 2^power of the header
struct PtauLagrange {
    const uint8_t* sec[4] = {nullptr, nullptr, nullptr, nullptr};      // 12, 13, 14, 15
};
PtauLagrange loadPtauLagrange(const BinFile& f, const PtauHeader& h);
extern const uint8_t BN254_Q_LE[32];          // the base modulus q, little-endian

// 32-byte little-endian plain integer -> decimal string
std::string toDecimal(const uint8_t le[32]);

// blinding randomness: OS entropy unless a test override is queued (ug_test_set_blinding)
void randomBytes(void* buf, size_t n);
bool setRandomOverride(const void* bytes, size_t n);      // false (and no effect) unless ULTRAGROTH_TEST_HOOKS=1
bool testHooksEnabled();

void keccak256(uint8_t out[32], const uint8_t* in, uint64_t len);

}  // namespace ughost
