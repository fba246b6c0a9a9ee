// setup_host.hpp -- the development setup (.r1cs + a KNOWN trapdoor -> a TEST proving key): the host layer.
//
// Everything but the three heavy steps is host code and lives in setup_host.cpp: the checks, the derived field constants, the
// column-major index of A, B, C, section 4, the headers, the verification key. The heavy steps -- Lagrange evaluation, the
// transposed sparse products and the fixed-base multiplications of the generators -- sit behind Backend: HostBackend runs them
// on host threads through the UG_HD field and curve code (device = -1, and the only backend a program that links no HIP code
// has), the device backend of setup.hip runs them as kernels. Both compute the same residues, and every record is canonical,
// so the two give the same bytes.
// Every failure is a C++ exception whose message starts with "setup: " (or with "r1cs: ", from the loader).
//
// The phase-2 setup from a prepared powers-of-tau file (setup_ptau.cpp: ug_setup_ptau_*) shares all of this. It has no scalars
// to multiply the generator by: its two heavy steps combine POINTS per wire and multiply many points by one scalar, and sit
// behind the same Backend (combine, scale). The parts of run() it needs are declared at the end of this header.
// Preparing a .ptau for phase 2 (ptau_prepare_host.cpp: ug_ptau_prepare_*) has one heavy step, an inverse transform over points: Backend::intt.
// The key check (zkey_verify_host.cpp) shares the circuit, section 4 and the point check. What all four have in common besides --
// the guard of the extern "C" entries, the phase clock, the small byte helpers -- is declared at the end of this header.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "ec.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"

namespace ug { namespace pr { struct FinalExpConsts; } }      // (pairing.hpp)

namespace ughost {
namespace setup {

using ug::Fr;
using ug::u32;
using ug::u64;

struct SetupError : public std::invalid_argument {
    explicit SetupError(const std::string& m) : std::invalid_argument("setup: " + m) {}
};

constexpr int MAX_LOG_DOMAIN = 27;             // the prover's largest domain
constexpr u32 SPLIT_THRESHOLD = 256;           // a column with more terms is cut into pieces
constexpr u32 SPLIT_PIECE = 4096;              // terms per piece: one workgroup of 256 lanes, 16 terms each
constexpr int WINDOW_MIN = 4, WINDOW_MAX = 16; // window widths of the fixed-base tables
constexpr int WINDOW_G1 = 16, WINDOW_G2 = 16;  // the defaults of the device path (profiles/dev_setup.txt)

// signed-digit windows of width c over a scalar below r < 2^254: ceil(255 / c) of them, so that the top window's raw digit plus
// the carry into it never exceeds 2^(c-1) and no carry leaves it
inline int windowCount(int c) { return (255 + c - 1) / c; }

// one of A, B, C by columns: the terms of wire s are [colPtr[s], colPtr[s + 1]), term p is coefficient val[32 p ..) (plain
// little-endian, below r) on row row[p]. A includes snarkjs' public rows. Rows ascend inside a column (a counting sort).
struct ColMatrix {
    std::vector<u32> colPtr, row;
    std::vector<uint8_t> val;
    u64 terms() const { return row.size(); }
};
// a piece of a column longer than SPLIT_THRESHOLD: terms [first, end) of matrix m; the pieces of one column follow each other
struct Piece { u32 m, wire, first, end; };

// what the checks and the host arithmetic leave for the heavy steps; field values are canonical, device Montgomery form
struct Plan {
    bool ultra = false;
    int logN = 0;
    u32 N = 0, nVars = 0, nPublic = 0, nConstraints = 0, randIndx = 0;
    std::vector<u32> roundSignals, finalSignals;
    std::vector<uint8_t> cls;                   // per wire, the divisor of K_s: 0 gamma, 1 the round delta, 2 the final delta
    ug_setup_options opt;                       // (the pointers inside are not used after plan())
    Fr x[2], lagScale[2];                       // tau and tau / g; (x^N - 1) / N of each
    Fr omega, alpha, beta, inv[3], hScale;      // inv: 1 / gamma, 1 / delta_round, 1 / delta_final; hScale: (tau^N - 1) / (-2 delta_final)
};

// the point arrays a combination indexes: `n` segments of `count` zkey-format records each, point (seg, k) has index seg * count + k
struct PointSegs {
    const uint8_t* base[3] = {nullptr, nullptr, nullptr};
    u64 count = 0;
    int n = 0;
    u64 total() const { return count * (u64)n; }
};

// one segment of the delta step of an UltraGroth key (Backend::scaleSegments): out[i] = scalar * src[index ? index[i] : i], i < count;
// src: nSrc zkey-format G1 records, every index below nSrc (the caller has checked); scalar plain, below r
struct ScaleSeg {
    const uint8_t* scalar = nullptr;
    const uint8_t* src = nullptr;
    u64 nSrc = 0;
    const u32* index = nullptr;
    u64 count = 0;
    uint8_t* out = nullptr;
};
constexpr int MAX_SCALE_SEGS = 3;              // C1, C2 and H

// The ratio test (Backend::ratio): which of n pairs (X_i, Y_i) of G1 records have e(X_i, Q) != e(Y_i, G2)?
// Two levels. Block level: blocks of RATIO_BLOCK consecutive records, one fresh 128-bit weight per record, block j holds when
// e(sum w_i X_i, Q) = e(sum w_i Y_i, G2): a block with a wrong record holds with probability at most 2^-128. Record level: every
// record of the first maxBlocks failing blocks is judged by its own pairings, without weights: exact.
constexpr u64 RATIO_BLOCK = 256;
constexpr u64 RATIO_MAX_BLOCKS = 64;           // the default of maxBlocks: at most 16 384 records in one launch
constexpr int RATIO_Q2_WORDS = 72;             // Q, then the generator of G2, in the pairing code's limb form (pairing.hpp: G2_WORDS each)
struct RatioOut {
    u64 blocks = 0, badBlocks = 0, resolvedBlocks = 0;
    u64 badRecords = 0;                         // over the resolved blocks: the total when exact
    bool exact = true;                          // every failing block was resolved
    std::vector<uint8_t> blockBad;              // one byte per block: 1 = the block fails
    std::vector<u64> resolved;                  // the resolved blocks, ascending
    std::vector<uint8_t> recordBad;             // one byte per record of the resolved blocks, block after block: 1 = wrong
    double ms[2] = {0, 0};                      // the block sums; the pairings of both levels (host threads: wall time)
    // the first maxListed wrong records, ascending, as indices into the n pairs
    std::vector<u64> listed(u64 n, u64 maxListed) const;
};

// phase times in ms: parse + index (+ upload), Lagrange, transposed products, G1 multiplications, G2 multiplications,
// download + assembly
constexpr int PHASES = 6;

class Backend {
public:
    virtual ~Backend() {}
    // out: N plain canonical integers, L_k(x) of the size-2^logN domain, scale = (x^N - 1) / N
    virtual void lagrange(int logN, const Fr& x, const Fr& scale, const Fr& omega, uint8_t* out) = 0;
    // out: n zkey-format affine records of scalar * G (64 bytes for G1, 128 for G2); scalars plain, below r; window 0: the default;
    // ms (may be null): two values, the table build and the multiplication (host threads: 0 and the whole)
    virtual void generatorMul(bool g2, const uint8_t* scalars, u64 n, int window, uint8_t* out, double* ms) = 0;
    // the point sections: a, b1, k (64 nVars bytes each), b2 (128 nVars), h (64 N). k[s] = (K_s / the divisor of cls[s]) * G1.
    virtual void points(const Plan& p, const ColMatrix cm[3], const std::vector<Piece>& pieces, uint8_t* a, uint8_t* b1, uint8_t* b2,
                        uint8_t* k, uint8_t* h, double ms[PHASES]) = 0;
    // out[c] = sum over the terms [colPtr[c], colPtr[c + 1]) of coef * point[index], a zkey-format affine record (64 bytes for G1,
    // 128 for G2); coefs plain, below r; points zkey-format records that passed the point check, all-zero = infinity. An empty
    // column and a sum that is the neutral element give the all-zero record. ms (may be null): two values, the per-term
    // products and the per-column sums (host threads: 0 and the whole)
    virtual void combine(bool g2, u64 nCols, const u32* colPtr, const u32* index, const uint8_t* coefs, const PointSegs& pts, uint8_t* out,
                         double* ms) = 0;
    // out[i] = scalar * point[i] over n G1 records; scalar plain, below r; infinity in gives infinity out. ms (may be null): one value
    virtual void scale(const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out, double* ms) = 0;
    // the whole delta step of an UltraGroth key: n <= MAX_SCALE_SEGS segments, each with a scalar of its own and an optional index
    // list into its source records (the device: one launch for all of them). A scalar of 1 copies the gathered records, 0 gives
    // all-zero records, infinity in gives infinity out. An output may be its own segment's source only without an index list.
    // ms (may be null): one value
    virtual void scaleSegments(const ScaleSeg* segs, int n, double* ms) = 0;
    // The ratio test over n pairs of zkey-format G1 records that passed the point check (all-zero = infinity; both infinity holds,
    // exactly one is wrong). q: a G2 record, not infinity, in the subgroup. maxBlocks 0: RATIO_MAX_BLOCKS. Both backends give the
    // same answers (their weights differ; the answers do not depend on them).
    virtual void ratio(const uint8_t* x, const uint8_t* y, u64 n, const uint8_t* q, u64 maxBlocks, RatioOut& out) = 0;
    // The inverse transform over points that prepares a .ptau (ptau_prepare_host.cpp). N = 2^logN, omega = 5^((r - 1) / N):
    // out[v][k] = (1 / N) sum_j omega^(-j k) in[v][j] for each of the nVec vectors; in[v]: nGiven <= N zkey-format records, the rest
    // of the N taken as infinity; out[v]: N records, which do not overlap any input. ms (may be null): two values, the 1 / N
    // products and the stages (host threads: 0 and the whole)
    virtual void intt(bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out, double* ms) = 0;
};
Backend& hostBackend();
// the generator of G1 (16 words) or G2 (32 words): affine, canonical device form, packed
void generatorWords(bool g2, u32* out);
// the device backend, set by setup.hip when that is linked in (null in a host-only program)
typedef Backend* (*DeviceBackendFactory)(int device);
extern DeviceBackendFactory deviceBackendFactory;

// ---- field helpers on canonical values (host) ----
Fr frFromPlain(const uint8_t* le);                       // any value below 2^256, taken mod r
void frToPlain(uint8_t* le, const Fr& a);
inline Fr frMul(const Fr& a, const Fr& b) { return ug::cond_sub_q(ug::mul(a, b)); }
inline Fr frAdd(const Fr& a, const Fr& b) { return ug::cond_sub_q(ug::norm_strict(ug::add(a, b))); }
inline Fr frSub(const Fr& a, const Fr& b) { return ug::cond_sub_q(ug::norm_strict(ug::sub<1>(a, b))); }

void parallelFor(u64 n, u64 grain, const std::function<void(u64, u64)>& fn);

// ---- what a point combination's two backends share ----
// A coefficient above r / 2 is taken as the negated point times r - coef: mag = min(coef, r - coef) as 8 plain words, the return
// value says whether the point is negated. coef plain, below r.
bool coefMagnitude(const uint8_t* le, u32 mag[8]);
inline int bitLength(const u32 w[8]) {
    for (int i = 7; i >= 0; i--)
        if (w[i]) return 32 * i + 32 - __builtin_clz(w[i]);
    return 0;
}
// the pieces of every column of colPtr with more than SPLIT_THRESHOLD terms, appended (the split rule of buildColumns)
void columnPieces(const u32* colPtr, u64 nCols, u32 m, std::vector<Piece>& pieces);
// width-w non-adjacent form of a scalar below 2^255: digit[i] is 0 or odd with |digit[i]| < 2^(w-1), scalar = sum digit[i] 2^i.
// Returns the index of the top non-zero digit, -1 for the scalar 0.
constexpr int SCALE_WINDOW = 4;                // the device's width: odd multiples 1, 3, 5, 7 in registers
int recodeWnaf(const uint8_t* le, int w, int8_t digit[256]);

// ---- what the ratio test's two backends share ----
// n values below 2^128, 16 bytes each, from getrandom: fresh in every call, never derived from the inputs
void drawWeights128(std::vector<uint8_t>& out, u64 n);
// q (a zkey-format G2 record) and the generator of G2 as the pairing code reads them
void ratioG2Words(const uint8_t* q, u32 out[RATIO_Q2_WORDS]);
// the constants of the is-one test, made once by host code (pairing.hpp: final_exp_consts)
const ug::pr::FinalExpConsts& ratioConsts();
// sums(weights, sumX, sumY, ms): the two weighted sums of every block as zkey-format records (blocks x 64 bytes each; weights: n x 16 bytes)
typedef std::function<void(const uint8_t*, uint8_t*, uint8_t*, double*)> RatioSums;
// judge(x, y, m, wrong, ms): wrong[i] = 1 unless e(x_i, Q) = e(y_i, G2), over m pairs of records
typedef std::function<void(const uint8_t*, const uint8_t*, u64, uint8_t*, double*)> RatioJudge;
// the two levels over a backend's two steps: draws the weights, judges the block sums, gathers the records of the first
// maxBlocks failing blocks and judges them
void ratioLevels(const uint8_t* x, const uint8_t* y, u64 n, u64 maxBlocks, RatioOut& out, const RatioSums& sums, const RatioJudge& judge);

// ---- what the inverse transform's two backends share ----
// A folded scalar: 8 plain words of a magnitude below 2^255, bit 255 set when the point is negated (coefMagnitude's fold).
// tw: the 2^(logN-1) twiddles omega^(-j), folded, 8 words each (stage s of the transform reads every 2^(logN-1-s)-th).
void inttTwiddles(int logN, std::vector<u32>& tw);
// 1 / 2^logN, folded: the negated point times (r - 1) / 2^logN
void inttScale(int logN, u32 folded[8]);
// a transform of one point (logN = 0) is the point itself: true when it was done here
bool inttTrivial(bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out);
struct PtauError : public std::invalid_argument {
    explicit PtauError(const std::string& m) : std::invalid_argument("ptau: " + m) {}
};

// ---- the point check of a file's records (point_check.cpp; it names the library's device entries, so a host-only program that
// links it supplies them) ----
// Through ug_points_check (device >= 0) or on host threads, with the messages of ug_setup_ptau_run: n records of section `id`;
// record i is the section's record first + stride * i. level 0 checks nothing.
class PointCheck {
public:
    PointCheck(int device, int level);
    ~PointCheck();
    void operator()(bool g2, const uint8_t* rec, u64 n, u32 id, u64 first, u64 stride) const;
    // the same check for a caller with messages of its own (zkey_verify_host.cpp): the lowest bad record and the first rule it breaks
    ug_point_fault find(bool g2, const uint8_t* rec, u64 n) const;
    static const char* reasonText(int reason);
    PointCheck(const PointCheck&) = delete;
    PointCheck& operator=(const PointCheck&) = delete;
private:
    int device_, level_;
    ug_ctx* ctx_ = nullptr;
};
// H's sources side by side: out[k] = record 2 k + 1 of sl.top, k < sl.n
void gatherOddTop(const PtauSlices& sl, uint8_t* out);
// every point a phase-2 setup of sl's domain reads: the four level-n slices, the odd records of the padded level (gathered: hOdd),
// record 0 of sections 4 and 5, section 6
void checkSlices(const PointCheck& check, const PtauSlices& sl, const uint8_t* hOdd);

// ---- the parts of a key that do not depend on where its points come from (setup_host.cpp), for setup_ptau.cpp ----
bool belowR(const uint8_t* le);
void planSizes(const R1csHeader& h, u32 logDomain, Plan& p);       // nVars .. N and cls (all wires of protocol 1) from the header
// protocol 1337 on a plan whose sizes are set: rand_indx is a public signal, the two lists partition the private signals (an empty
// list is legal); fills ultra, randIndx, the lists and cls. The rules and messages of ug_setup_run.
void planLists(Plan& p, u32 randIndx, const u32* roundSignals, u64 nRound, const u32* finalSignals, u64 nFinal);
void loadCircuit(const void* r1cs, u64 size, std::unique_ptr<BinFile>& f, R1csHeader& h);
void buildColumns(const R1cs& cs, const Plan& p, ColMatrix cm[3], std::vector<Piece>& pieces);
u64 countCoefs(const R1cs& cs, std::vector<u64>& perPiece);        // returns the sum of perPiece: the records of the constraint rows
// section 4's records (44 bytes each, without the count in front): the sum of perPiece for the constraints, then nPublic + 1
void writeCoefs(const R1cs& cs, const Plan& p, const std::vector<u64>& perPiece, uint8_t* out);
struct Layout {
    u64 nCoefs = 0, total = 0;
    std::vector<std::pair<u32, u64>> sections;      // id, payload size, in file order
    u64 offsetOf(u32 id) const;                     // of the payload
};
Layout makeLayout(const Plan& p, u64 nCoefs);
u64 vkeyBound(const Plan& p);
struct HeaderPoints { uint8_t g1[4][64], g2[4][128]; };        // alpha, beta, round delta, final delta | beta, gamma, round delta, final delta
void writeContainer(uint8_t* zkey, const Layout& lay);            // magic, version, the section headers
// sections 1 - 4 and the C sections from krec (one K record per wire), and the verification key's JSON. cPointsDone: the C point
// sections are in place already (a delta step that gathered them: Backend::scaleSegments), only the index sections are written
void finishKey(const R1cs& cs, const Plan& p, const Layout& lay, const std::vector<u64>& perPiece, const HeaderPoints& hp,
               const std::vector<uint8_t>& krec, uint8_t* zkey, std::string* vkey, bool cPointsDone = false);
Backend& backendFor(int device, std::unique_ptr<Backend>& owned);
// (setup_ptau.cpp) the columns of a combination that gives K_s over the three level-n slices side by side [T | aT | bT] of N records
// each: column i is wire s = wires ? wires[i] : first + i, M columns; an A term (k, s) names bT[k], a B term aT[k], a C term T[k]
void mergedColumns(const ColMatrix cm[3], const u32* wires, u64 first, u64 M, u64 N, std::vector<u32>& colPtr, std::vector<u32>& index,
                   std::vector<uint8_t>& coefs);
// the verification key's JSON into the caller's buffer (may be null: only the length is reported), with its terminating 0
void copyVkey(const std::string& vkey, char* dst, u64 capacity, uint64_t* bytes);
// uniform below r, never 0: 254 random bits, drawn again when out of range
void drawNonZeroScalar(uint8_t le[32]);

// ---- small helpers of all four host files ----
inline bool allZero(const uint8_t* p, size_t n) {
    uint8_t o = 0;
    for (size_t i = 0; i < n; i++) o |= p[i];
    return o == 0;
}
inline void put32(uint8_t*& o, u32 v) { memcpy(o, &v, 4); o += 4; }
inline void put64(uint8_t*& o, u64 v) { memcpy(o, &v, 8); o += 8; }
inline void putBytes(uint8_t*& o, const void* s, size_t n) { memcpy(o, s, n); o += n; }
double nowMs();
// phase times: lap(i) adds the time since the last lap (or since restart()) to ms[i]
class PhaseClock {
public:
    explicit PhaseClock(double* ms) : ms_(ms), t_(nowMs()) {}
    void lap(int phase) { const double n = nowMs(); ms_[phase] += n - t_; t_ = n; }
    void restart() { t_ = nowMs(); }
private:
    double* ms_;
    double t_;
};
// what every options struct starts with: refuses a null pointer, another size, and a `validate` outside lo .. hi ("is not " + words)
template <class Err, class Opt> void checkOptionsHead(const Opt* o, u32 lo, u32 hi, const char* words) {
    if (!o) throw Err("null options");
    if (o->size != sizeof(Opt)) throw Err("options struct of another size (" + std::to_string(o->size) + ")");
    if (o->validate < lo || o->validate > hi) throw Err("validate " + std::to_string(o->validate) + " is not " + words);
}

// ---- the guard of every extern "C" entry ----
// A path's prefix rule: a message that starts with one of `keep` stays as it is; any other gets `put` in front, after a leading
// "setup: " is dropped where `dropSetup` says so (the key check reports a shared helper's refusal under the file it read).
struct PrefixRule {
    const char* put;
    const char* keep[3];
    bool dropSetup;
};
constexpr PrefixRule SETUP_RULE = {"setup: ", {"setup: ", "r1cs: ", "ptau: "}, false};
std::string underPrefix(const PrefixRule& rule, const std::string& m);
void copyErr(char* dst, unsigned long long max, const char* msg);
// runs body(); an exception becomes UG_ERROR with its message, under the rule, in error_msg
template <class Body> int guarded(const PrefixRule& rule, char* error_msg, unsigned long long error_msg_maxsize, Body&& body) {
    try {
        body();
        return UG_OK;
    } catch (std::exception& e) {
        copyErr(error_msg, error_msg_maxsize, underPrefix(rule, e.what()).c_str());
    } catch (...) {
        copyErr(error_msg, error_msg_maxsize, (std::string(rule.put) + "unknown error").c_str());
    }
    return UG_ERROR;
}

}  // namespace setup
}  // namespace ughost
