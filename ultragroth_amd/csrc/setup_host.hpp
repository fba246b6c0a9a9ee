// setup_host.hpp -- the development setup (.r1cs + a KNOWN trapdoor -> a TEST proving key): the host layer.
//
// Everything but the three heavy steps is host code and lives in setup_host.cpp: the checks, the derived field constants, the
// column-major index of A, B, C, section 4, the headers, the verification key. The heavy steps -- Lagrange evaluation, the
// transposed sparse products and the fixed-base multiplications of the generators -- sit behind Backend: HostBackend runs them
// on host threads through the UG_HD field and curve code (device = -1, and the only backend a program that links no HIP code
// has), the device backend of setup.hip runs them as kernels. Both compute the same residues, and every record is canonical,
// so the two give the same bytes.
// Every failure is a C++ exception whose message starts with "setup: " (or with "r1cs: ", from the loader).
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "ec.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"

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

}  // namespace setup
}  // namespace ughost
