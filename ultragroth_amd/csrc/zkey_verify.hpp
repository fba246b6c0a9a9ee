// zkey_verify.hpp -- what the check of a key against its circuit and powers of tau (zkey_verify_host.cpp: ug_zkey_verify_run for a
// Groth16 key, ug_ultra_zkey_verify_run for an UltraGroth key) hands to the code that evaluates the sums of its relations: host
// threads (zkey_verify_host.cpp) or the device (zkey_verify.hip). The protocol is data here -- the number of weight classes and the
// list of C sections -- so neither evaluator asks which key it has: 12 sums for Groth16, 14 for UltraGroth.
#pragma once
#include <cstdint>
#include "host_util.hpp"

namespace ughost {
namespace zkv {

constexpr int MAX_CLASSES = 3, MAX_C_SECTIONS = 2;

// one C section of the key: n G1 records that stand against the class sum K^(1 + its place in the list), under weights
struct CSection {
    const uint8_t* points = nullptr;
    uint64_t n = 0;
    const uint8_t* weights = nullptr;             // n plain 32-byte integers: one per record
    // >= 0: the weights are rho's own run from this wire on (weights = rho + 32 * rhoFirst), and record 0 is that wire: the device
    // reads its copy of rho in place. < 0: they were gathered through a list of the key (a host step) and the device uploads them.
    int64_t rhoFirst = -1;
};

// everything both evaluators read; every size and every point has been checked before one of them runs
struct Inputs {
    uint64_t M = 0, N = 0, pub = 0;               // nVars, the domain, nPublic + 1
    int logN = 0;
    const void* r1cs = nullptr;                   // the file (the device parses it into its own form: ug_r1cs_create)
    uint64_t r1csSize = 0;
    const R1cs* cs = nullptr;                     // the same circuit, parsed (host threads)
    const uint8_t *ic = nullptr, *a = nullptr, *b1 = nullptr, *b2 = nullptr, *h = nullptr;      // sections 3, 5, 6, 7 and H (9 or 12)
    const uint8_t *T = nullptr, *T2 = nullptr, *aT = nullptr, *bT = nullptr;                    // level n of sections 12 - 15
    const uint8_t* top = nullptr;                 // level n + 1 of section 12: 2 N records, H's sources are the odd ones
    const uint8_t* rho = nullptr;                 // M plain 32-byte integers below 2^128
    const uint8_t* sigma = nullptr;               // N of them
    // the weight classes of the wires. Groth16: K = 2 (public, private), cls null: wire s is public when s < pub. UltraGroth:
    // K = 3 (public, round, final), cls one byte per wire. The C sections in the key's order: K - 1 of them.
    int K = 2;
    const uint8_t* cls = nullptr;
    CSection c[MAX_C_SECTIONS];
};

// the sums of the relations as zkey-format records (all-zero = infinity); canonical, so both evaluators give the same bytes
struct Sums {
    uint8_t keyA[64], keyB1[64], keyB2[128], keyIC[64], keyH[64];                // MSM(rho, A) .. MSM(sigma, H)
    uint8_t aT[64], bT[64], bT2[128];                                            // MSM(a, T), MSM(b, T), MSM(b, T2)
    uint8_t k[MAX_CLASSES][64];                                                  // K^m: K^pub, then one per C section
    uint8_t keyC[MAX_C_SECTIONS][64];                                            // MSM(its weights, C section i)
    uint8_t hP[64];                                                              // MSM(sigma, odd records of P)
};

// ms: fold (circuit upload + kernel), slice products, key products, H products; fold_kernel_ms: the kernel alone
struct SumsStats { double ms[4] = {0, 0, 0, 0}; double foldKernelMs = 0; uint64_t peakDeviceBytes = 0; };

typedef void (*DeviceSums)(int device, const Inputs& in, Sums& out, SumsStats& st);
// the fold alone (test tooling): cls null gives the eight vectors of a Groth16 key, cls a class byte per wire the eleven of an
// UltraGroth key (vector 3 m + t is matrix t over class m; then a, b)
typedef void (*DeviceFold)(int device, const void* r1cs, uint64_t r1csSize, const uint8_t* rho, const uint8_t* cls, uint32_t nPublic,
                           uint32_t logN, uint8_t* out, double* kernelMs);
// set by zkey_verify.hip when that is linked in (null in a host-only program)
extern DeviceSums deviceSums;
extern DeviceFold deviceFold;

}  // namespace zkv
}  // namespace ughost
