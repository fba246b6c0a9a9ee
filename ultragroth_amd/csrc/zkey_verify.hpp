// zkey_verify.hpp -- what the check of a Groth16 key against its circuit and powers of tau (zkey_verify_host.cpp) hands to the code
// that evaluates the twelve sums of its relations (fourteen for an UltraGroth key, ug_ultra_zkey_verify_run): host threads (zkey_verify_host.cpp) or the device (zkey_verify.hip).
#pragma once
#include <cstdint>
#include "host_util.hpp"

namespace ughost {
namespace zkv {

// everything both evaluators read; every size and every point has been checked before one of them runs
struct Inputs {
    uint64_t M = 0, N = 0, pub = 0;               // nVars, the domain, nPublic + 1
    int logN = 0;
    const void* r1cs = nullptr;                   // the file (the device parses it into its own form: ug_r1cs_create)
    uint64_t r1csSize = 0;
    const R1cs* cs = nullptr;                     // the same circuit, parsed (host threads)
    const uint8_t *ic = nullptr, *a = nullptr, *b1 = nullptr, *b2 = nullptr, *c = nullptr, *h = nullptr;      // sections 3, 5, 6, 7, 8, 9
    const uint8_t *T = nullptr, *T2 = nullptr, *aT = nullptr, *bT = nullptr;                                  // level n of sections 12 - 15
    const uint8_t* top = nullptr;                 // level n + 1 of section 12: 2 N records, H's sources are the odd ones
    const uint8_t* rho = nullptr;                 // M plain 32-byte integers below 2^128
    const uint8_t* sigma = nullptr;               // N of them
    // An UltraGroth key (ug_ultra_zkey_verify_run): c is section 8 (C1, n1 records), c2 section 9 (C2, n2), h section 12; cls has one
    // byte per wire, 0 public, 1 round, 2 final; rhoRound[i] = rho[round list[i]], rhoFinal likewise (the gather is a host step)
    bool ultra = false;
    const uint8_t* c2 = nullptr;
    uint64_t n1 = 0, n2 = 0;
    const uint8_t* cls = nullptr;
    const uint8_t *rhoRound = nullptr, *rhoFinal = nullptr;
};

// the sums of the relations as zkey-format records (all-zero = infinity); canonical, so both evaluators give the same bytes
struct Sums {
    uint8_t keyA[64], keyB1[64], keyB2[128], keyIC[64], keyC[64], keyH[64];      // MSM(rho, A) .. MSM(sigma, H)
    uint8_t aT[64], bT[64], bT2[128];                                            // MSM(a, T), MSM(b, T), MSM(b, T2)
    uint8_t kPub[64], kPriv[64];                                                 // K^pub, K^priv
    uint8_t hP[64];                                                              // MSM(sigma, odd records of P)
    uint8_t keyC2[64], kFinal[64];               // an UltraGroth key: keyC, kPriv are C1's and K^round, these C2's and K^final
};

// ms: fold (circuit upload + kernel), slice products, key products, H products; fold_kernel_ms: the kernel alone
struct SumsStats { double ms[4] = {0, 0, 0, 0}; double foldKernelMs = 0; uint64_t peakDeviceBytes = 0; };

typedef void (*DeviceSums)(int device, const Inputs& in, Sums& out, SumsStats& st);
typedef void (*DeviceFold)(int device, const void* r1cs, uint64_t r1csSize, const uint8_t* rho, uint32_t nPublic, uint32_t logN, uint8_t* out8,
                           double* kernelMs);
// set by zkey_verify.hip when that is linked in (null in a host-only program)
extern DeviceSums deviceSums;
extern DeviceFold deviceFold;
// the same for an UltraGroth key: the fold with a class per wire (eleven vectors: a^m, b^m, c^m for m = pub, round, final, then a, b)
typedef void (*DeviceFoldClasses)(int device, const void* r1cs, uint64_t r1csSize, const uint8_t* rho, const uint8_t* cls, uint32_t nPublic,
                                  uint32_t logN, uint8_t* out11, double* kernelMs);
extern DeviceSums deviceUltraSums;
extern DeviceFoldClasses deviceFoldClasses;

}  // namespace zkv
}  // namespace ughost
