// pairing_dev.hpp -- the device pass of batch verification (pairing.hip) as the host code of verifier_api.cpp sees it.
#pragma once
#include <cstddef>
#include "pairing.hpp"

namespace ug {

struct PairingBatch {
    int n = 0;                  // proofs of this pass, at most PAIRING_PASS
    int k = 1;                  // G1 sums per proof: 1 (Groth16: C) or 2 (UltraGroth: pi_f, pi_r)
    const u32* a = nullptr;     // n x G1_WORDS
    const u32* b = nullptr;     // n x G2_WORDS
    const u32* g = nullptr;     // n x k x G1_WORDS
    const u32* r = nullptr;     // n x 4: the 128-bit scalars
    u32* f_tree = nullptr;      // out: tree_nodes(n) x F12_WORDS, level 0 first
    u32* g_tree = nullptr;      // out: tree_nodes(n) x k x XYZZ_WORDS
    double kernel_ms[3] = {0, 0, 0};   // out: miller_batch_kernel, the Fq12 tree, the G1 tree
};
constexpr int PAIRING_PASS = 1 << 16;

// Runs the kernels of pairing.hip on `device` and brings both trees back. Throws on a device error.
void pairing_batch_device(int device, const pr::PairingConsts& kc, PairingBatch& pb);

}  // namespace ug
