// pairing_dev.hpp -- the device pass of batch verification (pairing.hip) as the host code of verifier_api.cpp sees it (BatchCall
// and the test hooks; the record layouts also name the formats that verifier_records.cpp reads on the host).
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

// the record layouts of include/verifier.h (UG_RECORDS_*) and their sizes in 32-bit words for a proof with k G1 points besides pi_a
enum { RECORDS_PLAIN = 0, RECORDS_EVM = 1, RECORDS_COMPRESSED = 2 };
constexpr size_t record_words(int k, int format) { return format == RECORDS_COMPRESSED ? 24 + 8 * (size_t)k : 48 + 16 * (size_t)k; }

// Runs the kernels of pairing.hip on `device` and brings both trees back. Throws on a device error.
void pairing_batch_device(int device, const pr::PairingConsts& kc, PairingBatch& pb);

// The resident form, for packed proof records (include/verifier.h): the raw records of a pass are uploaded once, and the arrays the
// Miller kernel reads are made on the device and stay there.
//   ingest   records_ingest_kernel (compressed records: records_decompress_kernel), then the subgroup ladder of check.hip in its mask form over the pi_b that passed;
//            status[i] = UG_POINT_OK, UG_POINT_OFF_CURVE (any point of record i) or UG_POINT_OFF_SUBGROUP (its pi_b).
//   run      the kernels of pairing_batch_device over the records keep[0..kept) (ascending positions within the pass), compacted by a
//            gather kernel first; keep == nullptr: all n records, the arrays used in place. r: kept x 4 words.
//   download the arrays as ingest left them (n x G1_WORDS, n x G2_WORDS, n x k x G1_WORDS; a null pointer skips one): the rows of
//            pi_r for the UltraGroth challenge of compressed records, and the test hook.
class ResidentBatch {
public:
    ResidentBatch(int device, int n, int k, int format = RECORDS_PLAIN);
    ~ResidentBatch();
    ResidentBatch(const ResidentBatch&) = delete;
    void ingest(const void* records, unsigned char* status);
    void download(u32* a, u32* b, u32* g);
    void run(const pr::PairingConsts& kc, const u32* keep, int kept, const u32* r, u32* f_tree, u32* g_tree, double kernel_ms[3]);
private:
    struct Impl;
    Impl* impl = nullptr;
};

// The suspects of a rejected pass, each judged by its own equation (pairing.hpp: judge_proof), one lane per suspect.
struct PairingJudge {
    int n = 0;                  // suspects of this launch, at most PAIRING_PASS
    int k = 1;                  // G1 points per proof besides A, as in PairingBatch
    int cols = 0;               // columns of vkX: IC_0, IC_1 .. IC_nPublic [, IC_rand]
    const u32* a = nullptr;     // n x G1_WORDS
    const u32* b = nullptr;     // n x G2_WORDS
    const u32* g = nullptr;     // n x k x G1_WORDS
    const u32* scalars = nullptr;   // n x cols x 8: plain 256-bit integers; column 0 is 1, then the signals [, the challenge]
    const u32* points = nullptr;    // cols x G1_WORDS: the key's points of the columns
    const u32* key_g2 = nullptr;    // (1 + k) x G2_WORDS: gamma, then the delta of each of the k points
    const u32* f_alpha_beta = nullptr;   // F12_WORDS: miller(beta, -alpha), computed once per call on the host
    u32* verdict = nullptr;     // out: n words, 1 = the equation holds
    double kernel_ms[2] = {0, 0};   // out: the vkx step (both kernels), judge_kernel
};
void pairing_judge_device(int device, const pr::FinalExpConsts& consts, PairingJudge& pj);

// f2_sqrt of pairing.hpp, one lane per element (test hook): in count x 16 words, plain c0 | c1; out the root that is not the larger
// one, plain (zeros when there is none); has_root one byte each.
void fq2_sqrt_device(int device, const pr::DecompressConsts& c, int count, const u32* in, u32* out, unsigned char* has_root);

// One lane of the device's final exponentiation (test hook): g = the value after the hard part, is_one = the verdict.
void final_exp_device(int device, const pr::FinalExpConsts& consts, const u32* f, u32* g, int* is_one);

}  // namespace ug
