// pairing_dev.hpp -- the device pass of batch verification (pairing.hip) as the host code of verifier_api.cpp sees it (BatchCall
// and the test hooks; the record layouts also name the formats that verifier_records.cpp reads on the host).
#pragma once
#include <cstddef>
#include <stdexcept>
#include <vector>
#include "pairing.hpp"

namespace ug {

// The trees of a pass whose proofs belong to several keys: one tree per SEGMENT (the proofs of one key, contiguous in the pass),
// kept as a forest, level by level. Level 0 is the n leaves in pass order; level l + 1 holds, in segment order, the (m + 1) / 2
// nodes of every segment that has m > 1 nodes on level l -- an odd last node is copied up inside its segment, and a segment that
// has reached one node stops there, so it is absent from the levels above. One segment: the layout of tree_nodes, offset for
// offset. A launch of the forest kernels (pairing.hip) makes one level of every segment; lane t of a launch writes node
// level_base[l + 1] + t and finds its segment in `start`.
struct ForestPlan {
    std::vector<size_t> size, first;               // per segment: its proofs, and the position of its first one in the pass
    std::vector<std::vector<size_t>> off;          // off[s][l]: the node (index into the forest) where level l of segment s begins
    std::vector<size_t> level_base;                // where level l begins; level_base.size() - 1 = launches per tree
    size_t nodes = 0;
    // the kernels' table of the step l -> l + 1, over the segments that go on: start[i] = the first lane of segment i (one entry
    // past the last: all lanes), src[i] = off[s][l], n_src[i] = its nodes on level l
    struct Step { std::vector<u32> start, src, n_src; };
    std::vector<Step> step;

    ForestPlan() {}
    ForestPlan(const u32* sizes, size_t n_segs) {
        size.assign(sizes, sizes + n_segs);
        first.resize(n_segs);
        off.resize(n_segs);
        std::vector<size_t> m(size);                                // nodes of every segment on the current level
        for (size_t s = 0; s < n_segs; s++) {
            if (!size[s]) throw std::invalid_argument("ForestPlan: empty segment");
            first[s] = nodes; off[s].push_back(nodes); nodes += size[s];
        }
        level_base.push_back(0);
        for (;;) {
            Step st;
            const size_t base = nodes;
            for (size_t s = 0; s < n_segs; s++) {
                if (m[s] <= 1) { m[s] = 0; continue; }              // stopped, now or before
                st.start.push_back((u32)(nodes - base)); st.src.push_back((u32)off[s].back()); st.n_src.push_back((u32)m[s]);
                m[s] = (m[s] + 1) / 2;
                off[s].push_back(nodes); nodes += m[s];
            }
            if (st.src.empty()) break;
            st.start.push_back((u32)(nodes - base));
            level_base.push_back(base);
            step.push_back(std::move(st));
        }
    }
    size_t launches() const { return step.size(); }
};

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
    // Several keys: the pass's segments, null = one segment of n proofs. With a plan the trees are its forest (plan->nodes nodes) and
    // are made by the forest kernels, one launch per level whatever the number of segments; tree_launches counts them, both trees.
    const ForestPlan* plan = nullptr;
    // leaves given (the test hook ug_test_tree_forest): n x F12_WORDS and n x k x XYZZ_WORDS, no Miller launch, only the forest
    // kernels; needs a plan, a one-segment plan too
    const u32* leaf_f = nullptr;
    const u32* leaf_g = nullptr;
    int tree_launches = 0;      // out
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
    const ForestPlan* plan = nullptr;   // the segments of the next run over its `kept` records (PairingBatch::plan); null = one segment
    int tree_launches = 0;              // out: the tree launches of the last run
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
    // Suspects under several keys in ONE launch of the judge (its keyed instantiation): n_keys > 1, the suspects ordered by key.
    // key_first[q] .. key_first[q + 1] are the suspects of key q, key_cols[q] its columns (`cols` is then unused); points, key_g2 and
    // f_alpha_beta hold every key's part one behind the other, scalars every suspect's key_cols x 8 words. The vkx step runs per key.
    int n_keys = 1;
    const int* key_first = nullptr;    // n_keys + 1
    const int* key_cols = nullptr;     // n_keys
};
void pairing_judge_device(int device, const pr::FinalExpConsts& consts, PairingJudge& pj);

// f2_sqrt of pairing.hpp, one lane per element (test hook): in count x 16 words, plain c0 | c1; out the root that is not the larger
// one, plain (zeros when there is none); has_root one byte each.
void fq2_sqrt_device(int device, const pr::DecompressConsts& c, int count, const u32* in, u32* out, unsigned char* has_root);

// One lane of the device's final exponentiation (test hook): g = the value after the hard part, is_one = the verdict.
void final_exp_device(int device, const pr::FinalExpConsts& consts, const u32* f, u32* g, int* is_one);

}  // namespace ug
