// pairing.hip -- the device pass of batch verification: one Miller loop per lane, then the trees of partial products.
//
// miller_batch_kernel   lane i: r_i A_i (128-bit ladder, then affine), f_i = miller(B_i, r_i A_i), and r_i times the proof's
//                       other G1 points as XYZZ records. The arithmetic is pairing.hpp, the host verifier's own.
// f12_tree_kernel       one level of the binary tree over the f_i: node j = node 2j * node 2j+1 of the level below, an odd last
// g1_tree_kernel        node copied up; the G1 twin adds. One launch per level; every level stays in HBM, so that a rejected
//                       batch can be searched from the root without the device.
// f12_forest_kernel     the same level for a pass of several keys: every segment (the proofs of one key) has its own tree, and one
// g1_forest_kernel      launch makes a level of all of them; a lane finds its segment in the step's table (pairing_dev.hpp:
//                       ForestPlan). Launches per tree: ceil(log2(largest segment)), whatever the number of keys.
// vkx_mul_kernel        the judge of a rejected pass, first step: lane (i, c) = column c of suspect i's vkX, scalar_ic * IC_c by the
// vkx_sum_kernel        256-bit ladder; then one block per suspect adds its columns (lanes stride the columns, a tree over the 64
//                       partial sums in LDS) and leaves -vkX_i as an affine G1 record.
// judge_kernel          lane i: suspect i's own equation -- the Miller loops of its three (four) pairs times miller(beta, -alpha),
//                       the final exponentiation's is-one test, one verdict word. No random scalar: the single verifier's answer.
//                       judge_kernel<true> takes the key's G2 points and miller(beta, -alpha) from a table by a per-suspect index.
// ratio_judge_kernel    lane i: e(x_i, Q) = e(y_i, G2) for two G1 records of a key -- two Miller loops, the is-one test, one word
//                       (the ratio test of Backend::ratio).
// final_exp_kernel      one lane of the final exponentiation alone (ug_test_final_exp).
// records_ingest_kernel the packed records of ug_*_verify_batch_records -> the arrays above, one record per lane: reduction mod q,
// gather_rows_kernel    infinity flags, curve equations, limb form; the gather compacts the arrays when records were dropped.
//                       The layout is a template parameter: plain little-endian coordinates or the big-endian EVM order.
// records_decompress_kernel   the same arrays from compressed records (x and a sign bit per point): the lane takes the square
//                       roots -- f1_sqrt / f2_sqrt of pairing.hpp, fixed-exponent powers -- and a point without one is off its curve.
// fq2_sqrt_kernel       one lane per element of f2_sqrt alone (ug_test_fq2_sqrt).
//
// Registers: an Fq12 value is 108 words, a product holds three and a column sum. The coefficient loops of pairing.hpp are
// kept as loops, so the values are indexed at run time and live in private (scratch) memory; the column products (81
// multiply-adds for 18 words read) run from registers. Every kernel asks for one wave per SIMD -- the whole 512-entry
// file -- so that nothing else is pushed out; tools/kernel_regs.py prints what the compiler made of it
// (profiles/verify_batch.txt).
#include <algorithm>
#include <vector>
#include "dev_common.hpp"
#include "internal.hpp"
#include "pairing_dev.hpp"
#include "../../include/ultragroth_hip.h"

namespace ug {

using namespace pr;

namespace {

#define UG_ONE_WAVE __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))

__global__ UG_ONE_WAVE void miller_batch_kernel(PairingConsts kc, const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ g,
                                                const u32* __restrict__ r, int n, int k, u32* __restrict__ f_out, u32* __restrict__ g_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    u32 rw[4];
#pragma unroll
    for (int j = 0; j < 4; j++) rw[j] = r[i * 4 + j];
    batch_leaf(kc, a + i * G1_WORDS, b + i * G2_WORDS, g + i * k * G1_WORDS, k, rw, f_out + i * F12_WORDS, g_out + i * k * XYZZ_WORDS);
}

__global__ UG_ONE_WAVE void f12_tree_kernel(PairingConsts kc, const u32* __restrict__ src, int n_src, u32* __restrict__ dst) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ((size_t)n_src + 1) / 2) return;
    f12_node(kc, src + 2 * j * F12_WORDS, 2 * j + 1 < (size_t)n_src ? src + (2 * j + 1) * F12_WORDS : nullptr, dst + j * F12_WORDS);
}

__global__ __launch_bounds__(64) void g1_tree_kernel(const u32* __restrict__ src, int n_src, int k, u32* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (((size_t)n_src + 1) / 2) * k) return;
    const size_t j = t / k, s = t % k;
    g1_node(src + (2 * j * k + s) * XYZZ_WORDS, 2 * j + 1 < (size_t)n_src ? src + ((2 * j + 1) * k + s) * XYZZ_WORDS : nullptr,
            dst + (j * k + s) * XYZZ_WORDS);
}

// The segment-aware forms: one launch makes level l + 1 of EVERY segment of a pass (pairing_dev.hpp: ForestPlan). Lane t writes
// node dst + t; its segment is the last i with start[i] <= t, found by bisection in the step's table (segs >= 1 entries and the
// total behind them, so every t < start[segs] has one), and its children are nodes src[i] + 2 j and 2 j + 1 of the level below.
struct ForestStep {
    const u32* start;           // segs + 1
    const u32* src;             // segs: where the segment's nodes of the level below begin
    const u32* n_src;           // segs: how many there are
    u32 segs, dst;              // dst: where the level above begins
};
__device__ __forceinline__ bool forest_lane(const ForestStep& st, u32 t, size_t& left, bool& pair) {
    if (t >= st.start[st.segs]) return false;
    u32 lo = 0, hi = st.segs;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (st.start[mid] <= t) lo = mid; else hi = mid;
    }
    const u32 j = t - st.start[lo];
    left = (size_t)st.src[lo] + 2 * (size_t)j;
    pair = 2 * j + 1 < st.n_src[lo];
    return true;
}

__global__ UG_ONE_WAVE void f12_forest_kernel(PairingConsts kc, const u32* __restrict__ src, ForestStep st, u32* __restrict__ dst) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    size_t left;
    bool pair;
    if (!forest_lane(st, t, left, pair)) return;
    f12_node(kc, src + left * F12_WORDS, pair ? src + (left + 1) * F12_WORDS : nullptr, dst + ((size_t)st.dst + t) * F12_WORDS);
}

__global__ __launch_bounds__(64) void g1_forest_kernel(const u32* __restrict__ src, ForestStep st, int k, u32* __restrict__ dst) {
    const u32 lane = blockIdx.x * blockDim.x + threadIdx.x, t = lane / (u32)k, s = lane % (u32)k;
    size_t left;
    bool pair;
    if (!forest_lane(st, t, left, pair)) return;
    g1_node(src + (left * k + s) * XYZZ_WORDS, pair ? src + ((left + 1) * k + s) * XYZZ_WORDS : nullptr,
            dst + (((size_t)st.dst + t) * k + s) * XYZZ_WORDS);
}

__global__ __launch_bounds__(64) void vkx_mul_kernel(const u32* __restrict__ points, const u32* __restrict__ scalars, size_t lanes, int cols,
                                                     u32* __restrict__ terms) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    u32 kw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) kw[j] = scalars[t * 8 + j];
    vkx_term(points + (t % cols) * G1_WORDS, kw, terms + t * XYZZ_WORDS);
}

// one block per suspect (the grid is exactly the suspects: no lane leaves before the barriers)
__global__ __launch_bounds__(64) void vkx_sum_kernel(const u32* __restrict__ terms, int cols, u32* __restrict__ neg_vkx) {
    __shared__ u32 part[64 * XYZZ_WORDS];
    const size_t i = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const u32* t = terms + i * cols * XYZZ_WORDS;
    G1XYZZ acc = xyzz_inf<Fq>();
    for (int c = lane; c < cols; c += 64) acc = xyzz_add(acc, xyzz_load(t + (size_t)c * XYZZ_WORDS));
    xyzz_store(part + lane * XYZZ_WORDS, acc);
    for (int half = 32; half >= 1; half >>= 1) {
        __syncthreads();
        if (lane < half) {
            acc = xyzz_add(acc, xyzz_load(part + (lane + half) * XYZZ_WORDS));
            xyzz_store(part + lane * XYZZ_WORDS, acc);
        }
    }
    if (lane == 0) vkx_finish(acc, neg_vkx + i * G1_WORDS);
}

// KEYED: key_g2 and f_ab are tables with one entry per key, and key_of[i] says which one suspect i is judged under
template <bool KEYED>
__global__ UG_ONE_WAVE void judge_kernel(FinalExpConsts kc, const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ neg_vkx,
                                         const u32* __restrict__ g, const u32* __restrict__ key_g2, const u32* __restrict__ f_ab,
                                         const u32* __restrict__ key_of, int n, int k, u32* __restrict__ verdict) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    if constexpr (KEYED) {
        const size_t q = key_of[i];
        key_g2 += q * (size_t)(1 + k) * G2_WORDS;
        f_ab += q * F12_WORDS;
    }
    verdict[i] = judge_proof(kc, a + i * G1_WORDS, b + i * G2_WORDS, neg_vkx + i * G1_WORDS, g + i * k * G1_WORDS, k, key_g2, f_ab) ? 1u : 0u;
}

// The ratio test (Backend::ratio): lane i says whether e(x_i, Q) = e(y_i, G2) for two zkey-format G1 records, which it converts
// itself; q2 = Q, then the generator of G2. Both levels of the test -- the block sums and the records -- go through this kernel.
__global__ UG_ONE_WAVE void ratio_judge_kernel(FinalExpConsts kc, const u32* __restrict__ x, const u32* __restrict__ y, const u32* __restrict__ q2,
                                               int n, u32* __restrict__ wrong) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    wrong[i] = ratio_holds(kc, x + i * 16, y + i * 16, q2) ? 0u : 1u;
}

__global__ UG_ONE_WAVE void final_exp_kernel(FinalExpConsts kc, const u32* __restrict__ f_in, u32* __restrict__ g_out, u32* __restrict__ is_one) {
    if (blockIdx.x || threadIdx.x) return;
    F12 f, g;
    f12_load(f, f_in);
    is_one[0] = final_exp_is_one(kc, f, g) ? 1u : 0u;
    f12_store(g_out, g);
}

// The packed proof records of include/verifier.h (plain 256-bit integers, 32 bytes a coordinate: pi_a | pi_b | the k other G1
// points), ONE RECORD PER LANE: a lane needs all of a point's coordinates for its curve equation, and the 8 (10) reductions of a
// record are nothing beside the Miller loop that follows, so the coalesced coordinate-per-lane mapping and its exchange through LDS
// were not worth having; a lane reads its record with 16-byte loads. Every coordinate is reduced mod q (from_normal takes any
// 256-bit value) into the canonical limb form, (0, 0) is infinity as in the JSON parsers, and the lane writes
//   a / b / g     the G1_WORDS / G2_WORDS arrays miller_batch_kernel reads, in record order (all zero = infinity),
//   bz            pi_b once more as a zkey record (Montgomery radix 2^256), what the subgroup ladder of check.hip reads; infinity
//                 for a record that failed here, so that the ladder passes over it,
//   status        UG_POINT_OK, or UG_POINT_OFF_CURVE when any of its points is off its curve.
// The EVM layout (FORMAT = RECORDS_EVM) differs in how a coordinate is loaded -- big-endian: the words in reverse order, each
// byte-reversed -- and in where the halves of an Fq2 coordinate lie (the imaginary part first); IngestConsts are pairing.hpp's.
template <int FORMAT> __device__ __forceinline__ F1 ingest_coord(const u32* p) {
    u32 w[8];
    load8(w, p);
    if constexpr (FORMAT == RECORDS_EVM) {
        u32 v[8];
        for (int j = 0; j < 8; j++) v[j] = __builtin_bswap32(w[7 - j]);
        return F1{canon(from_normal<FqParams>(v))};
    }
    return F1{canon(from_normal<FqParams>(w))};
}
template <int FORMAT> __device__ __forceinline__ bool ingest_g1(const u32* rec, const IngestConsts& c, u32* out) {
    const F1 x = ingest_coord<FORMAT>(rec), y = ingest_coord<FORMAT>(rec + 8);
    if (is0(x) && is0(y)) {
        for (int j = 0; j < G1_WORDS; j++) out[j] = 0;
        return true;
    }
    fq_store(out, x.v); fq_store(out + NL, y.v);
    return y * y == x * x * x + c.b1;
}

template <int FORMAT>
__global__ __launch_bounds__(64) void records_ingest_kernel(const u32* __restrict__ records, int n, int k, IngestConsts c, u32* __restrict__ a,
                                                            u32* __restrict__ b, u32* __restrict__ g, u32* __restrict__ bz,
                                                            uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    const u32* rec = records + i * (size_t)(48 + 16 * k);
    bool ok = ingest_g1<FORMAT>(rec, c, a + i * G1_WORDS);
    for (int s = 0; s < k; s++) ok = ingest_g1<FORMAT>(rec + 48 + 16 * s, c, g + (i * k + s) * G1_WORDS) && ok;
    constexpr int RE = FORMAT == RECORDS_EVM ? 8 : 0, IM = 8 - RE;  // where the real and the imaginary half of an Fq2 coordinate lie
    const F2 x{ingest_coord<FORMAT>(rec + 16 + RE), ingest_coord<FORMAT>(rec + 16 + IM)}, y{ingest_coord<FORMAT>(rec + 32 + RE), ingest_coord<FORMAT>(rec + 32 + IM)};
    const bool inf = is0(x) && is0(y);
    u32* bo = b + i * G2_WORDS;
    if (inf) { for (int j = 0; j < G2_WORDS; j++) bo[j] = 0; }
    else {
        fq_store(bo, x.a.v); fq_store(bo + NL, x.b.v); fq_store(bo + 2 * NL, y.a.v); fq_store(bo + 3 * NL, y.b.v);
        ok = (y * y == x * x * x + c.b2) && ok;
    }
    u32 z[32];
    if (inf || !ok) { for (int j = 0; j < 32; j++) z[j] = 0; }
    else { to_mont256(z, x.a.v); to_mont256(z + 8, x.b.v); to_mont256(z + 16, y.a.v); to_mont256(z + 24, y.b.v); }
    for (int j = 0; j < 4; j++) store8(bz + i * 32 + j * 8, z + j * 8);
    status[i] = ok ? (uint8_t)UG_POINT_OK : (uint8_t)UG_POINT_OFF_CURVE;
}

// Compressed records (include/verifier.h): a G1 point is x in 32 little-endian bytes, pi_b is x.c0 | x.c1, and the two top bits
// of a point's last byte say "infinity" (0x40) and "y is the larger root" (0x80); 24 + 8 k words a record: pi_a | pi_b | the k
// other G1 points. The mapping and the outputs are those of records_ingest_kernel. A point whose x^3 + b has no root is written
// as zeros and makes the record UG_POINT_OFF_CURVE; a point that has one is on its curve by construction (root^2 is compared).
// One copy of the Fq root serves pi_a and the k points (the loop is kept), pi_b has its own three inside f2_sqrt.
__device__ __forceinline__ bool decompress_g1(const u32* rec, const DecompressConsts& c, u32* out) {
    u32 w[8];
    load8(w, rec);
    const bool inf = (w[7] >> 30) & 1, larger = (w[7] >> 31) != 0;
    w[7] &= 0x3fffffffu;
    const F1 x{canon(from_normal<FqParams>(w))};
    F1 y = f1_zero();
    const bool ok = inf || g1_decompress(c, x, larger, y);
    if (inf || !ok) { for (int j = 0; j < G1_WORDS; j++) out[j] = 0; }
    else { fq_store(out, x.v); fq_store(out + NL, y.v); }
    return ok;
}

__global__ __launch_bounds__(64) void records_decompress_kernel(const u32* __restrict__ records, int n, int k, DecompressConsts c,
                                                                u32* __restrict__ a, u32* __restrict__ b, u32* __restrict__ g,
                                                                u32* __restrict__ bz, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    const u32* rec = records + i * (size_t)(24 + 8 * k);
    bool ok = true;
#pragma unroll 1
    for (int s = 0; s <= k; s++)                                    // s = 0: pi_a, s >= 1: the other G1 points
        ok = decompress_g1(s ? rec + 24 + 8 * (s - 1) : rec, c, s ? g + (i * k + (s - 1)) * G1_WORDS : a + i * G1_WORDS) && ok;
    u32 w0[8], w1[8];
    load8(w0, rec + 8);
    load8(w1, rec + 16);
    const bool inf = (w1[7] >> 30) & 1, larger = (w1[7] >> 31) != 0;
    w1[7] &= 0x3fffffffu;
    const F2 x{F1{canon(from_normal<FqParams>(w0))}, F1{canon(from_normal<FqParams>(w1))}};
    F2 y = f2_zero();
    const bool live = !inf && g2_decompress(c, x, larger, y);
    ok = ok && (inf || live);
    u32* bo = b + i * G2_WORDS;
    if (!live) { for (int j = 0; j < G2_WORDS; j++) bo[j] = 0; }
    else { fq_store(bo, x.a.v); fq_store(bo + NL, x.b.v); fq_store(bo + 2 * NL, y.a.v); fq_store(bo + 3 * NL, y.b.v); }
    u32 z[32];
    if (!live || !ok) { for (int j = 0; j < 32; j++) z[j] = 0; }
    else { to_mont256(z, x.a.v); to_mont256(z + 8, x.b.v); to_mont256(z + 16, y.a.v); to_mont256(z + 24, y.b.v); }
    for (int j = 0; j < 4; j++) store8(bz + i * 32 + j * 8, z + j * 8);
    status[i] = ok ? (uint8_t)UG_POINT_OK : (uint8_t)UG_POINT_OFF_CURVE;
}

// in: n x 16 words, plain c0 | c1 (any 256-bit values); out: the root that is not the larger one, plain and canonical (zeros when
// there is none); has_root: one byte each
__global__ __launch_bounds__(64) void fq2_sqrt_kernel(DecompressConsts c, const u32* __restrict__ in, int n, u32* __restrict__ out,
                                                      uint8_t* __restrict__ has_root) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    const F2 v{ingest_coord<RECORDS_PLAIN>(in + i * 16), ingest_coord<RECORDS_PLAIN>(in + i * 16 + 8)};
    F2 r;
    const bool ok = f2_sqrt(c, v, r);
    if (ok && f2_larger(c, r)) r = -r;
    u32 w[16];
    to_normal(w, r.a.v);
    to_normal(w + 8, r.b.v);
    store8(out + i * 16, w);
    store8(out + i * 16 + 8, w + 8);
    has_root[i] = ok ? 1 : 0;
}

// records were dropped: row t of dst = row index[t] of src (rows of `words` words), so that the Miller kernel sees a dense array
__global__ __launch_bounds__(256) void gather_rows_kernel(const u32* __restrict__ src, const u32* __restrict__ index, size_t m, int words,
                                                          u32* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * (size_t)words) return;
    const size_t row = t / (size_t)words, w = t - row * (size_t)words;
    dst[t] = src[(size_t)index[row] * (size_t)words + w];
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + 63) / 64); }

}  // namespace

// the kernels of a pass over arrays that are on the device already; both trees come back to the host
// plan: the pass's segments (null: one, the tree kernels; else the forest kernels, whose trees are the plan's forest); leaf_f / leaf_g:
// the leaves are given (host arrays) and no Miller loop runs. Returns the tree launches.
static int run_pass(const PairingConsts& kc, const u32* a, const u32* b, const u32* g, const u32* r, int n_, int k_, u32* f_tree, u32* g_tree,
                    double kernel_ms[3], const ForestPlan* plan = nullptr, const u32* leaf_f = nullptr, const u32* leaf_g = nullptr) {
    const size_t n = (size_t)n_, k = (size_t)k_, nodes = plan ? plan->nodes : tree_nodes(n);
    if (plan && (plan->size.empty() || plan->level_base.size() != plan->step.size() + 1 || plan->off.back()[0] + plan->size.back() != n))
        throw std::invalid_argument("run_pass: the segments do not cover the pass");
    if ((leaf_f || leaf_g) && !(plan && leaf_f && leaf_g)) throw std::invalid_argument("run_pass: given leaves need both arrays and a plan");
    DevBuf<u32> f(nodes * F12_WORDS), s(nodes * k * XYZZ_WORDS);
    Event t0(true), t1(true), t2(true), t3(true);
    int launches = 0;
    UG_HIP(hipEventRecord(t0.e, nullptr));
    if (leaf_f) {
        UG_HIP(hipMemcpy(f.get(), leaf_f, n * F12_WORDS * sizeof(u32), hipMemcpyHostToDevice));
        UG_HIP(hipMemcpy(s.get(), leaf_g, n * k * XYZZ_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    } else {
        hipLaunchKernelGGL(miller_batch_kernel, dim3(blocks(n)), dim3(64), 0, nullptr, kc, a, b, g, r, n_, k_, f.get(), s.get());
        UG_KERNEL_CHECK();
    }
    UG_HIP(hipEventRecord(t1.e, nullptr));
    if (plan) {
        // every step's table in one upload: start (segs + 1), src (segs), n_src (segs)
        std::vector<u32> table;
        std::vector<size_t> at;
        for (const ForestPlan::Step& st : plan->step) {
            if (st.src.empty() || st.start.size() != st.src.size() + 1 || st.n_src.size() != st.src.size()) throw std::invalid_argument("run_pass: bad forest step");
            at.push_back(table.size());
            table.insert(table.end(), st.start.begin(), st.start.end());
            table.insert(table.end(), st.src.begin(), st.src.end());
            table.insert(table.end(), st.n_src.begin(), st.n_src.end());
        }
        DevBuf<u32> dt(std::max<size_t>(table.size(), 1));
        if (!table.empty()) UG_HIP(hipMemcpy(dt.get(), table.data(), table.size() * sizeof(u32), hipMemcpyHostToDevice));
        auto step_of = [&](size_t l) {
            const u32 segs = (u32)plan->step[l].src.size();
            const u32* p = dt.get() + at[l];
            // (the last node a lane of this step may write is level_base[l + 1] + lanes - 1 < nodes, by the plan's construction)
            return ForestStep{p, p + segs + 1, p + 2 * segs + 1, segs, (u32)plan->level_base[l + 1]};
        };
        for (size_t l = 0; l < plan->step.size(); l++) {
            hipLaunchKernelGGL(f12_forest_kernel, dim3(blocks(plan->step[l].start.back())), dim3(64), 0, nullptr, kc, f.get(), step_of(l), f.get());
            UG_KERNEL_CHECK();
            launches++;
        }
        UG_HIP(hipEventRecord(t2.e, nullptr));
        for (size_t l = 0; l < plan->step.size(); l++) {
            hipLaunchKernelGGL(g1_forest_kernel, dim3(blocks(plan->step[l].start.back() * k)), dim3(64), 0, nullptr, s.get(), step_of(l), k_, s.get());
            UG_KERNEL_CHECK();
            launches++;
        }
    } else {
        size_t off = 0;
        for (size_t m = n; m > 1; m = (m + 1) / 2) {                // level of m nodes at `off` -> (m + 1) / 2 nodes behind it
            hipLaunchKernelGGL(f12_tree_kernel, dim3(blocks((m + 1) / 2)), dim3(64), 0, nullptr, kc, f.get() + off * F12_WORDS, (int)m, f.get() + (off + m) * F12_WORDS);
            UG_KERNEL_CHECK();
            off += m;
            launches++;
        }
        UG_HIP(hipEventRecord(t2.e, nullptr));
        off = 0;
        for (size_t m = n; m > 1; m = (m + 1) / 2) {
            hipLaunchKernelGGL(g1_tree_kernel, dim3(blocks(((m + 1) / 2) * k)), dim3(64), 0, nullptr, s.get() + off * k * XYZZ_WORDS, (int)m, k_, s.get() + (off + m) * k * XYZZ_WORDS);
            UG_KERNEL_CHECK();
            off += m;
            launches++;
        }
    }
    UG_HIP(hipEventRecord(t3.e, nullptr));
    UG_HIP(hipMemcpy(f_tree, f.get(), nodes * F12_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    UG_HIP(hipMemcpy(g_tree, s.get(), nodes * k * XYZZ_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    float ms[3] = {0, 0, 0};
    UG_HIP(hipEventElapsedTime(&ms[0], t0.e, t1.e));
    UG_HIP(hipEventElapsedTime(&ms[1], t1.e, t2.e));
    UG_HIP(hipEventElapsedTime(&ms[2], t2.e, t3.e));
    for (int i = 0; i < 3; i++) kernel_ms[i] = ms[i];
    return launches;
}

void pairing_batch_device(int device, const PairingConsts& kc, PairingBatch& pb) {
    if (pb.n <= 0 || pb.n > PAIRING_PASS || (pb.k != 1 && pb.k != 2)) throw std::invalid_argument("pairing_batch_device: bad shape");
    UG_HIP(hipSetDevice(device));
    const size_t n = (size_t)pb.n, k = (size_t)pb.k;
    if (pb.leaf_f || pb.leaf_g) {                                   // only the forest kernels, over given leaves
        pb.tree_launches = run_pass(kc, nullptr, nullptr, nullptr, nullptr, pb.n, pb.k, pb.f_tree, pb.g_tree, pb.kernel_ms, pb.plan, pb.leaf_f, pb.leaf_g);
        return;
    }
    DevBuf<u32> a(n * G1_WORDS), b(n * G2_WORDS), g(n * k * G1_WORDS), r(n * 4);
    UG_HIP(hipMemcpy(a.get(), pb.a, n * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(b.get(), pb.b, n * G2_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(g.get(), pb.g, n * k * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(r.get(), pb.r, n * 4 * sizeof(u32), hipMemcpyHostToDevice));
    pb.tree_launches = run_pass(kc, a.get(), b.get(), g.get(), r.get(), pb.n, pb.k, pb.f_tree, pb.g_tree, pb.kernel_ms, pb.plan);
}

// ---- the resident form: the pass's raw records cross PCIe once and its arrays never leave the device ---------------------
struct ResidentBatch::Impl {
    int device, n, k, format;
    DevBuf<u32> records, a, b, g, bz, status;
    Impl(int device_, int n_, int k_, int format_)
        : device(device_), n(n_), k(k_), format(format_), records((size_t)n_ * record_words(k_, format_)), a((size_t)n_ * G1_WORDS), b((size_t)n_ * G2_WORDS),
          g((size_t)n_ * k_ * G1_WORDS), bz((size_t)n_ * 32), status(((size_t)n_ + 3) / 4 * 2) {}      // status: n bytes from each check
};
ResidentBatch::ResidentBatch(int device, int n, int k, int format) {
    if (n <= 0 || n > PAIRING_PASS || (k != 1 && k != 2)) throw std::invalid_argument("ResidentBatch: bad shape");
    if (format != RECORDS_PLAIN && format != RECORDS_EVM && format != RECORDS_COMPRESSED) throw std::invalid_argument("ResidentBatch: unknown format");
    UG_HIP(hipSetDevice(device));
    impl = new Impl(device, n, k, format);
}
ResidentBatch::~ResidentBatch() { delete impl; }

void ResidentBatch::ingest(const void* records, unsigned char* status) {
    Impl& m = *impl;
    UG_HIP(hipSetDevice(m.device));
    static const DecompressConsts c = decompress_consts();         // the plain and EVM kernels take its IngestConsts part
    const IngestConsts& ci = c;
    const size_t n = (size_t)m.n, room = (n + 3) / 4 * 4;
    uint8_t* curve = reinterpret_cast<uint8_t*>(m.status.get());
    uint8_t* subgroup = curve + room;
    UG_HIP(hipMemcpy(m.records.get(), records, n * record_words(m.k, m.format) * sizeof(u32), hipMemcpyHostToDevice));
    if (m.format == RECORDS_COMPRESSED)
        hipLaunchKernelGGL(records_decompress_kernel, dim3(blocks(n)), dim3(64), 0, nullptr, m.records.get(), m.n, m.k, c, m.a.get(), m.b.get(), m.g.get(), m.bz.get(), curve);
    else if (m.format == RECORDS_EVM)
        hipLaunchKernelGGL(records_ingest_kernel<RECORDS_EVM>, dim3(blocks(n)), dim3(64), 0, nullptr, m.records.get(), m.n, m.k, ci, m.a.get(), m.b.get(), m.g.get(), m.bz.get(), curve);
    else
        hipLaunchKernelGGL(records_ingest_kernel<RECORDS_PLAIN>, dim3(blocks(n)), dim3(64), 0, nullptr, m.records.get(), m.n, m.k, ci, m.a.get(), m.b.get(), m.g.get(), m.bz.get(), curve);
    UG_KERNEL_CHECK();
    check_points_mask(true, m.bz.get(), n, 2, subgroup, nullptr);      // (a record that failed above is infinity here: it passes)
    std::vector<uint8_t> both(2 * room);
    UG_HIP(hipMemcpy(both.data(), curve, 2 * room, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) status[i] = both[i] ? both[i] : both[room + i];
}

void ResidentBatch::download(u32* a, u32* b, u32* g) {
    Impl& m = *impl;
    UG_HIP(hipSetDevice(m.device));
    const size_t n = (size_t)m.n;
    if (a) UG_HIP(hipMemcpy(a, m.a.get(), n * G1_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    if (b) UG_HIP(hipMemcpy(b, m.b.get(), n * G2_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    if (g) UG_HIP(hipMemcpy(g, m.g.get(), n * (size_t)m.k * G1_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
}

void ResidentBatch::run(const PairingConsts& kc, const u32* keep, int kept, const u32* r, u32* f_tree, u32* g_tree, double kernel_ms[3]) {
    Impl& m = *impl;
    if (kept <= 0 || kept > m.n || (!keep && kept != m.n)) throw std::invalid_argument("ResidentBatch: bad shape");
    UG_HIP(hipSetDevice(m.device));
    const size_t n = (size_t)kept, k = (size_t)m.k;
    DevBuf<u32> rd(n * 4);
    UG_HIP(hipMemcpy(rd.get(), r, n * 4 * sizeof(u32), hipMemcpyHostToDevice));
    if (!keep) { tree_launches = run_pass(kc, m.a.get(), m.b.get(), m.g.get(), rd.get(), kept, m.k, f_tree, g_tree, kernel_ms, plan); return; }
    for (size_t i = 0; i < n; i++)                                  // the gather reads row keep[i]: inside the pass, ascending
        if (keep[i] >= (u32)m.n || (i && keep[i] <= keep[i - 1])) throw std::invalid_argument("ResidentBatch: bad index list");
    DevBuf<u32> index(n), a(n * G1_WORDS), b(n * G2_WORDS), g(n * k * G1_WORDS);
    UG_HIP(hipMemcpy(index.get(), keep, n * sizeof(u32), hipMemcpyHostToDevice));
    auto gather = [&](const u32* src, int words, u32* dst) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n * (size_t)words + 255) / 256)), dim3(256), 0, nullptr, src, index.get(), n, words, dst);
        UG_KERNEL_CHECK();
    };
    gather(m.a.get(), G1_WORDS, a.get());
    gather(m.b.get(), G2_WORDS, b.get());
    gather(m.g.get(), (int)k * G1_WORDS, g.get());
    tree_launches = run_pass(kc, a.get(), b.get(), g.get(), rd.get(), kept, m.k, f_tree, g_tree, kernel_ms, plan);
}

// the vkx step keeps at most this many XYZZ products on the device at a time (144 bytes each)
constexpr size_t VKX_CHUNK_TERMS = (size_t)1 << 20;

void pairing_judge_device(int device, const FinalExpConsts& kc, PairingJudge& pj) {
    const bool keyed = pj.n_keys > 1;
    if (pj.n <= 0 || pj.n > PAIRING_PASS || (pj.k != 1 && pj.k != 2) || pj.n_keys < 1 || (!keyed && pj.cols <= 0) || (keyed && (!pj.key_first || !pj.key_cols)))
        throw std::invalid_argument("pairing_judge_device: bad shape");
    UG_HIP(hipSetDevice(device));
    const size_t n = (size_t)pj.n, k = (size_t)pj.k, n_keys = (size_t)pj.n_keys;
    // per key: its suspects first[q] .. first[q + 1], its columns, and where its points begin; one key: all suspects, pj.cols
    std::vector<size_t> first(n_keys + 1, 0), kcols(n_keys, 0), point_at(n_keys + 1, 0);
    std::vector<u32> key_of(n, 0);
    size_t max_cols = 0;
    for (size_t q = 0; q < n_keys; q++) {
        kcols[q] = keyed ? (size_t)std::max(pj.key_cols[q], 0) : (size_t)pj.cols;
        first[q + 1] = keyed ? (size_t)std::max(pj.key_first[q + 1], 0) : n;
        if (!kcols[q] || first[q + 1] < first[q] || first[q + 1] > n) throw std::invalid_argument("pairing_judge_device: bad key table");
        point_at[q + 1] = point_at[q] + kcols[q];
        max_cols = std::max(max_cols, kcols[q]);
        for (size_t i = first[q]; i < first[q + 1]; i++) key_of[i] = (u32)q;
    }
    if (first[0] != 0 || first[n_keys] != n) throw std::invalid_argument("pairing_judge_device: bad key table");
    const size_t all_cols = point_at[n_keys];
    const size_t chunk = std::min(n, std::max<size_t>(1, VKX_CHUNK_TERMS / max_cols));       // suspects per launch of the vkx step
    DevBuf<u32> a(n * G1_WORDS), b(n * G2_WORDS), g(n * k * G1_WORDS), points(all_cols * G1_WORDS), key(n_keys * (1 + k) * G2_WORDS), fab(n_keys * F12_WORDS);
    DevBuf<u32> scalars(chunk * max_cols * 8), terms(chunk * max_cols * XYZZ_WORDS), nvkx(n * G1_WORDS), verdict(n), dkey_of(n);
    Event t0(true), t1(true), t2(true);
    UG_HIP(hipMemcpy(a.get(), pj.a, n * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(b.get(), pj.b, n * G2_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(g.get(), pj.g, n * k * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(points.get(), pj.points, all_cols * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(key.get(), pj.key_g2, n_keys * (1 + k) * G2_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(fab.get(), pj.f_alpha_beta, n_keys * F12_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    if (keyed) UG_HIP(hipMemcpy(dkey_of.get(), key_of.data(), n * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipEventRecord(t0.e, nullptr));
    const u32* sc = pj.scalars;                                     // the next key's scalars
    for (size_t q = 0; q < n_keys; q++) {                           // the vkx step, once per key
        const size_t cols = kcols[q];
        for (size_t at = first[q]; at < first[q + 1]; at += chunk) {
            const size_t m = std::min(chunk, first[q + 1] - at);
            UG_HIP(hipMemcpy(scalars.get(), sc, m * cols * 8 * sizeof(u32), hipMemcpyHostToDevice));
            sc += m * cols * 8;
            hipLaunchKernelGGL(vkx_mul_kernel, dim3(blocks(m * cols)), dim3(64), 0, nullptr, points.get() + point_at[q] * G1_WORDS, scalars.get(), m * cols, (int)cols, terms.get());
            UG_KERNEL_CHECK();
            hipLaunchKernelGGL(vkx_sum_kernel, dim3((unsigned)m), dim3(64), 0, nullptr, terms.get(), (int)cols, nvkx.get() + at * G1_WORDS);
            UG_KERNEL_CHECK();
        }
    }
    UG_HIP(hipEventRecord(t1.e, nullptr));
    if (keyed)
        hipLaunchKernelGGL(judge_kernel<true>, dim3(blocks(n)), dim3(64), 0, nullptr, kc, a.get(), b.get(), nvkx.get(), g.get(), key.get(), fab.get(), dkey_of.get(), pj.n, pj.k, verdict.get());
    else
        hipLaunchKernelGGL(judge_kernel<false>, dim3(blocks(n)), dim3(64), 0, nullptr, kc, a.get(), b.get(), nvkx.get(), g.get(), key.get(), fab.get(), nullptr, pj.n, pj.k, verdict.get());
    UG_KERNEL_CHECK();
    UG_HIP(hipEventRecord(t2.e, nullptr));
    UG_HIP(hipMemcpy(pj.verdict, verdict.get(), n * sizeof(u32), hipMemcpyDeviceToHost));
    float ms[2] = {0, 0};
    UG_HIP(hipEventElapsedTime(&ms[0], t0.e, t1.e));
    UG_HIP(hipEventElapsedTime(&ms[1], t1.e, t2.e));
    for (int i = 0; i < 2; i++) pj.kernel_ms[i] = ms[i];
}

// The pairings of the ratio test (setup_host.hpp: Backend::ratio; pairing.hpp: ratio_holds), one lane per pair: wrong[i] = 1 unless
// e(x_i, Q) = e(y_i, G2). x, y: n zkey-format G1 records on the host; q2: Q, then the generator of G2, G2_WORDS each. On the caller's
// stream and current device, which it waits for; n is cut into launches of PAIRING_PASS lanes. kernel_ms (may be null): the kernel's time.
void ratio_judge_device(hipStream_t stream, const FinalExpConsts& kc, const uint8_t* x, const uint8_t* y, u64 n, const u32* q2, uint8_t* wrong,
                        double* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    if (!n) return;
    const size_t pass = std::min<u64>(n, PAIRING_PASS);
    DevBuf<u32> dx(pass * 16), dy(pass * 16), dq(2 * G2_WORDS), dw(pass);
    std::vector<u32> w(pass);
    Event t0(true), t1(true);
    UG_HIP(hipMemcpyAsync(dq.get(), q2, 2 * G2_WORDS * sizeof(u32), hipMemcpyHostToDevice, stream));
    for (u64 first = 0; first < n; first += pass) {
        const size_t m = (size_t)std::min<u64>(pass, n - first);
        UG_HIP(hipMemcpyAsync(dx.get(), x + first * 64, m * 64, hipMemcpyHostToDevice, stream));
        UG_HIP(hipMemcpyAsync(dy.get(), y + first * 64, m * 64, hipMemcpyHostToDevice, stream));
        UG_HIP(hipEventRecord(t0.e, stream));
        hipLaunchKernelGGL(ratio_judge_kernel, dim3(blocks(m)), dim3(64), 0, stream, kc, dx.get(), dy.get(), dq.get(), (int)m, dw.get());
        UG_KERNEL_CHECK();
        UG_HIP(hipEventRecord(t1.e, stream));
        UG_HIP(hipMemcpyAsync(w.data(), dw.get(), m * sizeof(u32), hipMemcpyDeviceToHost, stream));
        UG_HIP(hipStreamSynchronize(stream));
        float ms = 0;
        UG_HIP(hipEventElapsedTime(&ms, t0.e, t1.e));
        if (kernel_ms) *kernel_ms += ms;
        for (size_t i = 0; i < m; i++) wrong[first + i] = w[i] ? 1 : 0;
    }
}

void fq2_sqrt_device(int device, const DecompressConsts& c, int count, const u32* in, u32* out, unsigned char* has_root) {
    if (count <= 0) return;
    UG_HIP(hipSetDevice(device));
    const size_t n = (size_t)count;
    DevBuf<u32> din(n * 16), dout(n * 16), flag((n + 3) / 4);
    UG_HIP(hipMemcpy(din.get(), in, n * 16 * sizeof(u32), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(fq2_sqrt_kernel, dim3(blocks(n)), dim3(64), 0, nullptr, c, din.get(), count, dout.get(), reinterpret_cast<uint8_t*>(flag.get()));
    UG_KERNEL_CHECK();
    UG_HIP(hipMemcpy(out, dout.get(), n * 16 * sizeof(u32), hipMemcpyDeviceToHost));
    UG_HIP(hipMemcpy(has_root, flag.get(), n, hipMemcpyDeviceToHost));
}

void final_exp_device(int device, const FinalExpConsts& kc, const u32* f, u32* g, int* is_one) {
    UG_HIP(hipSetDevice(device));
    DevBuf<u32> in(F12_WORDS), out(F12_WORDS), flag(1);
    UG_HIP(hipMemcpy(in.get(), f, F12_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(final_exp_kernel, dim3(1), dim3(64), 0, nullptr, kc, in.get(), out.get(), flag.get());
    UG_KERNEL_CHECK();
    u32 one = 0;
    UG_HIP(hipMemcpy(g, out.get(), F12_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    UG_HIP(hipMemcpy(&one, flag.get(), sizeof(u32), hipMemcpyDeviceToHost));
    *is_one = (int)one;
}

}  // namespace ug
