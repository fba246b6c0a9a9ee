// setup_points.hip -- the two heavy steps of the phase-2 setup from a .ptau on the device (setup_host.hpp: Backend::combine and
// Backend::scale; include/ultragroth_hip.h: ug_setup_ptau_run, ug_points_combine, ug_points_scale). A real setup has no scalar
// per wire to multiply the generator by: it combines POINTS per wire, a variable-base problem.
//
//   term_products_kernel   one lane per NON-UNIT term, in class order (the host sorts the terms by the bit length of their
//                          coefficient): |coef| * (+-base) by double-and-add over exactly that many bits, stored as XYZZ. The
//                          lanes of a wave run the same number of steps, or one more.
//   piece_points_kernel    a column of more than SPLIT_THRESHOLD terms: one workgroup per piece of SPLIT_PIECE terms, the lanes'
//                          partial sums added in LDS (column_pieces_kernel of setup.hip, on points)
//   column_points_kernel   one lane per column: unit terms are a mixed addition of the gathered base (negated for r - 1), the
//                          others add their product; long columns add their pieces' sums; KPL results share one inversion and
//                          leave as canonical zkey records
//   scale_kernel           one scalar times many G1 points: the scalar's width-4 non-adjacent form comes from the host in the
//                          kernel argument, so every lane of the launch takes the same branch at every step
//   ratio_block_sums_kernel  the block level of the ratio test (Backend::ratio): one workgroup per block of
//                          256 pairs of records, a lane walks its 128-bit weight once for both points, the sums leave as records
// A coefficient above r / 2 is the negated point times r - coef, so 1 and r - 1 cost one addition and r - small costs as small.
// Plain C++ and vector stores only. DESIGN.md section 5.9 has the registers and what was measured.
#include "setup_dev.hpp"
#include "stream_timer.hpp"
#include "setup_host.hpp"
#include "internal.hpp"

#include <algorithm>

namespace ug {
namespace {

using namespace sdev;
using namespace ughost::setup;

struct P1 : S1 { static constexpr int PIECE_BLOCK = 256; };      // 36 limbs of an XYZZ point x 256 lanes: 36 KiB of LDS
struct P2 : S2 { static constexpr int PIECE_BLOCK = 64; };       // 72 limbs x 64 lanes: 18 KiB

// an XYZZ point in HBM: four packed coordinates, canonical (a packed value must be below 2^256; X may reach 7 q)
template <class Cfg> __device__ __forceinline__ void ld_xyzz(const u32* p, XYZZ<typename Cfg::F>& r) {
    Cfg::load(p, r.x, r.y);
    Cfg::load(p + Cfg::AFF_WORDS, r.zz, r.zzz);
}
template <class Cfg> __device__ __forceinline__ void st_xyzz(u32* p, const XYZZ<typename Cfg::F>& r) {
    Cfg::store_packed(p, canon(r.x), canon(r.y));
    Cfg::store_packed(p + Cfg::AFF_WORDS, canon(r.zz), canon(r.zzz));
}

// ---- per-term products ----
// slot_coef: 8 words per slot, |coef| plain (2 <= |coef| <= (r - 1) / 2 < 2^253), bit 255 set when the base is negated.
// The bit walk itself is setup_dev.hpp's walk_product, which the butterflies of ptau_prepare.hip share.
template <class Cfg>
__global__ __launch_bounds__(Cfg::BLOCK) void term_products_kernel(const u32* __restrict__ pts, const u32* __restrict__ slot_index,
                                                                   const u32* __restrict__ slot_coef, u32 n, u32* __restrict__ prod) {
    typedef typename Cfg::F F;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    u32 s[8];
    load8(s, slot_coef + (size_t)t * 8);
    const bool negate = (s[7] >> 31) != 0;
    s[7] &= 0x7fffffffu;
    F x, y;
    Cfg::load(pts + (size_t)slot_index[t] * Cfg::AFF_WORDS, x, y);
    u32* o = prod + (size_t)t * 2 * Cfg::AFF_WORDS;
    if (affine_is_inf(x, y)) { zero_record<2 * Cfg::AFF_WORDS>(o); return; }
    if (negate) y = neg<1>(y);                   // q - y: y is canonical
    const XYZZ<F> acc = walk_product(s, x, y);
    st_xyzz<Cfg>(o, acc);
}

// ---- per-column sums ----
// code[t] of term t: 0 nothing (a zero coefficient), 1 + base, 2 - base, 3 + slot: the product in that slot
struct ColArgs {
    const u32 *col_ptr, *index, *code, *pts, *prod, *partial;
    const Piece* pieces;
    u32 n_cols, n_pieces;
};
template <class Cfg>
__device__ __forceinline__ void add_term(XYZZ<typename Cfg::F>& acc, const ColArgs& a, u64 t) {
    typedef typename Cfg::F F;
    const u32 code = a.code[t];
    if (code == 0) return;
    if (code < 3) {
        F x, y;
        Cfg::load(a.pts + (size_t)a.index[t] * Cfg::AFF_WORDS, x, y);
        if (affine_is_inf(x, y)) return;
        if (code == 2) y = neg<1>(y);
        acc = xyzz_madd(acc, x, y);
    } else {
        XYZZ<F> q;
        ld_xyzz<Cfg>(a.prod + (size_t)(code - 3) * 2 * Cfg::AFF_WORDS, q);
        acc = xyzz_add(acc, q);
    }
}

// limbs of a coordinate <-> LDS, lane t's column of sh
template <int B> __device__ __forceinline__ void sh_put(u32 (*sh)[B], int row, u32 t, const Fq& v) {
#pragma unroll
    for (int i = 0; i < NL; i++) sh[row + i][t] = v.l[i];
}
template <int B> __device__ __forceinline__ void sh_put(u32 (*sh)[B], int row, u32 t, const Fq2& v) {
    sh_put<B>(sh, row, t, v.a); sh_put<B>(sh, row + NL, t, v.b);
}
template <int B> __device__ __forceinline__ void sh_get(u32 (*sh)[B], int row, u32 t, Fq& v) {
#pragma unroll
    for (int i = 0; i < NL; i++) v.l[i] = sh[row + i][t];
}
template <int B> __device__ __forceinline__ void sh_get(u32 (*sh)[B], int row, u32 t, Fq2& v) {
    sh_get<B>(sh, row, t, v.a); sh_get<B>(sh, row + NL, t, v.b);
}

// One workgroup per piece: lane t takes the terms first + t, + B, ...; the B partial sums are added in LDS (the limbs as they
// are: the lazily reduced ranges of ec.hpp survive the round trip). partial[piece]: XYZZ, packed.
template <class Cfg>
__global__ __launch_bounds__(Cfg::PIECE_BLOCK) void piece_points_kernel(ColArgs a, u32* __restrict__ partial) {
    typedef typename Cfg::F F;
    constexpr int B = Cfg::PIECE_BLOCK, FW = sizeof(F) / sizeof(u32);
    __shared__ u32 sh[4 * FW][B];
    const u32 t = threadIdx.x;
    if (blockIdx.x >= a.n_pieces) return;
    const Piece pc = a.pieces[blockIdx.x];
    XYZZ<F> acc = xyzz_inf<F>();
#pragma unroll 1
    for (u64 p = (u64)pc.first + t; p < pc.end; p += B) add_term<Cfg>(acc, a, p);
#pragma unroll 1
    for (u32 off = B / 2; off > 0; off >>= 1) {
        if (t < 2 * off) { sh_put<B>(sh, 0, t, acc.x); sh_put<B>(sh, FW, t, acc.y); sh_put<B>(sh, 2 * FW, t, acc.zz); sh_put<B>(sh, 3 * FW, t, acc.zzz); }
        __syncthreads();
        if (t < off) {
            XYZZ<F> o;
            sh_get<B>(sh, 0, t + off, o.x); sh_get<B>(sh, FW, t + off, o.y); sh_get<B>(sh, 2 * FW, t + off, o.zz); sh_get<B>(sh, 3 * FW, t + off, o.zzz);
            acc = xyzz_add(acc, o);
        }
        __syncthreads();
    }
    if (t == 0) st_xyzz<Cfg>(partial + (size_t)blockIdx.x * 2 * Cfg::AFF_WORDS, acc);
}

template <class Cfg>
__device__ __forceinline__ XYZZ<typename Cfg::F> column_point(const ColArgs& a, u32 c) {
    typedef typename Cfg::F F;
    const u32 lo = a.col_ptr[c], hi = a.col_ptr[c + 1];
    XYZZ<F> acc = xyzz_inf<F>();
    if (hi - lo <= SPLIT_THRESHOLD) {
#pragma unroll 1
        for (u32 t = lo; t < hi; t++) add_term<Cfg>(acc, a, t);
    } else {
        u32 l = 0, r = a.n_pieces;
        while (l < r) {                          // the first piece of column c (the pieces are column ascending)
            const u32 mid = l + (r - l) / 2;
            if (a.pieces[mid].wire < c) l = mid + 1; else r = mid;
        }
#pragma unroll 1
        for (u32 p = l; p < a.n_pieces && a.pieces[p].wire == c; p++) {
            XYZZ<F> q;
            ld_xyzz<Cfg>(a.partial + (size_t)p * 2 * Cfg::AFF_WORDS, q);
            acc = xyzz_add(acc, q);
        }
    }
    return acc;
}
// A lane takes KPL columns one after the other and converts the KPL sums with one shared inversion (gen_mul_kernel's ending).
template <class Cfg>
__global__ __launch_bounds__(Cfg::BLOCK) void column_points_kernel(ColArgs a, u32* __restrict__ out) {
    typedef typename Cfg::F F;
    constexpr int K = Cfg::KPL;
    const u64 n = a.n_cols;
    const u64 t0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * K;
    if (t0 >= n) return;
    XYZZ<F> res[K];
    F pre[K];
    F run = field_one((F*)0);
    // (always_inline: a lambda this large is otherwise left a function, and its captures -- res, run -- then live in scratch)
    Static<0, K>::up([&](auto k) __attribute__((always_inline)) {
        res[k] = t0 + k < n ? column_point<Cfg>(a, (u32)(t0 + k)) : xyzz_inf<F>();
        pre[k] = run;
        if (!is_inf(res[k])) run = mulk<8>(run, res[k].zzz);
    });
    F irun = inv(run);
    Static<0, K>::down([&](auto k) {
        if (t0 + k >= n) return;
        u32* o = out + (t0 + k) * Cfg::AFF_WORDS;
        if (is_inf(res[k])) { zero_record<Cfg::AFF_WORDS>(o); return; }
        const F izzz = mulk<8>(irun, pre[k]);
        irun = mulk<8>(irun, res[k].zzz);
        const F iz = mulk<8>(izzz, res[k].zz);
        const F izz = sqrk<8>(iz);
        Cfg::store_mont(o, mulk<8>(res[k].x, izz), mulk<8>(res[k].y, izzz));
    });
}

// ---- one scalar times many points ----
// digit[i] of the scalar's width-4 non-adjacent form: 0 or odd, |digit| <= 7, at most one non-zero digit in any four. The
// odd multiples P, 3P, 5P, 7P of a lane's point stay in registers as XYZZ; the digits are read from the kernel argument (scalar
// loads), so the whole launch takes the same branch at every step. xyzz_add handles every exceptional case, and a point of
// order r meets none before the last step.
struct WnafArgs { int8_t digit[256]; int top; };
// the walk both scale kernels share: digits top .. 0 of one scalar (top >= 0) over the affine point (x, y), which is not infinity;
// the result leaves as a canonical zkey record
__device__ __forceinline__ void scale_walk(const int8_t* digit, int top, const Fq& x, const Fq& y, u32* o) {
    const XYZZ<Fq> d2 = xyzz_dbl_affine(x, y);
    const XYZZ<Fq> t3 = xyzz_madd(d2, x, y), t5 = xyzz_add(t3, d2), t7 = xyzz_add(t5, d2);
    XYZZ<Fq> acc = xyzz_inf<Fq>();
#pragma unroll 1
    for (int b = top; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        const int d = digit[b];
        if (d == 0) continue;
        const int m = d < 0 ? -d : d;
        if (m == 1) {
            acc = xyzz_madd(acc, x, d < 0 ? neg<1>(y) : y);
        } else {
            XYZZ<Fq> q = m == 3 ? t3 : m == 5 ? t5 : t7;
            if (d < 0) q = xyzz_neg(q);
            acc = xyzz_add(acc, q);
        }
    }
    if (is_inf(acc)) { zero_record<16>(o); return; }
    Fq ax, ay;
    xyzz_to_affine(ax, ay, acc);
    S1::store_mont(o, ax, ay);
}
__global__ __launch_bounds__(128) void scale_kernel(const u32* __restrict__ pts, u64 n, WnafArgs a, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fq x, y;
    S1::load(pts + i * 16, x, y);
    u32* o = out + i * 16;
    if (a.top < 0 || affine_is_inf(x, y)) { zero_record<16>(o); return; }
    scale_walk(a.digit, a.top, x, y, o);
}

// ---- the delta step of an UltraGroth key: up to three segments (C1, C2, H), each with a scalar of its own ----
// A segment starts at a workgroup boundary (first_block) and its digit string is chosen by blockIdx alone, so a whole workgroup
// -- every wave of the launch, in fact, within a segment -- takes the same branch at every step, as in scale_kernel. A lane
// gathers its source record through the segment's index list (null: record i). top = -1: the scalar 0, all-zero records;
// top = -2: the scalar 1, the gathered record as it is, no walk.
constexpr int SEG_BLOCK = 128;
struct SegArgs {
    const u32* src;                              // the segment's source records, device form
    const u32* index;                            // count indexes into src, or null
    u32* out;
    u32 count, first_block;
    int top;
};
struct SegmentsArgs {
    SegArgs seg[MAX_SCALE_SEGS];
    int8_t digit[MAX_SCALE_SEGS][256];
    int n;
};
__global__ __launch_bounds__(SEG_BLOCK) void scale_segments_kernel(SegmentsArgs a) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < MAX_SCALE_SEGS; k++)
        if (k < a.n && blockIdx.x >= a.seg[k].first_block) s = k;
    const SegArgs& g = a.seg[s];
    const u32 i = (blockIdx.x - g.first_block) * SEG_BLOCK + threadIdx.x;
    if (i >= g.count) return;
    u32* o = g.out + (size_t)i * 16;
    if (g.top == -1) { zero_record<16>(o); return; }
    const size_t from = g.index ? g.index[i] : i;
    Fq x, y;
    S1::load(g.src + from * 16, x, y);
    if (affine_is_inf(x, y)) { zero_record<16>(o); return; }
    if (g.top == -2) { S1::store_mont(o, x, y); return; }
    scale_walk(a.digit[s], g.top, x, y, o);
}

// ---- the block sums of the ratio test (Backend::ratio): sum w_i X_i and sum w_i Y_i over each block of 256 records ----
// One workgroup per block, one record per lane. The lane walks the 128 bits of its weight once for both points (doubling an
// accumulator that is still infinity costs nothing, so the leading zero bits are free); a point at infinity stays out. The 256
// partial sums of each of the two sets are then added by a tree in LDS, the two sets one after the other through the same 36 KiB,
// and lane 0 converts both sums with one shared inversion. A sum may be infinity: the all-zero record.
constexpr int RATIO_LANES = 256;
static_assert(RATIO_LANES == (int)RATIO_BLOCK, "one lane per record of a block");
__device__ __forceinline__ void ratio_emit(u32* o, const XYZZ<Fq>& p, const Fq& izzz) {
    if (is_inf(p)) { zero_record<16>(o); return; }
    const Fq iz = mulk<8>(izzz, p.zz);
    const Fq izz = sqrk<8>(iz);
    S1::store_mont(o, mulk<8>(p.x, izz), mulk<8>(p.y, izzz));
}
__global__ __launch_bounds__(RATIO_LANES) void ratio_block_sums_kernel(const u32* __restrict__ xs, const u32* __restrict__ ys,
                                                                       const u32* __restrict__ weights, u32 n, u32* __restrict__ sums) {
    constexpr int B = RATIO_LANES, FW = NL;
    __shared__ u32 sh[4 * FW][B];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * B + t;
    XYZZ<Fq> ax = xyzz_inf<Fq>(), ay = xyzz_inf<Fq>();
    if (i < n) {                                 // (no lane leaves before the barriers below)
        Fq x1, y1, x2, y2;
        S1::load(xs + i * 16, x1, y1);
        S1::load(ys + i * 16, x2, y2);
        const bool live1 = !affine_is_inf(x1, y1), live2 = !affine_is_inf(x2, y2);
        const uint4 wv = reinterpret_cast<const uint4*>(weights)[i];
        u32 s0 = wv.x, s1 = wv.y, s2 = wv.z, s3 = wv.w;
#pragma unroll 1
        for (int b = 0; b < 128; b++) {
            ax = xyzz_dbl(ax);
            ay = xyzz_dbl(ay);
            const bool bit = (s3 >> 31) != 0;
            s3 = (s3 << 1) | (s2 >> 31); s2 = (s2 << 1) | (s1 >> 31); s1 = (s1 << 1) | (s0 >> 31); s0 <<= 1;
            if (bit) {
                if (live1) ax = xyzz_madd(ax, x1, y1);
                if (live2) ay = xyzz_madd(ay, x2, y2);
            }
        }
    }
    XYZZ<Fq> sx = ax, sy = ay;
#pragma unroll 1
    for (int set = 0; set < 2; set++) {
        XYZZ<Fq> acc = set ? ay : ax;
#pragma unroll 1
        for (u32 off = B / 2; off > 0; off >>= 1) {
            if (t < 2 * off) { sh_put<B>(sh, 0, t, acc.x); sh_put<B>(sh, FW, t, acc.y); sh_put<B>(sh, 2 * FW, t, acc.zz); sh_put<B>(sh, 3 * FW, t, acc.zzz); }
            __syncthreads();
            if (t < off) {
                XYZZ<Fq> o;
                sh_get<B>(sh, 0, t + off, o.x); sh_get<B>(sh, FW, t + off, o.y); sh_get<B>(sh, 2 * FW, t + off, o.zz); sh_get<B>(sh, 3 * FW, t + off, o.zzz);
                acc = xyzz_add(acc, o);
            }
            __syncthreads();
        }
        if (set) sy = acc; else sx = acc;
    }
    if (t != 0) return;
    const Fq one = field_one((Fq*)0);
    const Fq zx = is_inf(sx) ? one : sx.zzz, zy = is_inf(sy) ? one : sy.zzz;
    const Fq irun = inv(mulk<8>(zx, zy));
    u32* o = sums + (size_t)blockIdx.x * 32;
    ratio_emit(o, sx, mulk<8>(irun, zy));
    ratio_emit(o + 16, sy, mulk<8>(irun, zx));
}

// ---- host side ----
// The terms of a combination by class. code: one word per term (see ColArgs); the non-unit terms get a slot each, slots in the
// order of their coefficient's bit length, so a wave of term_products_kernel holds one length or two neighbouring ones.
struct Classes {
    std::vector<u32> code, slotIndex, slotCoef;
    u32 slots = 0;
};
void classify(u64 terms, const u32* index, const uint8_t* coefs, Classes& c) {
    constexpr u64 G = 1 << 15;
    const u64 chunks = (terms + G - 1) / G;
    std::vector<uint8_t> bits(terms);
    std::vector<u32> hist(chunks * 256, 0);
    parallelFor(terms, G, [&](u64 lo, u64 hi) {
        u32* h = &hist[(size_t)(lo / G) * 256];
        for (u64 t = lo; t < hi; t++) {
            u32 mag[8];
            coefMagnitude(coefs + t * 32, mag);
            const int b = bitLength(mag);
            bits[t] = (uint8_t)b;
            if (b >= 2) h[b]++;
        }
    });
    u32 run = 0;
    for (int b = 2; b < 256; b++)
        for (u64 k = 0; k < chunks; k++) {
            const u32 n = hist[(size_t)k * 256 + b];
            hist[(size_t)k * 256 + b] = run;
            run += n;
        }
    c.slots = run;
    c.code.resize(terms);
    c.slotIndex.resize(run);
    c.slotCoef.resize((size_t)run * 8);
    parallelFor(terms, G, [&](u64 lo, u64 hi) {
        u32* h = &hist[(size_t)(lo / G) * 256];
        for (u64 t = lo; t < hi; t++) {
            u32 mag[8];
            const bool negate = coefMagnitude(coefs + t * 32, mag);
            const int b = bits[t];
            if (b < 2) { c.code[t] = b == 0 ? 0u : negate ? 2u : 1u; continue; }
            const u32 slot = h[b]++;
            c.code[t] = slot + 3;
            c.slotIndex[slot] = index[t];
            if (negate) mag[7] |= 0x80000000u;
            memcpy(&c.slotCoef[(size_t)slot * 8], mag, 32);
        }
    });
}

template <class T> void upload(DevBuf<T>& d, const T* src, u64 n, hipStream_t stream) {
    d.alloc(n);
    if (n) UG_HIP(hipMemcpyAsync(d.get(), src, n * sizeof(T), hipMemcpyHostToDevice, stream));
}

template <class Cfg>
void combine_on_device(hipStream_t stream, StreamTimer& timer, u64 nCols, const u32* colPtr, const u32* index, const uint8_t* coefs,
                       const PointSegs& pts, uint8_t* out, double* ms) {
    constexpr u64 REC = Cfg::AFF_WORDS * 4;
    const u64 terms = colPtr[nCols];
    if (nCols > 0xffffffffull || terms > 0xfffffff0ull || pts.total() > 0xffffffffull)
        throw SetupError("sizes that cannot be represented: a combination of more than 2^32 - 16 columns, terms or points");
    Classes cls;
    classify(terms, index, coefs, cls);
    std::vector<Piece> pieces;
    columnPieces(colPtr, nCols, 0, pieces);

    DevBuf<u32> dColPtr, dIndex, dCode, dSlotIndex, dSlotCoef;
    DevBuf<Piece> dPieces;
    upload(dColPtr, colPtr, nCols + 1, stream);
    upload(dIndex, index, terms, stream);
    upload(dCode, cls.code.data(), terms, stream);
    upload(dSlotIndex, cls.slotIndex.data(), (u64)cls.slots, stream);
    upload(dSlotCoef, cls.slotCoef.data(), (u64)cls.slots * 8, stream);
    upload(dPieces, pieces.data(), (u64)pieces.size(), stream);
    DevBuf<u32> dPts(std::max<u64>(pts.total(), 1) * Cfg::AFF_WORDS);
    for (int s = 0; s < pts.n; s++)
        if (pts.count) UG_HIP(hipMemcpyAsync(dPts.get() + (u64)s * pts.count * Cfg::AFF_WORDS, pts.base[s], pts.count * REC, hipMemcpyHostToDevice, stream));
    if (std::is_same<typename Cfg::F, Fq2>::value) convert_points_g2(dPts.get(), pts.total(), stream);
    else convert_points_g1(dPts.get(), pts.total(), stream);
    DevBuf<u32> dProd((u64)cls.slots * 2 * Cfg::AFF_WORDS), dPartial((u64)pieces.size() * 2 * Cfg::AFF_WORDS), dOut(nCols * Cfg::AFF_WORDS);

    ColArgs a;
    a.col_ptr = dColPtr.get(); a.index = dIndex.get(); a.code = dCode.get(); a.pts = dPts.get(); a.prod = dProd.get(); a.partial = dPartial.get();
    a.pieces = dPieces.get(); a.n_cols = (u32)nCols; a.n_pieces = (u32)pieces.size();
    TimeSink products, sums;
    {
        StreamTimer::Scope sc = timer.time(stream, &products);
        if (cls.slots) {
            hipLaunchKernelGGL(term_products_kernel<Cfg>, dim3(grid_for(cls.slots, Cfg::BLOCK)), dim3(Cfg::BLOCK), 0, stream, dPts.get(), dSlotIndex.get(),
                               dSlotCoef.get(), cls.slots, dProd.get());
            UG_KERNEL_CHECK();
        }
        sc.stop();
    }
    {
        StreamTimer::Scope sc = timer.time(stream, &sums);
        if (!pieces.empty()) {
            hipLaunchKernelGGL(piece_points_kernel<Cfg>, dim3((unsigned)pieces.size()), dim3(Cfg::PIECE_BLOCK), 0, stream, a, dPartial.get());
            UG_KERNEL_CHECK();
        }
        hipLaunchKernelGGL(column_points_kernel<Cfg>, dim3(grid_for((nCols + Cfg::KPL - 1) / Cfg::KPL, Cfg::BLOCK)), dim3(Cfg::BLOCK), 0, stream, a, dOut.get());
        UG_KERNEL_CHECK();
        sc.stop();
    }
    UG_HIP(hipMemcpyAsync(out, dOut.get(), nCols * REC, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipStreamSynchronize(stream));
    timer.resolve();
    if (ms) { ms[0] = products.ms; ms[1] = sums.ms; }
}

}  // namespace

void device_points_combine(hipStream_t stream, StreamTimer& timer, bool g2, u64 nCols, const u32* colPtr, const u32* index,
                           const uint8_t* coefs, const ughost::setup::PointSegs& pts, uint8_t* out, double* ms) {
    if (ms) ms[0] = ms[1] = 0;
    if (!nCols) return;
    if (g2) combine_on_device<P2>(stream, timer, nCols, colPtr, index, coefs, pts, out, ms);
    else combine_on_device<P1>(stream, timer, nCols, colPtr, index, coefs, pts, out, ms);
}

void device_points_scale(hipStream_t stream, StreamTimer& timer, const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out, double* ms) {
    if (ms) ms[0] = 0;
    if (!n) return;
    uint8_t one[32] = {1};
    if (!memcmp(scalar, one, 32)) { memcpy(out, points, n * 64); return; }      // (delta = 1: no launch)
    if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
    WnafArgs a;
    a.top = recodeWnaf(scalar, SCALE_WINDOW, a.digit);
    DevBuf<u32> dPts(n * 16), dOut(n * 16);
    UG_HIP(hipMemcpyAsync(dPts.get(), points, n * 64, hipMemcpyHostToDevice, stream));
    convert_points_g1(dPts.get(), n, stream);
    TimeSink sink;
    {
        StreamTimer::Scope sc = timer.time(stream, &sink);
        hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n, 128)), dim3(128), 0, stream, dPts.get(), n, a, dOut.get());
        UG_KERNEL_CHECK();
        sc.stop();
    }
    UG_HIP(hipMemcpyAsync(out, dOut.get(), n * 64, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipStreamSynchronize(stream));
    timer.resolve();
    volatile int8_t* w = a.digit;                // (the digits are 1 / delta)
    for (int i = 0; i < 256; i++) w[i] = 0;
    if (ms) ms[0] = sink.ms;
}

// The block sums of the ratio test: weights n x 16 bytes; sumX, sumY: one record per block of RATIO_BLOCK records.
void device_points_ratio_sums(hipStream_t stream, StreamTimer& timer, const uint8_t* x, const uint8_t* y, u64 n, const uint8_t* weights,
                              uint8_t* sumX, uint8_t* sumY, double* ms) {
    if (ms) ms[0] = 0;
    if (!n) return;
    if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
    const u64 blocks = (n + RATIO_LANES - 1) / RATIO_LANES;
    DevBuf<u32> dX(n * 16), dY(n * 16), dW(n * 4), dSums(blocks * 32);
    UG_HIP(hipMemcpyAsync(dX.get(), x, n * 64, hipMemcpyHostToDevice, stream));
    UG_HIP(hipMemcpyAsync(dY.get(), y, n * 64, hipMemcpyHostToDevice, stream));
    UG_HIP(hipMemcpyAsync(dW.get(), weights, n * 16, hipMemcpyHostToDevice, stream));
    convert_points_g1(dX.get(), n, stream);
    convert_points_g1(dY.get(), n, stream);
    TimeSink sink;
    {
        StreamTimer::Scope sc = timer.time(stream, &sink);
        hipLaunchKernelGGL(ratio_block_sums_kernel, dim3((unsigned)blocks), dim3(RATIO_LANES), 0, stream, dX.get(), dY.get(), dW.get(), (u32)n, dSums.get());
        UG_KERNEL_CHECK();
        sc.stop();
    }
    std::vector<uint8_t> both((size_t)blocks * 128);
    UG_HIP(hipMemcpyAsync(both.data(), dSums.get(), blocks * 128, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipStreamSynchronize(stream));
    timer.resolve();
    for (u64 j = 0; j < blocks; j++) {
        memcpy(sumX + j * 64, &both[(size_t)j * 128], 64);
        memcpy(sumY + j * 64, &both[(size_t)j * 128 + 64], 64);
    }
    if (ms) ms[0] = sink.ms;
}

// One launch for all segments. Segments that name the same source array share one upload (C1 and C2 both gather from the K
// records); every index was checked against nSrc by the caller.
void device_points_scale_segments(hipStream_t stream, StreamTimer& timer, const ScaleSeg* segs, int n, double* ms) {
    if (ms) ms[0] = 0;
    if (n < 0 || n > MAX_SCALE_SEGS) throw SetupError("internal: " + std::to_string(n) + " segments");
    SegmentsArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    const uint8_t one[32] = {1};
    DevBuf<u32> dSrc[MAX_SCALE_SEGS], dIndex[MAX_SCALE_SEGS], dOut[MAX_SCALE_SEGS];
    u64 blocks = 0;
    for (int s = 0; s < n; s++) {
        const ScaleSeg& g = segs[s];
        if (g.count > 0xffffffffull || g.nSrc > 0xffffffffull || blocks + grid_for(g.count, SEG_BLOCK) > 0x7fffffffull)
            throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        a.seg[s].count = (u32)g.count;
        a.seg[s].first_block = (u32)blocks;
        blocks += grid_for(g.count, SEG_BLOCK);
        a.seg[s].top = !memcmp(g.scalar, one, 32) ? -2 : recodeWnaf(g.scalar, SCALE_WINDOW, a.digit[s]);
        if (!g.count) continue;
        int same = -1;
        for (int t = 0; t < s; t++)
            if (segs[t].count && segs[t].src == g.src && segs[t].nSrc == g.nSrc) { same = t; break; }
        if (same >= 0) a.seg[s].src = a.seg[same].src;
        else {
            dSrc[s].alloc(std::max<u64>(g.nSrc, 1) * 16);
            if (g.nSrc) UG_HIP(hipMemcpyAsync(dSrc[s].get(), g.src, g.nSrc * 64, hipMemcpyHostToDevice, stream));
            convert_points_g1(dSrc[s].get(), g.nSrc, stream);
            a.seg[s].src = dSrc[s].get();
        }
        if (g.index) {
            upload(dIndex[s], g.index, g.count, stream);
            a.seg[s].index = dIndex[s].get();
        }
        dOut[s].alloc(g.count * 16);
        a.seg[s].out = dOut[s].get();
    }
    TimeSink sink;
    if (blocks) {
        StreamTimer::Scope sc = timer.time(stream, &sink);
        hipLaunchKernelGGL(scale_segments_kernel, dim3((unsigned)blocks), dim3(SEG_BLOCK), 0, stream, a);
        UG_KERNEL_CHECK();
        sc.stop();
    }
    for (int s = 0; s < n; s++)
        if (segs[s].count) UG_HIP(hipMemcpyAsync(segs[s].out, dOut[s].get(), segs[s].count * 64, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipStreamSynchronize(stream));
    timer.resolve();
    volatile int8_t* w = &a.digit[0][0];         // (the digits are 1 / delta)
    for (int i = 0; i < MAX_SCALE_SEGS * 256; i++) w[i] = 0;
    if (ms) ms[0] = sink.ms;
}

}  // namespace ug
