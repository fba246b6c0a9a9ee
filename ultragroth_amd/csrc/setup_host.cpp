// setup_host.cpp -- the development setup's host layer: checks, plan, column index, section 4, headers, verification key, the
// host-thread backend, and the extern "C" entries (include/ultragroth_hip.h: ug_setup_*, ug_generator_mul, ug_lagrange_at).
// The key this makes is a TEST key: whoever knows the trapdoor forges proofs.
//
// The specification is tests/golden/make_trapdoor_fixtures.py; the file layout follows it byte for byte.
#include "setup_host.hpp"
#include "pairing.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

namespace ughost {
namespace setup {

using namespace ug;

DeviceBackendFactory deviceBackendFactory = nullptr;

double nowMs() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace {

unsigned threadCount(u64 n, u64 grain) {
    unsigned hw = std::thread::hardware_concurrency();
    return (unsigned)std::max<u64>(1, std::min<u64>({hw ? hw : 1u, 16u, n / std::max<u64>(grain, 1) + 1}));
}

}  // namespace

// fn(lo, hi) over [0, n) in pieces of `grain`, handed out to at most 16 host threads
void parallelFor(u64 n, u64 grain, const std::function<void(u64, u64)>& fn) {
    if (!n) return;
    const unsigned T = threadCount(n, grain);
    std::atomic<u64> next{0};
    std::mutex errLock;
    std::exception_ptr err;
    auto work = [&]() {
        try {
            for (;;) {
                const u64 lo = next.fetch_add(grain);
                if (lo >= n) return;
                fn(lo, std::min(n, lo + grain));
            }
        } catch (...) {
            std::lock_guard<std::mutex> g(errLock);
            if (!err) err = std::current_exception();
            next.store(n);
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    if (err) std::rethrow_exception(err);
}

Fr frFromPlain(const uint8_t* le) {
    u32 w[8];
    memcpy(w, le, 32);
    return cond_sub_q(from_normal<FrParams>(w));
}
void frToPlain(uint8_t* le, const Fr& a) {
    u32 w[8];
    to_normal(w, a);
    memcpy(le, w, 32);
}

bool belowR(const uint8_t* le) {
    for (int i = 31; i >= 0; i--) {
        if (le[i] < BN254_R_BYTES[i]) return true;
        if (le[i] > BN254_R_BYTES[i]) return false;
    }
    return false;
}

bool coefMagnitude(const uint8_t* le, u32 mag[8]) {
    u32 c[8], d[8];
    memcpy(c, le, 32);
    // d = r - c; negate when d < c, i.e. c > r / 2 (r is odd: never equal)
    int64_t borrow = 0;
    for (int i = 0; i < 8; i++) {
        const int64_t v = (int64_t)FrParams::q32[i] - (int64_t)c[i] + borrow;
        d[i] = (u32)v;
        borrow = v >> 32;
    }
    bool less = false;                          // d < c, decided by the highest differing word
    for (int i = 0; i < 8; i++)
        if (d[i] != c[i]) less = d[i] < c[i];
    memcpy(mag, less ? d : c, 32);
    return less;
}

int recodeWnaf(const uint8_t* le, int w, int8_t digit[256]) {
    u32 k[9] = {0};
    memcpy(k, le, 32);
    memset(digit, 0, 256);
    int top = -1;
    const int full = 1 << w, half = full >> 1;
    for (int i = 0; i < 256; i++) {
        if (k[0] & 1) {
            int d = (int)(k[0] & (u32)(full - 1));
            if (d >= half) d -= full;
            digit[i] = (int8_t)d;
            top = i;
            // k -= d
            int64_t carry = -(int64_t)d;
            for (int j = 0; j < 9 && carry; j++) {
                const int64_t v = (int64_t)k[j] + carry;
                k[j] = (u32)v;
                carry = v >> 32;
            }
        }
        for (int j = 0; j < 8; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 31);
        k[8] >>= 1;
    }
    return top;
}

void columnPieces(const u32* colPtr, u64 nCols, u32 m, std::vector<Piece>& pieces) {
    for (u64 s = 0; s < nCols; s++) {
        const u32 lo = colPtr[s], hi = colPtr[s + 1];
        if (hi - lo <= SPLIT_THRESHOLD) continue;
        for (u64 f = lo; f < hi; f += SPLIT_PIECE) pieces.push_back({m, (u32)s, (u32)f, (u32)std::min<u64>(hi, f + SPLIT_PIECE)});
    }
}

namespace {

Fr frSmall(u32 v) {
    uint8_t le[32] = {0};
    memcpy(le, &v, 4);
    return frFromPlain(le);
}
Fr frPow2k(Fr a, int k) {                       // a^(2^k)
    for (int i = 0; i < k; i++) a = frMul(a, a);
    return a;
}
Fr frInv(const Fr& a) { return cond_sub_q(inv(a)); }
bool frIsZero(const Fr& a) { return limbs_all_zero(a); }
bool frIsOne(const Fr& a) { return equal(a, fp_one<FrParams>()); }

// 5^((r - 1) / 2^k): the 2^k-th root of unity the prover's domains use
Fr rootOfUnity(int k) {
    u32 e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::q32[i];
    e[0] -= 1;
    for (int s = 0; s < k; s++) {               // e >>= 1
        for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i + 1 < 8 ? e[i + 1] << 31 : 0u);
    }
    return cond_sub_q(pow256(frSmall(FrParams::generator), e));
}

// ---- the generators, affine, canonical device form ----
const u32 G2_WORDS[4][8] = {
    {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
    {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
    {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
    {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};

Fq fqPlain(const u32* w) { return cond_sub_q(from_normal<FqParams>(w)); }

template <class F> struct Gen;
template <> struct Gen<Fq> {
    static constexpr int REC = 64;
    static void generator(Fq& x, Fq& y) {
        const u32 one[8] = {1}, two[8] = {2};
        x = fqPlain(one); y = fqPlain(two);
    }
    static void store(uint8_t* o, const Fq& x, const Fq& y) {
        u32 w[16];
        to_mont256(w, x); to_mont256(w + 8, y);
        memcpy(o, w, 64);
    }
    static bool load(const uint8_t* rec, Fq& x, Fq& y) {      // false: the all-zero record, infinity
        u32 w[16];
        memcpy(w, rec, 64);
        u32 o = 0;
        for (int i = 0; i < 16; i++) o |= w[i];
        if (!o) return false;
        x = cond_sub_q(from_mont256<FqParams>(w)); y = cond_sub_q(from_mont256<FqParams>(w + 8));
        return true;
    }
};
template <> struct Gen<Fq2> {
    static constexpr int REC = 128;
    static void generator(Fq2& x, Fq2& y) {
        x.a = fqPlain(G2_WORDS[0]); x.b = fqPlain(G2_WORDS[1]); y.a = fqPlain(G2_WORDS[2]); y.b = fqPlain(G2_WORDS[3]);
    }
    static void store(uint8_t* o, const Fq2& x, const Fq2& y) {
        u32 w[32];
        to_mont256(w, x.a); to_mont256(w + 8, x.b); to_mont256(w + 16, y.a); to_mont256(w + 24, y.b);
        memcpy(o, w, 128);
    }
    static bool load(const uint8_t* rec, Fq2& x, Fq2& y) {
        u32 w[32];
        memcpy(w, rec, 128);
        u32 o = 0;
        for (int i = 0; i < 32; i++) o |= w[i];
        if (!o) return false;
        x.a = cond_sub_q(from_mont256<FqParams>(w)); x.b = cond_sub_q(from_mont256<FqParams>(w + 8));
        y.a = cond_sub_q(from_mont256<FqParams>(w + 16)); y.b = cond_sub_q(from_mont256<FqParams>(w + 24));
        return true;
    }
};

// XYZZ points -> affine with one shared inversion (Montgomery's trick); infinity: live[i] = false
template <class F> void batchAffine(std::vector<XYZZ<F>>& p, std::vector<F>& ax, std::vector<F>& ay, std::vector<char>& live) {
    const size_t n = p.size();
    ax.resize(n); ay.resize(n); live.resize(n);
    std::vector<F> pre(n);
    F run = field_one((F*)0);
    for (size_t i = 0; i < n; i++) {
        live[i] = !is_inf(p[i]);
        pre[i] = run;
        if (live[i]) run = mulk<8>(run, p[i].zzz);
    }
    F irun = inv(run);
    for (size_t i = n; i-- > 0;) {
        if (!live[i]) continue;
        F izzz = mulk<8>(irun, pre[i]);
        irun = mulk<8>(irun, p[i].zzz);
        F iz = mulk<8>(izzz, p[i].zz);
        F izz = sqrk<8>(iz);
        ax[i] = canon(mulk<8>(p[i].x, izz));
        ay[i] = canon(mulk<8>(p[i].y, izzz));
    }
}

// the host's window tables: 32 tables of the unsigned 8-bit digits 1 .. 255, entry (j, d) = d * 2^(8 j) * G
template <class F> struct HostTable {
    static constexpr int C = 8, W = 32, D = 255;
    std::vector<F> x, y;
    HostTable() {
        std::vector<XYZZ<F>> pts((size_t)W * D);
        F gx, gy;
        Gen<F>::generator(gx, gy);
        XYZZ<F> base = xyzz_from_affine(gx, gy);
        for (int j = 0; j < W; j++) {
            XYZZ<F> acc = base;
            for (int d = 1; d <= D; d++) {
                pts[(size_t)j * D + d - 1] = acc;
                acc = xyzz_add(acc, base);
            }
            base = acc;                          // 256 * base
        }
        std::vector<char> live;
        batchAffine(pts, x, y, live);
    }
    static const HostTable& get() {
        static const HostTable t;
        return t;
    }
};

template <class F> void hostGeneratorMul(const uint8_t* scalars, u64 n, uint8_t* out) {
    const HostTable<F>& tab = HostTable<F>::get();
    constexpr int REC = Gen<F>::REC;
    parallelFor(n, 256, [&](u64 lo, u64 hi) {
        std::vector<XYZZ<F>> acc(hi - lo);
        for (u64 i = lo; i < hi; i++) {
            const uint8_t* s = scalars + i * 32;
            XYZZ<F> a = xyzz_inf<F>();
            for (int j = 0; j < 32; j++) {
                const int d = s[j];
                if (d) a = xyzz_madd(a, tab.x[(size_t)j * 255 + d - 1], tab.y[(size_t)j * 255 + d - 1]);
            }
            acc[i - lo] = a;
        }
        std::vector<F> ax, ay;
        std::vector<char> live;
        batchAffine(acc, ax, ay, live);
        for (u64 i = lo; i < hi; i++) {
            if (live[i - lo]) Gen<F>::store(out + i * REC, ax[i - lo], ay[i - lo]);
            else memset(out + i * REC, 0, REC);
        }
    });
}

void checkScalars(const uint8_t* scalars, u64 n) {
    for (u64 i = 0; i < n; i++)
        if (!belowR(scalars + i * 32)) throw SetupError("scalar " + std::to_string(i) + " is not below the field modulus");
}

// results of a piece of work -> zkey records, one shared inversion
template <class F> void storeAffine(std::vector<XYZZ<F>>& acc, uint8_t* out) {
    std::vector<F> ax, ay;
    std::vector<char> live;
    batchAffine(acc, ax, ay, live);
    for (size_t i = 0; i < acc.size(); i++) {
        if (live[i]) Gen<F>::store(out + i * Gen<F>::REC, ax[i], ay[i]);
        else memset(out + i * Gen<F>::REC, 0, Gen<F>::REC);
    }
}

// The per-column point combination, one column at a time (a long column stays with one thread, as in points() below). A unit
// coefficient is a mixed addition; every other one goes through the host's 4-bit signed-window product of its magnitude.
template <class F>
void hostCombine(u64 nCols, const u32* colPtr, const u32* index, const uint8_t* coefs, const PointSegs& pts, uint8_t* out) {
    constexpr int REC = Gen<F>::REC;
    parallelFor(nCols, 64, [&](u64 lo, u64 hi) {
        std::vector<XYZZ<F>> acc(hi - lo);
        for (u64 s = lo; s < hi; s++) {
            XYZZ<F> a = xyzz_inf<F>();
            for (u32 q = colPtr[s]; q < colPtr[s + 1]; q++) {
                u32 mag[8];
                const bool negate = coefMagnitude(coefs + (size_t)q * 32, mag);
                const int bits = bitLength(mag);
                F x, y;
                if (!bits || !Gen<F>::load(pts.base[index[q] / pts.count] + (index[q] % pts.count) * REC, x, y)) continue;
                if (negate) y = canon(neg<1>(y));
                if (bits == 1) a = xyzz_madd(a, x, y);
                else a = xyzz_add(a, xyzz_mul_scalar_w4(xyzz_from_affine(x, y), mag));
            }
            acc[s - lo] = a;
        }
        storeAffine(acc, out + lo * REC);
    });
}

void hostScale(const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out) {
    u32 k[8];
    memcpy(k, scalar, 32);
    parallelFor(n, 64, [&](u64 lo, u64 hi) {
        std::vector<XYZZ<Fq>> acc(hi - lo);
        for (u64 i = lo; i < hi; i++) {
            Fq x, y;
            acc[i - lo] = Gen<Fq>::load(points + i * 64, x, y) ? xyzz_mul_scalar_w4(xyzz_from_affine(x, y), k) : xyzz_inf<Fq>();
        }
        storeAffine(acc, out + lo * 64);
    });
}

// The delta step of an UltraGroth key, a segment at a time: the gather, then hostScale (1: the gathered records as they are)
void hostScaleSegments(const ScaleSeg* segs, int n) {
    const uint8_t one[32] = {1};
    for (int s = 0; s < n; s++) {
        const ScaleSeg& g = segs[s];
        if (!g.count) continue;
        const uint8_t* in = g.src;
        std::vector<uint8_t> gathered;
        if (g.index) {
            gathered.resize((size_t)g.count * 64);
            parallelFor(g.count, 4096, [&](u64 lo, u64 hi) {
                for (u64 i = lo; i < hi; i++) memcpy(&gathered[(size_t)i * 64], g.src + (size_t)g.index[i] * 64, 64);
            });
            in = gathered.data();
        }
        if (!memcmp(g.scalar, one, 32)) { if (in != g.out) memcpy(g.out, in, (size_t)g.count * 64); }
        else hostScale(g.scalar, in, g.count, g.out);
    }
}

// The inverse transform over points, the stages of ptau_prepare.hip on host threads: (1 / N) P_i to the bit-reversed index, then
// one pass per stage over the butterflies, the records affine in `out` between the passes; a piece of butterflies shares one
// inversion. The products go through the host's 4-bit signed-window form.
template <class F> XYZZ<F> foldedProduct(const u32 folded[8], F x, F y) {
    u32 mag[8];
    memcpy(mag, folded, 32);
    if (mag[7] >> 31) y = canon(neg<1>(y));
    mag[7] &= 0x7fffffffu;
    return xyzz_mul_scalar_w4(xyzz_from_affine(x, y), mag);
}
template <class F> void hostIntt(int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out) {
    constexpr int REC = Gen<F>::REC;
    const u64 N = 1ull << logN, half = N / 2;
    std::vector<u32> tw;
    inttTwiddles(logN, tw);
    u32 c[8];
    inttScale(logN, c);
    for (int v = 0; v < nVec; v++) {
        const uint8_t* src = in[v];
        uint8_t* dst = out[v];
        parallelFor(N, 64, [&](u64 lo, u64 hi) {
            std::vector<XYZZ<F>> acc(hi - lo);
            for (u64 i = lo; i < hi; i++) {
                F x, y;
                acc[i - lo] = i < nGiven && Gen<F>::load(src + i * REC, x, y) ? foldedProduct(c, x, y) : xyzz_inf<F>();
            }
            std::vector<F> ax, ay;
            std::vector<char> live;
            batchAffine(acc, ax, ay, live);
            for (u64 i = lo; i < hi; i++) {
                u64 j = 0;
                for (int b = 0; b < logN; b++) j |= ((i >> b) & 1) << (logN - 1 - b);
                if (live[i - lo]) Gen<F>::store(dst + j * REC, ax[i - lo], ay[i - lo]);
                else memset(dst + j * REC, 0, REC);
            }
        });
        for (int s = 0; s < logN; s++) {
            parallelFor(half, 32, [&](u64 lo, u64 hi) {
                std::vector<XYZZ<F>> res(2 * (hi - lo));
                std::vector<uint8_t*> at(2 * (hi - lo));
                for (u64 t = lo; t < hi; t++) {
                    const u64 j = t & ((1ull << s) - 1);
                    uint8_t* pa = dst + (((t >> s) << (s + 1)) + j) * REC;
                    uint8_t* pb = pa + ((u64)REC << s);
                    F ax, ay, bx, by;
                    XYZZ<F> tv = xyzz_inf<F>();
                    if (Gen<F>::load(pb, bx, by)) tv = j ? foldedProduct(&tw[(size_t)(j << (logN - 1 - s)) * 8], bx, by) : xyzz_from_affine(bx, by);
                    XYZZ<F> sum = tv, dif = xyzz_neg(tv);
                    if (Gen<F>::load(pa, ax, ay)) {
                        sum = xyzz_madd(tv, ax, ay);
                        dif = xyzz_neg(xyzz_madd(tv, ax, canon(neg<1>(ay))));       // a - t = -(t - a)
                    }
                    res[2 * (t - lo)] = sum; at[2 * (t - lo)] = pa;
                    res[2 * (t - lo) + 1] = dif; at[2 * (t - lo) + 1] = pb;
                }
                std::vector<F> x, y;
                std::vector<char> live;
                batchAffine(res, x, y, live);
                for (size_t i = 0; i < res.size(); i++) {
                    if (live[i]) Gen<F>::store(at[i], x[i], y[i]);
                    else memset(at[i], 0, REC);
                }
            });
        }
    }
}

// ---- the host-thread backend ----
class HostBackend : public Backend {
public:
    void lagrange(int logN, const Fr& x, const Fr& scale, const Fr& omega, uint8_t* out) override {
        const u64 N = 1ull << logN;
        parallelFor(N, 1024, [&](u64 lo, u64 hi) {
            // omega^lo by square and multiply, then a running product; one inversion for the piece
            Fr w = fp_one<FrParams>(), b = omega;
            for (u64 e = lo; e; e >>= 1) { if (e & 1) w = frMul(w, b); b = frMul(b, b); }
            const size_t n = (size_t)(hi - lo);
            std::vector<Fr> wk(n), d(n), pre(n);
            Fr run = fp_one<FrParams>();
            for (size_t i = 0; i < n; i++) {
                wk[i] = w;
                d[i] = frSub(x, w);
                pre[i] = run;
                run = frMul(run, d[i]);
                w = frMul(w, omega);
            }
            Fr irun = frInv(run);
            for (size_t i = n; i-- > 0;) {
                const Fr id = frMul(irun, pre[i]);
                irun = frMul(irun, d[i]);
                frToPlain(out + (lo + i) * 32, frMul(frMul(scale, wk[i]), id));
            }
        });
    }
    void generatorMul(bool g2, const uint8_t* scalars, u64 n, int, uint8_t* out, double* ms) override {
        const double t0 = nowMs();
        if (g2) hostGeneratorMul<Fq2>(scalars, n, out);
        else hostGeneratorMul<Fq>(scalars, n, out);
        if (ms) { ms[0] = 0; ms[1] = nowMs() - t0; }
    }
    void combine(bool g2, u64 nCols, const u32* colPtr, const u32* index, const uint8_t* coefs, const PointSegs& pts, uint8_t* out,
                 double* ms) override {
        const double t0 = nowMs();
        if (g2) hostCombine<Fq2>(nCols, colPtr, index, coefs, pts, out);
        else hostCombine<Fq>(nCols, colPtr, index, coefs, pts, out);
        if (ms) { ms[0] = 0; ms[1] = nowMs() - t0; }
    }
    void scale(const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out, double* ms) override {
        const double t0 = nowMs();
        hostScale(scalar, points, n, out);
        if (ms) ms[0] = nowMs() - t0;
    }
    void scaleSegments(const ScaleSeg* segs, int n, double* ms) override {
        const double t0 = nowMs();
        hostScaleSegments(segs, n);
        if (ms) ms[0] = nowMs() - t0;
    }
    // the block sums are a combination with one column per block; the pairings are pairing.hpp's on host threads
    void ratio(const uint8_t* x, const uint8_t* y, u64 n, const uint8_t* q, u64 maxBlocks, RatioOut& out) override {
        if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        u32 q2[RATIO_Q2_WORDS];
        ratioG2Words(q, q2);
        const pr::FinalExpConsts& kc = ratioConsts();
        ratioLevels(x, y, n, maxBlocks, out,
                    [&](const uint8_t* w, uint8_t* sx, uint8_t* sy, double* ms) {
                        const double t0 = nowMs();
                        const u64 blocks = (n + RATIO_BLOCK - 1) / RATIO_BLOCK;
                        std::vector<u32> colPtr((size_t)blocks + 1), index((size_t)n);
                        std::vector<uint8_t> coefs((size_t)n * 32, 0);
                        for (u64 j = 0; j <= blocks; j++) colPtr[(size_t)j] = (u32)std::min(n, j * RATIO_BLOCK);
                        for (u64 i = 0; i < n; i++) { index[(size_t)i] = (u32)i; memcpy(&coefs[(size_t)i * 32], w + i * 16, 16); }
                        PointSegs p;
                        p.count = n; p.n = 1;
                        p.base[0] = x;
                        hostCombine<Fq>(blocks, colPtr.data(), index.data(), coefs.data(), p, sx);
                        p.base[0] = y;
                        hostCombine<Fq>(blocks, colPtr.data(), index.data(), coefs.data(), p, sy);
                        *ms = nowMs() - t0;
                    },
                    [&](const uint8_t* px, const uint8_t* py, u64 m, uint8_t* wrong, double* ms) {
                        const double t0 = nowMs();
                        parallelFor(m, 4, [&](u64 lo, u64 hi) {
                            for (u64 i = lo; i < hi; i++) {
                                u32 rx[16], ry[16];      // (a file's records sit at any alignment)
                                memcpy(rx, px + i * 64, 64);
                                memcpy(ry, py + i * 64, 64);
                                wrong[i] = pr::ratio_holds(kc, rx, ry, q2) ? 0 : 1;
                            }
                        });
                        *ms = nowMs() - t0;
                    });
    }
    void intt(bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out, double* ms) override {
        const double t0 = nowMs();
        if (!inttTrivial(g2, logN, nVec, in, nGiven, out)) {
            if (g2) hostIntt<Fq2>(logN, nVec, in, nGiven, out);
            else hostIntt<Fq>(logN, nVec, in, nGiven, out);
        }
        if (ms) { ms[0] = 0; ms[1] = nowMs() - t0; }
    }
    void points(const Plan& p, const ColMatrix cm[3], const std::vector<Piece>&, uint8_t* a, uint8_t* b1, uint8_t* b2, uint8_t* k,
                uint8_t* h, double ms[PHASES]) override {
        PhaseClock clock(ms);
        const u64 N = p.N, M = p.nVars;
        std::vector<uint8_t> lag(N * 32), lagCoset(N * 32);
        lagrange(p.logN, p.x[0], p.lagScale[0], p.omega, lag.data());
        lagrange(p.logN, p.x[1], p.lagScale[1], p.omega, lagCoset.data());
        clock.lap(1);
        // the transposed products: one wire at a time over its column (a long column stays with one thread here: the pieces
        // are the device's answer to a lane that would otherwise walk a million terms alone)
        std::vector<uint8_t> sa(M * 32), sb(M * 32), sk(M * 32), sh(N * 32);
        parallelFor(M, 512, [&](u64 lo, u64 hi) {
            for (u64 s = lo; s < hi; s++) {
                Fr uvw[3];
                for (int m = 0; m < 3; m++) {
                    Fr acc = fp_zero<FrParams>();
                    for (u32 q = cm[m].colPtr[s]; q < cm[m].colPtr[s + 1]; q++)
                        acc = frAdd(acc, frMul(frFromPlain(&cm[m].val[(size_t)q * 32]), frFromPlain(&lag[(size_t)cm[m].row[q] * 32])));
                    uvw[m] = acc;
                }
                const Fr K = frAdd(frAdd(frMul(p.beta, uvw[0]), frMul(p.alpha, uvw[1])), uvw[2]);
                frToPlain(&sa[s * 32], uvw[0]);
                frToPlain(&sb[s * 32], uvw[1]);
                frToPlain(&sk[s * 32], frMul(K, p.inv[p.cls[s]]));
            }
        });
        parallelFor(N, 4096, [&](u64 lo, u64 hi) {
            for (u64 i = lo; i < hi; i++) frToPlain(&sh[i * 32], frMul(frFromPlain(&lagCoset[i * 32]), p.hScale));
        });
        clock.lap(2);
        hostGeneratorMul<Fq>(sa.data(), M, a);
        hostGeneratorMul<Fq>(sb.data(), M, b1);
        hostGeneratorMul<Fq>(sk.data(), M, k);
        hostGeneratorMul<Fq>(sh.data(), N, h);
        clock.lap(3);
        hostGeneratorMul<Fq2>(sb.data(), M, b2);
        clock.lap(4);
    }
};

}  // namespace

// ---- options -> plan ----
void planSizes(const R1csHeader& h, u32 logDomain, Plan& p) {
    p.nVars = h.nWires; p.nConstraints = h.nConstraints;
    const u64 nPublic = (u64)h.nPubOut + h.nPubIn;
    if (nPublic + 1 > h.nWires) throw SetupError("nPubOut + nPubIn + 1 exceeds nWires");
    p.nPublic = (u32)nPublic;
    const u64 rows = (u64)h.nConstraints + nPublic + 1;
    int need = 0;
    while ((1ull << need) < rows) need++;
    if (need > MAX_LOG_DOMAIN) throw SetupError("sizes that cannot be represented: " + std::to_string(rows) + " rows need a domain above 2^" + std::to_string(MAX_LOG_DOMAIN));
    if (logDomain == 0) p.logN = std::max(need, 1);
    else {
        if (logDomain > (u32)MAX_LOG_DOMAIN) throw SetupError("log_domain " + std::to_string(logDomain) + " is above the prover's largest domain, 2^" + std::to_string(MAX_LOG_DOMAIN));
        if ((int)logDomain < need) throw SetupError("log_domain " + std::to_string(logDomain) + " is too small for " + std::to_string(rows) + " rows");
        p.logN = (int)logDomain;
    }
    p.N = 1u << p.logN;
    p.cls.assign(p.nVars, 2);
    for (u32 s = 0; s <= p.nPublic; s++) p.cls[s] = 0;
}

void planLists(Plan& p, u32 randIndx, const u32* roundSignals, u64 nRound, const u32* finalSignals, u64 nFinal) {
    p.ultra = true;
    if (randIndx < 1 || randIndx > p.nPublic) throw SetupError("rand_indx " + std::to_string(randIndx) + " is not a public signal");
    p.randIndx = randIndx;
    if ((nRound && !roundSignals) || (nFinal && !finalSignals)) throw SetupError("null signal list");
    if (nRound + nFinal != (u64)p.nVars - p.nPublic - 1)
        throw SetupError("the round and final signal lists do not partition the private signals " + std::to_string(p.nPublic + 1) + " .. " + std::to_string(p.nVars - 1));
    p.roundSignals.assign(roundSignals, roundSignals + nRound);
    p.finalSignals.assign(finalSignals, finalSignals + nFinal);
    std::vector<uint8_t> seen(p.nVars, 0);
    for (int which = 0; which < 2; which++)
        for (u32 s : which ? p.finalSignals : p.roundSignals) {
            if (s <= p.nPublic || s >= p.nVars || seen[s])
                throw SetupError("the round and final signal lists do not partition the private signals: signal " + std::to_string(s));
            seen[s] = 1;
            p.cls[s] = which ? 2 : 1;
        }
}

namespace {

struct Named { const char* name; const uint8_t* v; bool nonzero; };

void makePlan(const ug_setup_options* o, const R1csHeader& h, Plan& p) {
    if (!o) throw SetupError("null options");
    if (o->size != sizeof(ug_setup_options)) throw SetupError("options struct of another size (" + std::to_string(o->size) + ")");
    if (o->protocol != 1 && o->protocol != 1337) throw SetupError("protocol " + std::to_string(o->protocol) + " is neither 1 (Groth16) nor 1337 (UltraGroth)");
    p.ultra = o->protocol == 1337;
    p.opt = *o;
    const Named vals[6] = {{"tau", o->tau, false}, {"alpha", o->alpha, true}, {"beta", o->beta, true}, {"gamma", o->gamma, true},
                           {"delta_round", o->delta_round, p.ultra}, {"delta_final", o->delta_final, true}};
    for (const Named& n : vals) {
        if (!p.ultra && n.v == o->delta_round) continue;      // (protocol 1 reads delta_final only)
        if (!belowR(n.v)) throw SetupError(std::string(n.name) + " is not below the field modulus");
        if (n.nonzero && frIsZero(frFromPlain(n.v))) throw SetupError(std::string(n.name) + " is 0 mod r");
    }
    planSizes(h, o->log_domain, p);
    if (p.ultra) planLists(p, o->rand_indx, o->round_signals, o->n_round, o->final_signals, o->n_final);
    // field constants
    const Fr tau = frFromPlain(o->tau), one = fp_one<FrParams>();
    const Fr tauN = frPow2k(tau, p.logN);
    if (frIsOne(frMul(tauN, tauN))) throw SetupError("tau^(2N) = 1: tau or tau / g lies in the evaluation domain");
    p.omega = rootOfUnity(p.logN);
    const Fr g = rootOfUnity(p.logN + 1);
    const Fr nInv = frInv(frSmall(p.N));
    p.x[0] = tau;
    p.x[1] = frMul(tau, frInv(g));
    p.lagScale[0] = frMul(frSub(tauN, one), nInv);
    p.lagScale[1] = frMul(frSub(frPow2k(p.x[1], p.logN), one), nInv);
    p.alpha = frFromPlain(o->alpha); p.beta = frFromPlain(o->beta);
    p.inv[0] = frInv(frFromPlain(o->gamma));
    p.inv[1] = p.ultra ? frInv(frFromPlain(o->delta_round)) : fp_zero<FrParams>();
    p.inv[2] = frInv(frFromPlain(o->delta_final));
    const Fr minus2d = frSub(fp_zero<FrParams>(), frMul(frSmall(2), frFromPlain(o->delta_final)));
    p.hScale = frMul(frSub(tauN, one), frInv(minus2d));
}

}  // namespace

// ---- the column index: a counting sort of each matrix's terms by wire, rows ascending inside a column ----
void buildColumns(const R1cs& cs, const Plan& p, ColMatrix cm[3], std::vector<Piece>& pieces) {
    uint8_t oneLe[32] = {1};
    for (int m = 0; m < 3; m++) {
        const R1csMatrix& src = cs.m[m];
        const u64 extra = m == 0 ? (u64)p.nPublic + 1 : 0, terms = src.sig.size() + extra;
        if (terms > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 terms in one matrix");
        ColMatrix& c = cm[m];
        c.colPtr.assign((size_t)p.nVars + 1, 0);
        for (u32 s : src.sig) c.colPtr[s + 1]++;
        for (u64 s = 0; s < extra; s++) c.colPtr[s + 1]++;
        for (u32 s = 0; s < p.nVars; s++) c.colPtr[s + 1] += c.colPtr[s];
        c.row.assign(terms, 0);
        c.val.assign(terms * 32, 0);
        std::vector<u32> at(c.colPtr.begin(), c.colPtr.end() - 1);
        for (u32 k = 0; k < p.nConstraints; k++)
            for (u32 q = src.rowPtr[k]; q < src.rowPtr[k + 1]; q++) {
                const u32 pos = at[src.sig[q]]++;
                c.row[pos] = k;
                memcpy(&c.val[(size_t)pos * 32], &src.val[(size_t)q * 32], 32);
            }
        for (u64 s = 0; s < extra; s++) {
            const u32 pos = at[s]++;
            c.row[pos] = p.nConstraints + (u32)s;
            memcpy(&c.val[(size_t)pos * 32], oneLe, 32);
        }
        columnPieces(c.colPtr.data(), p.nVars, (u32)m, pieces);
    }
}

namespace {

// ---- section 4: one record per (matrix, row, wire), row first, A before B, wire ascending; repeated wires added, sums of 0 left out ----
struct CoefTerm { u32 wire; Fr v; };
// the merged terms of one combination, wire ascending
void mergedRow(const R1csMatrix& m, u32 k, std::vector<CoefTerm>& out) {
    out.clear();
    for (u32 q = m.rowPtr[k]; q < m.rowPtr[k + 1]; q++) out.push_back({m.sig[q], frFromPlain(&m.val[(size_t)q * 32])});
    std::stable_sort(out.begin(), out.end(), [](const CoefTerm& a, const CoefTerm& b) { return a.wire < b.wire; });
    size_t w = 0;
    for (size_t i = 0; i < out.size();) {
        Fr sum = out[i].v;
        size_t j = i + 1;
        for (; j < out.size() && out[j].wire == out[i].wire; j++) sum = frAdd(sum, out[j].v);
        if (!frIsZero(sum)) out[w++] = {out[i].wire, sum};
        i = j;
    }
    out.resize(w);
}
// per piece of 4096 rows: the records of the constraint rows (the public rows add nPublic + 1 at the end)
constexpr u64 COEF_GRAIN = 4096;
}  // namespace
u64 countCoefs(const R1cs& cs, std::vector<u64>& perPiece) {
    const u64 rows = cs.hdr.nConstraints;
    perPiece.assign((size_t)((rows + COEF_GRAIN - 1) / COEF_GRAIN), 0);
    parallelFor(rows, COEF_GRAIN, [&](u64 lo, u64 hi) {
        std::vector<CoefTerm> t;
        u64 n = 0;
        for (u64 k = lo; k < hi; k++)
            for (int m = 0; m < 2; m++) { mergedRow(cs.m[m], (u32)k, t); n += t.size(); }
        perPiece[(size_t)(lo / COEF_GRAIN)] = n;
    });
    u64 total = 0;
    for (u64 n : perPiece) total += n;
    return total;
}
namespace {
void putCoef(uint8_t* o, u32 m, u32 row, u32 wire, const Fr& v) {
    memcpy(o, &m, 4); memcpy(o + 4, &row, 4); memcpy(o + 8, &wire, 4);
    // coef * 2^512 mod r as a plain integer: twice "to the reference's Montgomery form", the first result read as plain again
    u32 w[8];
    to_mont256(w, v);
    to_mont256(w, cond_sub_q(from_normal<FrParams>(w)));
    memcpy(o + 12, w, 32);
}
void fillCoefs(const R1cs& cs, const Plan& p, const std::vector<u64>& perPiece, uint8_t* out) {
    std::vector<u64> first(perPiece.size() + 1, 0);
    for (size_t i = 0; i < perPiece.size(); i++) first[i + 1] = first[i] + perPiece[i];
    parallelFor(cs.hdr.nConstraints, COEF_GRAIN, [&](u64 lo, u64 hi) {
        std::vector<CoefTerm> t;
        uint8_t* o = out + first[(size_t)(lo / COEF_GRAIN)] * 44;
        for (u64 k = lo; k < hi; k++)
            for (u32 m = 0; m < 2; m++) {
                mergedRow(cs.m[m], (u32)k, t);
                for (const CoefTerm& c : t) { putCoef(o, m, (u32)k, c.wire, c.v); o += 44; }
            }
    });
    uint8_t* o = out + first.back() * 44;
    for (u32 s = 0; s <= p.nPublic; s++, o += 44) putCoef(o, 0, p.nConstraints + s, s, fp_one<FrParams>());
}

}  // namespace
void writeCoefs(const R1cs& cs, const Plan& p, const std::vector<u64>& perPiece, uint8_t* out) { fillCoefs(cs, p, perPiece, out); }

// ---- file layout ----
u64 Layout::offsetOf(u32 id) const {
    u64 at = 12;
    for (auto& s : sections) { at += 12; if (s.first == id) return at; at += s.second; }
    throw SetupError("internal: no section " + std::to_string(id));
}
Layout makeLayout(const Plan& p, u64 nCoefs) {
    if (nCoefs > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 records in section 4");
    Layout l;
    l.nCoefs = nCoefs;
    const u64 M = p.nVars, N = p.N, pub = (u64)p.nPublic + 1;
    const u64 hdr = 4 + 32 + 4 + 32 + 12 + (p.ultra ? 12 : 0) + 64 + 64 + 128 + 128 + (p.ultra ? 192 : 0) + 192;
    l.sections = {{1, 4}, {2, hdr}, {3, 64 * pub}, {4, 4 + 44 * nCoefs}, {5, 64 * M}, {6, 64 * M}, {7, 128 * M}};
    if (p.ultra) {
        const u64 n1 = p.roundSignals.size(), n2 = p.finalSignals.size();
        l.sections.insert(l.sections.end(), {{8, 64 * n1}, {9, 64 * n2}, {10, 4 * n1}, {11, 4 * n2}, {12, 64 * N}, {13, 0}});
    } else {
        l.sections.insert(l.sections.end(), {{8, 64 * (M - pub)}, {9, 64 * N}, {10, 0}});
    }
    l.total = 12;
    for (auto& s : l.sections) l.total += 12 + s.second;
    return l;
}

namespace {

// ---- verification key ----
std::string fqDecimal(const uint8_t* mont) {
    u32 w[8], plain[8];
    memcpy(w, mont, 32);
    to_normal(plain, from_mont256<FqParams>(w));
    return toDecimal((const uint8_t*)plain);
}
std::string jsonG1(const uint8_t* rec) {
    if (allZero(rec, 64)) return "[\"0\", \"1\", \"0\"]";
    return "[\"" + fqDecimal(rec) + "\", \"" + fqDecimal(rec + 32) + "\", \"1\"]";
}
std::string jsonG2(const uint8_t* rec) {
    return "[[\"" + fqDecimal(rec) + "\", \"" + fqDecimal(rec + 32) + "\"], [\"" + fqDecimal(rec + 64) + "\", \"" + fqDecimal(rec + 96) +
           "\"], [\"1\", \"0\"]]";
}
std::string vkeyJson(const Plan& p, const HeaderPoints& hp, const uint8_t* ic) {
    std::string s = "{\n";
    s += std::string(" \"protocol\": \"") + (p.ultra ? "ultragroth" : "groth16") + "\",\n \"curve\": \"bn128\",\n";
    s += " \"nPublic\": " + std::to_string(p.ultra ? p.nPublic - 1 : p.nPublic) + ",\n";
    s += " \"vk_alpha_1\": " + jsonG1(hp.g1[0]) + ",\n \"vk_beta_2\": " + jsonG2(hp.g2[0]) + ",\n \"vk_gamma_2\": " + jsonG2(hp.g2[1]) + ",\n";
    if (p.ultra) s += " \"vk_delta_c1_2\": " + jsonG2(hp.g2[2]) + ",\n \"vk_delta_c2_2\": " + jsonG2(hp.g2[3]) + ",\n";
    else s += " \"vk_delta_2\": " + jsonG2(hp.g2[3]) + ",\n";
    s += " \"IC\": [";
    bool first = true;
    for (u32 i = 0; i <= p.nPublic; i++) {
        if (p.ultra && i == p.randIndx) continue;
        s += (first ? "\n  " : ",\n  ") + jsonG1(ic + (size_t)i * 64);
        first = false;
    }
    s += "\n ]";
    if (p.ultra) s += ",\n \"IC_rand\": " + jsonG1(ic + (size_t)p.randIndx * 64);
    return s + "\n}\n";
}

}  // namespace

void inttTwiddles(int logN, std::vector<u32>& tw) {
    const u64 half = logN ? 1ull << (logN - 1) : 0;
    tw.assign((size_t)half * 8, 0);
    const Fr wi = frInv(rootOfUnity(logN));
    parallelFor(half, 4096, [&](u64 lo, u64 hi) {
        Fr w = fp_one<FrParams>(), b = wi;         // omega^(-lo) by square and multiply, then a running product
        for (u64 e = lo; e; e >>= 1) { if (e & 1) w = frMul(w, b); b = frMul(b, b); }
        for (u64 j = lo; j < hi; j++) {
            uint8_t le[32];
            u32 mag[8];
            frToPlain(le, w);
            if (coefMagnitude(le, mag)) mag[7] |= 0x80000000u;
            memcpy(&tw[(size_t)j * 8], mag, 32);
            w = frMul(w, wi);
        }
    });
}

void inttScale(int logN, u32 folded[8]) {       // N * (r - 1) / N = -1 mod r
    for (int i = 0; i < 8; i++) folded[i] = FrParams::q32[i];
    folded[0] -= 1;
    for (int s = 0; s < logN; s++)
        for (int i = 0; i < 8; i++) folded[i] = (folded[i] >> 1) | (i + 1 < 8 ? folded[i + 1] << 31 : 0u);
    folded[7] |= 0x80000000u;
}

bool inttTrivial(bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out) {
    if (logN) return false;
    const size_t rec = g2 ? 128 : 64;
    for (int v = 0; v < nVec; v++) {
        if (nGiven) memcpy(out[v], in[v], rec);
        else memset(out[v], 0, rec);
    }
    return true;
}

// an upper bound of the JSON's length: 78 characters per coordinate leave room for any value below 2^256 and the punctuation
u64 vkeyBound(const Plan& p) { return 512 + 84ull * (2 + 4 * 4 + 2 * ((u64)p.nPublic + 2)) + 16ull * (p.nPublic + 8); }

void copyErr(char* dst, unsigned long long max, const char* msg) {
    if (!dst || !max) return;
    strncpy(dst, msg, max);
    dst[max - 1] = 0;
}

std::string underPrefix(const PrefixRule& rule, const std::string& m) {
    for (const char* k : rule.keep)
        if (k && m.rfind(k, 0) == 0) return m;
    return rule.put + (rule.dropSetup && m.rfind("setup: ", 0) == 0 ? m.substr(7) : m);
}

void copyVkey(const std::string& vkey, char* dst, u64 capacity, uint64_t* bytes) {
    if (bytes) *bytes = vkey.size();
    if (!dst) return;
    if (capacity < vkey.size() + 1) throw SetupError("the verification-key buffer is too small: " + std::to_string(vkey.size() + 1) + " bytes are needed");
    memcpy(dst, vkey.c_str(), vkey.size() + 1);
}

void drawNonZeroScalar(uint8_t le[32]) {
    do {
        randomBytes(le, 32);
        le[31] &= 0x3f;
    } while (allZero(le, 32) || !belowR(le));
}

// ---- the ratio test: what both backends share ----
void drawWeights128(std::vector<uint8_t>& out, u64 n) {
    out.assign((size_t)n * 16, 0);
    parallelFor(n, 1 << 16, [&](u64 lo, u64 hi) { randomBytes(&out[(size_t)lo * 16], (size_t)(hi - lo) * 16); });
}

const pr::FinalExpConsts& ratioConsts() {
    static const pr::FinalExpConsts c = pr::final_exp_consts();
    return c;
}

void ratioG2Words(const uint8_t* q, u32 out[RATIO_Q2_WORDS]) {
    u32 rec[32], gen[32];
    memcpy(rec, q, 128);
    generatorWords(true, gen);
    const pr::G2A pt = pr::g2_from_record(rec);
    const Fq c[8] = {pt.x.a.v, pt.x.b.v, pt.y.a.v, pt.y.b.v, cond_sub_q(unpack256<FqParams>(gen)), cond_sub_q(unpack256<FqParams>(gen + 8)),
                     cond_sub_q(unpack256<FqParams>(gen + 16)), cond_sub_q(unpack256<FqParams>(gen + 24))};
    for (int i = 0; i < 8; i++) pr::fq_store(out + i * NL, c[i]);
}

std::vector<u64> RatioOut::listed(u64 n, u64 maxListed) const {
    std::vector<u64> v;
    for (size_t b = 0; b < resolved.size() && v.size() < maxListed; b++)
        for (u64 k = 0; k < RATIO_BLOCK && resolved[b] * RATIO_BLOCK + k < n && v.size() < maxListed; k++)
            if (recordBad[b * RATIO_BLOCK + k]) v.push_back(resolved[b] * RATIO_BLOCK + k);
    return v;
}

void ratioLevels(const uint8_t* x, const uint8_t* y, u64 n, u64 maxBlocks, RatioOut& out, const RatioSums& sums, const RatioJudge& judge) {
    out = RatioOut();
    if (!maxBlocks) maxBlocks = RATIO_MAX_BLOCKS;
    const u64 blocks = (n + RATIO_BLOCK - 1) / RATIO_BLOCK;
    out.blocks = blocks;
    if (!n) return;
    // block level
    out.blockBad.assign((size_t)blocks, 0);
    {
        std::vector<uint8_t> w, sx((size_t)blocks * 64), sy((size_t)blocks * 64);
        drawWeights128(w, n);
        sums(w.data(), sx.data(), sy.data(), &out.ms[0]);
        judge(sx.data(), sy.data(), blocks, out.blockBad.data(), &out.ms[1]);
    }
    for (u64 j = 0; j < blocks; j++) {
        if (!out.blockBad[(size_t)j]) continue;
        out.badBlocks++;
        if (out.resolved.size() < maxBlocks) out.resolved.push_back(j);
    }
    out.resolvedBlocks = out.resolved.size();
    out.exact = out.resolvedBlocks == out.badBlocks;
    if (out.resolved.empty()) return;
    // record level: the records of the resolved blocks side by side (a short last block is padded with infinity pairs, which hold)
    const size_t m = out.resolved.size() * (size_t)RATIO_BLOCK;
    std::vector<uint8_t> gx(m * 64, 0), gy(m * 64, 0);
    for (size_t b = 0; b < out.resolved.size(); b++) {
        const u64 first = out.resolved[b] * RATIO_BLOCK, count = std::min(RATIO_BLOCK, n - first);
        memcpy(&gx[b * RATIO_BLOCK * 64], x + first * 64, (size_t)count * 64);
        memcpy(&gy[b * RATIO_BLOCK * 64], y + first * 64, (size_t)count * 64);
    }
    out.recordBad.assign(m, 0);
    double ms = 0;
    judge(gx.data(), gy.data(), m, out.recordBad.data(), &ms);
    out.ms[1] += ms;
    for (uint8_t b : out.recordBad) out.badRecords += b;
}

Backend& backendFor(int device, std::unique_ptr<Backend>& owned) {
    if (device < 0) return hostBackend();
    if (!deviceBackendFactory) throw SetupError("this program has no device path: use device = -1 (host threads)");
    owned.reset(deviceBackendFactory(device));
    return *owned;
}

void loadCircuit(const void* r1cs, u64 size, std::unique_ptr<BinFile>& f, R1csHeader& h) {
    f = openBinFile(r1cs, size, "r1cs", "setup: ", "null r1cs buffer");
    h = loadR1csHeader(*f);
}

void writeContainer(uint8_t* zkey, const Layout& lay) {
    uint8_t* o = zkey;
    putBytes(o, "zkey", 4); put32(o, 1); put32(o, (u32)lay.sections.size());
    for (auto& s : lay.sections) { put32(o, s.first); put64(o, s.second); o += s.second; }
}

void finishKey(const R1cs& cs, const Plan& p, const Layout& lay, const std::vector<u64>& perPiece, const HeaderPoints& hp,
               const std::vector<uint8_t>& krec, uint8_t* zkey, std::string* vkey, bool cPointsDone) {
    const u64 M = p.nVars, pub = (u64)p.nPublic + 1;
    uint8_t* o = zkey + lay.offsetOf(1);
    put32(o, p.ultra ? 1337 : 1);
    o = zkey + lay.offsetOf(2);
    put32(o, 32); putBytes(o, BN254_Q_LE, 32); put32(o, 32); putBytes(o, BN254_R_BYTES, 32);
    put32(o, p.nVars); put32(o, p.nPublic); put32(o, p.N);
    if (p.ultra) { put32(o, (u32)p.roundSignals.size()); put32(o, (u32)p.finalSignals.size()); put32(o, p.randIndx); }
    putBytes(o, hp.g1[0], 64); putBytes(o, hp.g1[1], 64); putBytes(o, hp.g2[0], 128); putBytes(o, hp.g2[1], 128);
    if (p.ultra) { putBytes(o, hp.g1[2], 64); putBytes(o, hp.g2[2], 128); }
    putBytes(o, hp.g1[3], 64); putBytes(o, hp.g2[3], 128);
    memcpy(zkey + lay.offsetOf(3), krec.data(), pub * 64);
    o = zkey + lay.offsetOf(4);
    put32(o, (u32)lay.nCoefs);
    fillCoefs(cs, p, perPiece, o);
    if (p.ultra) {
        if (!cPointsDone) {
            uint8_t* c1 = zkey + lay.offsetOf(8);
            uint8_t* c2 = zkey + lay.offsetOf(9);
            for (size_t i = 0; i < p.roundSignals.size(); i++) memcpy(c1 + i * 64, &krec[(size_t)p.roundSignals[i] * 64], 64);
            for (size_t i = 0; i < p.finalSignals.size(); i++) memcpy(c2 + i * 64, &krec[(size_t)p.finalSignals[i] * 64], 64);
        }
        if (!p.roundSignals.empty()) memcpy(zkey + lay.offsetOf(10), p.roundSignals.data(), 4 * p.roundSignals.size());
        if (!p.finalSignals.empty()) memcpy(zkey + lay.offsetOf(11), p.finalSignals.data(), 4 * p.finalSignals.size());
    } else if (M > pub && !cPointsDone) {
        memcpy(zkey + lay.offsetOf(8), &krec[pub * 64], (M - pub) * 64);
    }
    if (vkey) *vkey = vkeyJson(p, hp, krec.data());
}

Backend& hostBackend() {
    static HostBackend b;
    return b;
}

void generatorWords(bool g2, u32* out) {
    if (g2) {
        Fq2 x, y;
        Gen<Fq2>::generator(x, y);
        pack256(out, x.a); pack256(out + 8, x.b); pack256(out + 16, y.a); pack256(out + 24, y.b);
    } else {
        Fq x, y;
        Gen<Fq>::generator(x, y);
        pack256(out, x); pack256(out + 8, y);
    }
}

// the whole setup; returns the zkey's size, writes the JSON to vkey
u64 run(const ug_setup_options* opt, const void* r1cs, u64 size, int device, uint8_t* zkey, u64 zkeyCap, std::string* vkey, double ms[PHASES],
        bool sizeOnly, u64* vkeyMax) {
    for (int i = 0; i < PHASES; i++) ms[i] = 0;
    PhaseClock clock(ms);
    std::unique_ptr<BinFile> f;
    R1cs cs;
    loadCircuit(r1cs, size, f, cs.hdr);
    Plan p;
    makePlan(opt, cs.hdr, p);                    // (every check of the options before the constraints are walked)
    loadR1cs(*f, cs);
    std::vector<u64> perPiece;
    const Layout lay = makeLayout(p, (u64)p.nPublic + 1 + countCoefs(cs, perPiece));
    if (vkeyMax) *vkeyMax = vkeyBound(p);
    if (sizeOnly) return lay.total;
    if (!zkey) throw SetupError("null zkey buffer");
    if (zkeyCap < lay.total) throw SetupError("the zkey buffer is too small: " + std::to_string(lay.total) + " bytes are needed");
    std::unique_ptr<Backend> owned;
    Backend& be = backendFor(device, owned);

    ColMatrix cm[3];
    std::vector<Piece> pieces;
    buildColumns(cs, p, cm, pieces);
    clock.lap(0);

    writeContainer(zkey, lay);
    const u64 M = p.nVars;
    std::vector<uint8_t> krec(M * 64);
    be.points(p, cm, pieces, zkey + lay.offsetOf(5), zkey + lay.offsetOf(6), zkey + lay.offsetOf(7), krec.data(),
              zkey + lay.offsetOf(p.ultra ? 12 : 9), ms);
    clock.restart();
    // the eight header points, on host threads whatever the backend
    HeaderPoints hp;
    {
        uint8_t sc[4][32];
        memcpy(sc[0], p.opt.alpha, 32); memcpy(sc[1], p.opt.beta, 32); memcpy(sc[2], p.opt.delta_round, 32); memcpy(sc[3], p.opt.delta_final, 32);
        if (!p.ultra) memset(sc[2], 0, 32);
        hostBackend().generatorMul(false, sc[0], 4, 0, hp.g1[0], nullptr);
        memcpy(sc[0], p.opt.beta, 32); memcpy(sc[1], p.opt.gamma, 32);
        hostBackend().generatorMul(true, sc[0], 4, 0, hp.g2[0], nullptr);
    }
    finishKey(cs, p, lay, perPiece, hp, krec, zkey, vkey);
    clock.lap(5);
    return lay.total;
}

}  // namespace setup
}  // namespace ughost

// =====================================================================================================================
using namespace ughost::setup;

extern "C" {

int ug_setup_draw_trapdoor(ug_setup_options* opt, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (!opt) throw SetupError("null options");
        for (uint8_t* d : {opt->tau, opt->alpha, opt->beta, opt->gamma, opt->delta_round, opt->delta_final}) drawNonZeroScalar(d);
    });
}

int ug_setup_size(const ug_setup_options* opt, const void* r1cs, uint64_t r1cs_size, uint64_t* zkey_bytes, uint64_t* vkey_bytes_max,
                  char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        double ms[PHASES];
        u64 vmax = 0;
        const u64 total = run(opt, r1cs, r1cs_size, -1, nullptr, 0, nullptr, ms, true, &vmax);
        if (zkey_bytes) *zkey_bytes = total;
        if (vkey_bytes_max) *vkey_bytes_max = vmax;
    });
}

int ug_setup_run(const ug_setup_options* opt, const void* r1cs, uint64_t r1cs_size, int device, void* zkey, uint64_t zkey_capacity,
                 uint64_t* zkey_bytes, char* vkey_json, uint64_t vkey_capacity, uint64_t* vkey_bytes, double* phase_ms, char* error_msg,
                 unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        double ms[PHASES];
        std::string vkey;
        const u64 total = run(opt, r1cs, r1cs_size, device, (uint8_t*)zkey, zkey_capacity, &vkey, ms, false, nullptr);
        if (zkey_bytes) *zkey_bytes = total;
        copyVkey(vkey, vkey_json, vkey_capacity, vkey_bytes);
        if (phase_ms) for (int i = 0; i < PHASES; i++) phase_ms[i] = ms[i];
    });
}

int ug_generator_mul(int device, int g2, const void* scalars, uint64_t n, int window, void* out, double* kernel_ms, char* error_msg,
                     unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (n && (!scalars || !out)) throw SetupError("null buffer");
        if (window && (window < WINDOW_MIN || window > WINDOW_MAX))
            throw SetupError("window " + std::to_string(window) + " is outside " + std::to_string(WINDOW_MIN) + " .. " + std::to_string(WINDOW_MAX));
        checkScalars((const uint8_t*)scalars, n);
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
        if (!n) return;
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).generatorMul(g2 != 0, (const uint8_t*)scalars, n, window, (uint8_t*)out, kernel_ms);
    });
}

int ug_lagrange_at(int device, int log_n, const void* x, int coset, void* out, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (!x || !out) throw SetupError("null buffer");
        if (log_n < 1 || log_n > MAX_LOG_DOMAIN) throw SetupError("log_n " + std::to_string(log_n) + " is outside 1 .. " + std::to_string(MAX_LOG_DOMAIN));
        if (!belowR((const uint8_t*)x)) throw SetupError("x is not below the field modulus");
        Fr v = frFromPlain((const uint8_t*)x);
        if (coset) v = frMul(v, frInv(rootOfUnity(log_n + 1)));
        const Fr vN = frPow2k(v, log_n);
        if (frIsOne(vN)) throw SetupError("x lies in the evaluation domain");
        const Fr scale = frMul(frSub(vN, ug::fp_one<ug::FrParams>()), frInv(frSmall(1u << log_n)));
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).lagrange(log_n, v, scale, rootOfUnity(log_n), (uint8_t*)out);
    });
}

}  // extern "C"
