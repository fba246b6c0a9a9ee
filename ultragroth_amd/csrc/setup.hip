// setup.hip -- the development setup's device path (include/ultragroth_hip.h: ug_setup_run with device >= 0): the kernels of a
// TEST proving key made from an .r1cs and a known trapdoor, and the backend that queues them (setup_host.hpp: Backend).
//
//   lagrange_kernel        all N values L_k(x) of one point x: a lane takes 8 consecutive k, omega^k from one power and a running
//                          product, one inversion for the eight (Montgomery's trick)
//   column_pieces_kernel   the transposed sparse product of a LONG column: one workgroup per piece of 4 096 terms
//   wire_sums_kernel       one lane per wire: u, v, w over its columns of A, B, C (short columns term by term, long ones from
//                          their pieces' partial sums), then K_s and the division by gamma or a delta
//   gen_table_*_kernel     window tables of a generator: table j holds d * 2^(c j) * G for the digits d = 1 .. 2^(c-1)
//   compact_kernel         the non-zero scalars' indices, and the all-zero record of every zero scalar
//   gen_mul_kernel         the hot path: scalar * G for millions of independent scalars, signed c-bit digits, ceil(255 / c) mixed
//                          additions from the tables, KPL results of a lane converted to affine with one shared inversion
// This is a translation unit of its own: no kernel of the prover or the verifier is compiled differently because it exists.
// Plain C++ and vector stores only. DESIGN.md section 5.8 has the registers, the column-split rule and the window choice.
#include "setup_dev.hpp"
#include "stream_timer.hpp"
#include "setup_host.hpp"

#include <memory>

namespace ug {

// setup_points.hip
void device_points_combine(hipStream_t stream, StreamTimer& timer, bool g2, u64 nCols, const u32* colPtr, const u32* index,
                           const uint8_t* coefs, const ughost::setup::PointSegs& pts, uint8_t* out, double* ms);
void device_points_scale(hipStream_t stream, StreamTimer& timer, const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out, double* ms);
void device_points_scale_segments(hipStream_t stream, StreamTimer& timer, const ughost::setup::ScaleSeg* segs, int n, double* ms);
void device_points_ratio_sums(hipStream_t stream, StreamTimer& timer, const uint8_t* x, const uint8_t* y, u64 n, const uint8_t* weights,
                              uint8_t* sumX, uint8_t* sumY, double* ms);
// pairing.hip
void ratio_judge_device(hipStream_t stream, const pr::FinalExpConsts& kc, const uint8_t* x, const uint8_t* y, u64 n, const u32* q2, uint8_t* wrong,
                        double* kernel_ms);
// ptau_prepare.hip
void device_points_intt(hipStream_t stream, StreamTimer& timer, bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven,
                        uint8_t* const* out, double* ms);

namespace {

using ughost::setup::Piece;
using ughost::setup::SPLIT_PIECE;
using ughost::setup::SPLIT_THRESHOLD;
using namespace sdev;

struct FrWords { u32 w[8]; };                   // a canonical Fr value in device form, packed: kernel arguments by value
__device__ __forceinline__ Fr fr_arg(const FrWords& a) { return unpack256<FrParams>(a.w); }

// ---- plain <-> device form, in place ----
__global__ void fr_from_plain_kernel(u32* v, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    load8(w, v + i * 8);
    st_packed(v + i * 8, cond_sub_q(from_normal<FrParams>(w)));
}
__global__ void fr_to_plain_kernel(u32* v, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    to_normal(w, ld_packed<FrParams>(v + i * 8));
    store8(v + i * 8, w);
}

// ---- Lagrange evaluation ----
// out[k] = scale * omega^k / (x - omega^k), canonical device form, for k < n. x is outside the domain (the host refuses
// tau^(2N) = 1), so no denominator is 0. A lane's eight denominators are multiplied up, inverted once and peeled off again
// from the top; omega^k is walked back down with 1 / omega instead of being kept.
constexpr int LAG_K = 8;
struct LagArgs { FrWords x, scale, omega, omega_inv; };
__global__ __launch_bounds__(256) void lagrange_kernel(u32* out, u32 n, LagArgs a) {
    const u64 k0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LAG_K;
    if (k0 >= n) return;
    const int cnt = n - k0 < (u64)LAG_K ? (int)(n - k0) : LAG_K;       // (n = 2: K > N)
    const Fr x = fr_arg(a.x), om = fr_arg(a.omega);
    Fr w = fp_one<FrParams>();                                         // omega^k0, every value below 2q
    {
        Fr b = om;
        for (u64 e = k0; e; e >>= 1) {
            if (e & 1) w = mul(w, b);
            b = sqr(b);
        }
    }
    // (all eight are computed whatever cnt is: past n the powers of omega wrap round the domain, every denominator is still
    // non-zero, and only the stores are guarded)
    Fr pre[LAG_K];
    Fr run = fp_one<FrParams>();
    Static<0, LAG_K>::up([&](auto i) {
        pre[i] = run;
        run = mul(run, sub<2>(x, w));                                  // x - w + 2q < 3q
        w = mul(w, om);
    });
    Fr irun = inv(run);
    const Fr scale = fr_arg(a.scale), om_inv = fr_arg(a.omega_inv);
    Static<0, LAG_K>::down([&](auto i) {
        w = mul(w, om_inv);                                            // omega^(k0 + i)
        const Fr id = mul(irun, pre[i]);                               // 1 / (x - omega^(k0 + i))
        irun = mul(irun, sub<2>(x, w));
        if (i < cnt) st_packed(out + (k0 + i) * 8, cond_sub_q(mul(mul(scale, w), id)));
    });
}

// ---- transposed sparse products ----
struct ColDev {
    const u32* col_ptr[3]; const u32* row[3]; const u32* val[3];       // val: coefficients in device form, column order
};
// sum of coef * lag[row] over the terms [s, e), step `step`: below 2.01 q, strict (the contraction of matvec_row)
__device__ __forceinline__ Fr column_sum(const u32* row, const u32* val, const u32* lag, u32 s, u32 e, u32 step) {
    Fr acc = fp_zero<FrParams>();
    u32 since = 0;
    for (u64 p = s; p < e; p += step) {         // (64 bits: p + step may pass 2^32 in a matrix of nearly 2^32 terms)
        acc = add(acc, mul(ld_packed<FrParams>(val + (size_t)p * 8), ld_packed<FrParams>(lag + (size_t)row[p] * 8)));
        if (++since == 24) { acc = contract(acc); since = 0; }
    }
    return contract(acc);
}
// One workgroup of 256 lanes per piece: lane t takes the terms first + t, + 256, ...; the 256 partial sums are added in LDS.
// partial[piece]: canonical device form.
__global__ __launch_bounds__(256) void column_pieces_kernel(ColDev c, const Piece* pieces, u32 n_pieces, const u32* lag, u32* partial) {
    __shared__ u32 sh[NL][256];
    const u32 t = threadIdx.x;
    if (blockIdx.x >= n_pieces) return;
    const Piece pc = pieces[blockIdx.x];
    Fr acc = column_sum(c.row[pc.m], c.val[pc.m], lag, pc.first + t, pc.end, 256);
#pragma unroll
    for (int i = 0; i < NL; i++) sh[i][t] = acc.l[i];
    for (u32 off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (t < off) {
            Fr o;
#pragma unroll
            for (int i = 0; i < NL; i++) o.l[i] = sh[i][t + off];
            acc = contract(add(acc, o));
#pragma unroll
            for (int i = 0; i < NL; i++) sh[i][t] = acc.l[i];
        }
    }
    if (t == 0) st_packed(partial + (size_t)blockIdx.x * 8, canon(acc));
}
struct WireArgs {
    FrWords alpha, beta, inv[3];
    u32 n_wires;
    u32 piece_first[4];                          // the pieces of matrix m are [piece_first[m], piece_first[m + 1]), wire ascending
};
// One lane per wire. A column of more than SPLIT_THRESHOLD terms is the sum of its pieces' partial sums, found by a binary
// search of the (few) pieces; every other column is walked term by term. Scalars out: plain canonical integers.
__global__ __launch_bounds__(256) void wire_sums_kernel(ColDev c, const Piece* pieces, const u32* partial, const u32* lag,
                                                        const uint8_t* cls, WireArgs a, u32* sa, u32* sb, u32* sk) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_wires) return;
    Fr uvw[3];
#pragma unroll
    for (int m = 0; m < 3; m++) {                // (unrolled: uvw stays in registers)
        const u32 lo = c.col_ptr[m][s], hi = c.col_ptr[m][s + 1];
        if (hi - lo <= SPLIT_THRESHOLD) {
            uvw[m] = column_sum(c.row[m], c.val[m], lag, lo, hi, 1);
        } else {
            u32 l = a.piece_first[m], r = a.piece_first[m + 1];
            while (l < r) {                      // the first piece of wire s
                const u32 mid = l + (r - l) / 2;
                if (pieces[mid].wire < s) l = mid + 1; else r = mid;
            }
            Fr acc = fp_zero<FrParams>();
            for (u32 p = l; p < a.piece_first[m + 1] && pieces[p].wire == s; p++)
                acc = contract(add(acc, ld_packed<FrParams>(partial + (size_t)p * 8)));
            uvw[m] = acc;
        }
    }
    // K = beta u + alpha v + w: below 2q + 2q + 2.01 q
    const Fr k = add(add(mul(fr_arg(a.beta), uvw[0]), mul(fr_arg(a.alpha), uvw[1])), uvw[2]);
    const u32 cl = cls[s];
    const Fr ks = mul(k, fr_arg(cl == 0 ? a.inv[0] : cl == 1 ? a.inv[1] : a.inv[2]));
    u32 w[8];
    to_normal(w, uvw[0]); store8(sa + (size_t)s * 8, w);
    to_normal(w, uvw[1]); store8(sb + (size_t)s * 8, w);
    to_normal(w, ks); store8(sk + (size_t)s * 8, w);
}
// the H scalars: lag (device form) * scale -> plain
__global__ void h_scalars_kernel(u32* out, const u32* lag, u64 n, FrWords scale) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    to_normal(w, mul(ld_packed<FrParams>(lag + i * 8), fr_arg(scale)));
    store8(out + i * 8, w);
}

// ---- window tables of a generator ----
// table: tables * half records, affine, canonical device form; record (j, d - 1) = d * 2^(c j) * G, d = 1 .. half = 2^(c-1).
// First the bases 2^(c j) * G, one lane per table (the walk of synth_points_kernel's table, on the device): c j doublings.
template <class Cfg>
__global__ __launch_bounds__(64) void gen_table_bases_kernel(u32* table, const u32* generator, int c, int tables, u32 half) {
    typedef typename Cfg::F F;
    const int j = threadIdx.x;
    if (blockIdx.x || j >= tables) return;
    F x, y;
    Cfg::load(generator, x, y);
    if (j) {
        XYZZ<F> p = xyzz_dbl_affine(x, y);
        for (int d = 1; d < c * j; d++) p = xyzz_dbl(p);
        xyzz_to_affine(x, y, p);
    }
    Cfg::store_packed(table + (size_t)j * half * Cfg::AFF_WORDS, x, y);
}
// Then every other record, one lane each: d * base by double-and-add over the bits of d (at most 15 doublings and as many
// mixed additions), and its own inversion.
template <class Cfg>
__global__ __launch_bounds__(128) void gen_table_fill_kernel(u32* table, int tables, u32 half) {
    typedef typename Cfg::F F;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (half < 2 || t >= (u64)tables * (half - 1)) return;
    const u32 j = (u32)(t / (half - 1)), d = 2 + (u32)(t % (half - 1));
    F x, y;
    Cfg::load(table + (size_t)j * half * Cfg::AFF_WORDS, x, y);
    XYZZ<F> p = xyzz_from_affine(x, y);
    for (int b = 30 - __clz(d); b >= 0; b--) {
        p = xyzz_dbl(p);
        if ((d >> b) & 1) p = xyzz_madd(p, x, y);
    }
    F ax, ay;
    xyzz_to_affine(ax, ay, p);
    Cfg::store_packed(table + ((size_t)j * half + d - 1) * Cfg::AFF_WORDS, ax, ay);
}

// ---- zero scalars ----
// idx[0 .. *count) = the indices of the non-zero scalars (in no particular order: every result goes to its own index), and
// the all-zero record at every zero scalar's place in out1 (64-byte records) and out2 (128-byte records), either may be null.
// One atomic per wave.
__global__ __launch_bounds__(256) void compact_kernel(const u32* scalars, u64 n, u32* idx, u32* count, u32* out1, u32* out2) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool nz = false;
    if (i < n) {
        u32 w[8];
        load8(w, scalars + i * 8);
        nz = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;
        if (!nz) {
            if (out1) zero_record<16>(out1 + i * 16);
            if (out2) zero_record<32>(out2 + i * 32);
        }
    }
    const unsigned long long m = __ballot(nz);
    if (!m) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    u32 base = 0;
    if (lane == leader) base = atomicAdd(count, (u32)__popcll(m));
    base = __shfl(base, leader, 64);
    if (nz) idx[base + __popcll(m & ((1ull << lane) - 1))] = (u32)i;
}

// ---- the fixed-base multiplication ----
// One scalar (plain, below r < 2^254) through `tables` signed digits of c bits: digit = raw + carry; above 2^(c-1) it becomes
// digit - 2^c with a carry into the next window. tables * c >= 255, so the top window's raw digit is below 2^(c-1) and its
// sum with the carry never above it: no carry leaves the top window. A negative digit takes the table's record with y negated.
// xyzz_madd handles every exceptional case (ec.hpp: infinity, the doubling when the table's point equals the accumulator, and
// the sum that is infinity), so the one scalar per width whose last addition is a doubling is right as well.
// The scalar's words are shifted down by c after every window, so that no register array is indexed by a run-time value.
template <class Cfg>
__device__ __forceinline__ XYZZ<typename Cfg::F> gen_mul_one(const u32* scalar, const u32* table, int c, int tables, u32 half) {
    typedef typename Cfg::F F;
    u32 s[8];
    load8(s, scalar);
    XYZZ<F> acc = xyzz_inf<F>();
    const u32 mask = (1u << c) - 1;
    u32 carry = 0;
#pragma unroll 1
    for (int j = 0; j < tables; j++) {
        u32 d = (s[0] & mask) + carry;
#pragma unroll
        for (int i = 0; i < 7; i++) s[i] = (s[i] >> c) | (s[i + 1] << (32 - c));
        s[7] >>= c;
        carry = d > half ? 1u : 0u;
        if (carry) d = (mask + 1) - d;
        if (d) {
            F x, y;
            Cfg::load(table + ((size_t)j * half + d - 1) * Cfg::AFF_WORDS, x, y);
            if (carry) y = neg<1>(y);            // q - y: y is canonical
            acc = xyzz_madd(acc, x, y);
        }
    }
    return acc;
}
// A lane takes KPL scalars -- idx[t] for t < *count when idx is given, else t < n -- one after the other and converts the
// KPL results with one shared inversion. A non-zero scalar below r never gives infinity; one that does is written as zeros.
template <class Cfg>
__global__ __launch_bounds__(Cfg::BLOCK) void gen_mul_kernel(const u32* scalars, const u32* idx, const u32* count, u64 n, const u32* table,
                                                             int c, int tables, u32 half, u32* out) {
    typedef typename Cfg::F F;
    constexpr int K = Cfg::KPL;
    if (idx) n = *count;
    const u64 t0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * K;
    if (t0 >= n) return;
    XYZZ<F> res[K];
    u64 at[K];
    F pre[K];
    F run = field_one((F*)0);
    Static<0, K>::up([&](auto k) {
        if (t0 + k < n) {
            at[k] = idx ? (u64)idx[t0 + k] : t0 + k;
            res[k] = gen_mul_one<Cfg>(scalars + at[k] * 8, table, c, tables, half);
        } else {
            at[k] = ~(u64)0;
            res[k] = xyzz_inf<F>();
        }
        pre[k] = run;
        if (!is_inf(res[k])) run = mulk<8>(run, res[k].zzz);
    });
    F irun = inv(run);
    Static<0, K>::down([&](auto k) {
        if (at[k] == ~(u64)0) return;
        u32* o = out + at[k] * Cfg::AFF_WORDS;
        if (is_inf(res[k])) { zero_record<Cfg::AFF_WORDS>(o); return; }
        const F izzz = mulk<8>(irun, pre[k]);
        irun = mulk<8>(irun, res[k].zzz);
        const F iz = mulk<8>(izzz, res[k].zz);
        const F izz = sqrk<8>(iz);
        Cfg::store_mont(o, mulk<8>(res[k].x, izz), mulk<8>(res[k].y, izzz));
    });
}

// ---- host side ----
FrWords words_of(const Fr& a) {
    FrWords w;
    pack256(w.w, a);
    return w;
}
int env_window(const char* name, int fallback) {
    const char* e = getenv(name);                // tuning knob: every width in range gives the same bytes
    const int v = e ? atoi(e) : 0;
    return v >= ughost::setup::WINDOW_MIN && v <= ughost::setup::WINDOW_MAX ? v : fallback;
}

using namespace ughost::setup;

class DeviceBackend : public Backend {
public:
    explicit DeviceBackend(int device) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || device >= n) throw SetupError("no HIP device " + std::to_string(device));
        if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;      // the calling thread's device, put back when the run ends
        UG_HIP(hipSetDevice(device));
        UG_HIP(hipStreamCreate(&stream_));
    }
    ~DeviceBackend() override {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
        if (previous_ >= 0) (void)hipSetDevice(previous_);
    }

    void lagrange(int logN, const Fr& x, const Fr& scale, const Fr& omega, uint8_t* out) override {
        const u64 N = 1ull << logN;
        DevBuf<u32> d(N * 8);
        launchLagrange(d.get(), logN, x, scale, omega);
        hipLaunchKernelGGL(fr_to_plain_kernel, dim3(grid_for(N, 256)), dim3(256), 0, stream_, d.get(), N);
        UG_KERNEL_CHECK();
        UG_HIP(hipMemcpyAsync(out, d.get(), N * 32, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipStreamSynchronize(stream_));
    }

    void generatorMul(bool g2, const uint8_t* scalars, u64 n, int window, uint8_t* out, double* ms) override {
        if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 scalars");
        const int rec = g2 ? 128 : 64;
        DevBuf<u32> s(n * 8), o(n * (rec / 4)), idx(n), count(1);
        UG_HIP(hipMemcpyAsync(s.get(), scalars, n * 32, hipMemcpyHostToDevice, stream_));
        TimeSink build, mul;
        Table t;
        {
            StreamTimer::Scope sc = timer_.time(stream_, &build);
            buildTable(t, g2, window ? window : (g2 ? WINDOW_G2 : WINDOW_G1));
            sc.stop();
        }
        {
            StreamTimer::Scope sc = timer_.time(stream_, &mul);
            mulSet(t, s.get(), n, idx.get(), count.get(), true, o.get());
            sc.stop();
        }
        UG_HIP(hipMemcpyAsync(out, o.get(), n * rec, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipStreamSynchronize(stream_));
        timer_.resolve();
        if (ms) { ms[0] = build.ms; ms[1] = mul.ms; }
    }

    // (the point combinations of the phase-2 setup: setup_points.hip, on this backend's stream and timer)
    void combine(bool g2, u64 nCols, const u32* colPtr, const u32* index, const uint8_t* coefs, const PointSegs& pts, uint8_t* out,
                 double* ms) override {
        device_points_combine(stream_, timer_, g2, nCols, colPtr, index, coefs, pts, out, ms);
    }
    void scale(const uint8_t* scalar, const uint8_t* points, u64 n, uint8_t* out, double* ms) override {
        device_points_scale(stream_, timer_, scalar, points, n, out, ms);
    }
    void scaleSegments(const ScaleSeg* segs, int n, double* ms) override { device_points_scale_segments(stream_, timer_, segs, n, ms); }
    // (the ratio test: ratio_block_sums_kernel of setup_points.hip, then ratio_judge_kernel of pairing.hip for both levels)
    void ratio(const uint8_t* x, const uint8_t* y, u64 n, const uint8_t* q, u64 maxBlocks, RatioOut& out) override {
        if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        u32 q2[RATIO_Q2_WORDS];
        ratioG2Words(q, q2);
        ratioLevels(x, y, n, maxBlocks, out,
                    [&](const uint8_t* w, uint8_t* sx, uint8_t* sy, double* ms) { device_points_ratio_sums(stream_, timer_, x, y, n, w, sx, sy, ms); },
                    [&](const uint8_t* px, const uint8_t* py, u64 m, uint8_t* wrong, double* ms) { ratio_judge_device(stream_, ratioConsts(), px, py, m, q2, wrong, ms); });
    }
    // (the inverse transform over points that prepares a .ptau: ptau_prepare.hip)
    void intt(bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out, double* ms) override {
        device_points_intt(stream_, timer_, g2, logN, nVec, in, nGiven, out, ms);
    }

    void points(const Plan& p, const ColMatrix cm[3], const std::vector<Piece>& pieces, uint8_t* a, uint8_t* b1, uint8_t* b2, uint8_t* k,
                uint8_t* h, double ms[PHASES]) override {
        const u64 N = p.N, M = p.nVars;
        double t0 = nowMs();
        // upload: the column index, coefficients to device form
        DevBuf<u32> colPtr[3], row[3], val[3];
        ColDev cd;
        for (int m = 0; m < 3; m++) {
            const u64 terms = cm[m].terms();
            colPtr[m].alloc(M + 1); row[m].alloc(terms); val[m].alloc(terms * 8);
            UG_HIP(hipMemcpyAsync(colPtr[m].get(), cm[m].colPtr.data(), (M + 1) * 4, hipMemcpyHostToDevice, stream_));
            if (terms) {
                UG_HIP(hipMemcpyAsync(row[m].get(), cm[m].row.data(), terms * 4, hipMemcpyHostToDevice, stream_));
                UG_HIP(hipMemcpyAsync(val[m].get(), cm[m].val.data(), terms * 32, hipMemcpyHostToDevice, stream_));
                hipLaunchKernelGGL(fr_from_plain_kernel, dim3(grid_for(terms, 256)), dim3(256), 0, stream_, val[m].get(), terms);
                UG_KERNEL_CHECK();
            }
            cd.col_ptr[m] = colPtr[m].get(); cd.row[m] = row[m].get(); cd.val[m] = val[m].get();
        }
        DevBuf<Piece> dPieces(pieces.size());
        DevBuf<u32> partial(pieces.size() * 8);
        DevBuf<uint8_t> cls(M);
        if (!pieces.empty()) UG_HIP(hipMemcpyAsync(dPieces.get(), pieces.data(), pieces.size() * sizeof(Piece), hipMemcpyHostToDevice, stream_));
        UG_HIP(hipMemcpyAsync(cls.get(), p.cls.data(), M, hipMemcpyHostToDevice, stream_));
        DevBuf<u32> lag(N * 8), lagCoset(N * 8), sa(M * 8), sb(M * 8), sk(M * 8), sh(N * 8);
        UG_HIP(hipStreamSynchronize(stream_));
        ms[0] += nowMs() - t0;

        TimeSink sinks[4];
        {
            StreamTimer::Scope sc = timer_.time(stream_, &sinks[0]);
            launchLagrange(lag.get(), p.logN, p.x[0], p.lagScale[0], p.omega);
            launchLagrange(lagCoset.get(), p.logN, p.x[1], p.lagScale[1], p.omega);
            sc.stop();
        }
        {
            StreamTimer::Scope sc = timer_.time(stream_, &sinks[1]);
            WireArgs wa;
            wa.alpha = words_of(p.alpha); wa.beta = words_of(p.beta);
            for (int i = 0; i < 3; i++) wa.inv[i] = words_of(p.inv[i]);
            wa.n_wires = p.nVars;
            u32 at = 0;
            for (int m = 0; m < 3; m++) {
                wa.piece_first[m] = at;
                while (at < pieces.size() && pieces[at].m == (u32)m) at++;
            }
            wa.piece_first[3] = at;
            if (!pieces.empty()) {
                hipLaunchKernelGGL(column_pieces_kernel, dim3((unsigned)pieces.size()), dim3(256), 0, stream_, cd, dPieces.get(), (u32)pieces.size(), lag.get(), partial.get());
                UG_KERNEL_CHECK();
            }
            hipLaunchKernelGGL(wire_sums_kernel, dim3(grid_for(M, 256)), dim3(256), 0, stream_, cd, dPieces.get(), partial.get(), lag.get(), cls.get(), wa, sa.get(), sb.get(), sk.get());
            UG_KERNEL_CHECK();
            hipLaunchKernelGGL(h_scalars_kernel, dim3(grid_for(N, 256)), dim3(256), 0, stream_, sh.get(), lagCoset.get(), N, words_of(p.hScale));
            UG_KERNEL_CHECK();
            sc.stop();
        }
        // G1: A, B1, K, H; the B scalars' compaction serves B2 as well
        const u64 most = std::max(M, N);
        DevBuf<u32> idx(most), idxB(M), count(1), countB(1);
        DevBuf<u32> oa(M * 16), ob1(M * 16), ok(M * 16), oh(N * 16), ob2(M * 32);
        {
            StreamTimer::Scope sc = timer_.time(stream_, &sinks[2]);
            Table t;
            buildTable(t, false, env_window("UG_SETUP_WINDOW_G1", WINDOW_G1));
            mulSet(t, sa.get(), M, idx.get(), count.get(), true, oa.get());
            mulSet(t, sk.get(), M, idx.get(), count.get(), true, ok.get());
            mulSet(t, sh.get(), N, idx.get(), count.get(), true, oh.get());
            mulSet(t, sb.get(), M, idxB.get(), countB.get(), true, ob1.get(), ob2.get());
            sc.stop();
            UG_HIP(hipStreamSynchronize(stream_));      // (the table is freed when t goes)
        }
        {
            StreamTimer::Scope sc = timer_.time(stream_, &sinks[3]);
            Table t;
            buildTable(t, true, env_window("UG_SETUP_WINDOW_G2", WINDOW_G2));
            mulSet(t, sb.get(), M, idxB.get(), countB.get(), false, ob2.get());
            sc.stop();
            UG_HIP(hipStreamSynchronize(stream_));
        }
        timer_.resolve();
        for (int i = 0; i < 4; i++) ms[1 + i] += sinks[i].ms;
        t0 = nowMs();
        UG_HIP(hipMemcpyAsync(a, oa.get(), M * 64, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipMemcpyAsync(b1, ob1.get(), M * 64, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipMemcpyAsync(b2, ob2.get(), M * 128, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipMemcpyAsync(k, ok.get(), M * 64, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipMemcpyAsync(h, oh.get(), N * 64, hipMemcpyDeviceToHost, stream_));
        UG_HIP(hipStreamSynchronize(stream_));
        ms[5] += nowMs() - t0;
    }

private:
    struct Table { DevBuf<u32> rec; bool g2 = false; int c = 0, tables = 0; u32 half = 0; };

    void launchLagrange(u32* out, int logN, const Fr& x, const Fr& scale, const Fr& omega) {
        const u64 N = 1ull << logN;
        LagArgs a;
        a.x = words_of(x); a.scale = words_of(scale); a.omega = words_of(omega);
        a.omega_inv = words_of(cond_sub_q(inv(omega)));
        hipLaunchKernelGGL(lagrange_kernel, dim3(grid_for((N + LAG_K - 1) / LAG_K, 256)), dim3(256), 0, stream_, out, (u32)N, a);
        UG_KERNEL_CHECK();
    }
    void buildTable(Table& t, bool g2, int c) {
        t.g2 = g2; t.c = c; t.tables = windowCount(c); t.half = 1u << (c - 1);
        const int words = g2 ? 32 : 16;
        t.rec.alloc((u64)t.tables * t.half * words);
        u32 gen[32];
        generatorWords(g2, gen);
        DevBuf<u32> dGen(words);
        UG_HIP(hipMemcpyAsync(dGen.get(), gen, words * 4, hipMemcpyHostToDevice, stream_));
        const u64 rest = (u64)t.tables * (t.half - 1);
        if (g2) {
            hipLaunchKernelGGL(gen_table_bases_kernel<S2>, dim3(1), dim3(64), 0, stream_, t.rec.get(), dGen.get(), c, t.tables, t.half);
            UG_KERNEL_CHECK();
            hipLaunchKernelGGL(gen_table_fill_kernel<S2>, dim3(grid_for(rest, 128)), dim3(128), 0, stream_, t.rec.get(), t.tables, t.half);
        } else {
            hipLaunchKernelGGL(gen_table_bases_kernel<S1>, dim3(1), dim3(64), 0, stream_, t.rec.get(), dGen.get(), c, t.tables, t.half);
            UG_KERNEL_CHECK();
            hipLaunchKernelGGL(gen_table_fill_kernel<S1>, dim3(grid_for(rest, 128)), dim3(128), 0, stream_, t.rec.get(), t.tables, t.half);
        }
        UG_KERNEL_CHECK();
        UG_HIP(hipStreamSynchronize(stream_));          // (dGen goes here)
    }
    // out = scalars * G over the table's group. compact: find the non-zero scalars first (and write the zero records -- of the
    // table's group into out, of the other group into other when that is given); else idx / count are taken as they are.
    void mulSet(const Table& t, const u32* scalars, u64 n, u32* idx, u32* count, bool compact, u32* out, u32* other = nullptr) {
        if (!n) return;
        if (compact) {
            UG_HIP(hipMemsetAsync(count, 0, 4, stream_));
            hipLaunchKernelGGL(compact_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream_, scalars, n, idx, count, t.g2 ? other : out, t.g2 ? out : other);
            UG_KERNEL_CHECK();
        }
        if (t.g2) {
            hipLaunchKernelGGL(gen_mul_kernel<S2>, dim3(grid_for((n + S2::KPL - 1) / S2::KPL, S2::BLOCK)), dim3(S2::BLOCK), 0, stream_, scalars, idx, count, n,
                               t.rec.get(), t.c, t.tables, t.half, out);
        } else {
            hipLaunchKernelGGL(gen_mul_kernel<S1>, dim3(grid_for((n + S1::KPL - 1) / S1::KPL, S1::BLOCK)), dim3(S1::BLOCK), 0, stream_, scalars, idx, count, n,
                               t.rec.get(), t.c, t.tables, t.half, out);
        }
        UG_KERNEL_CHECK();
    }

    hipStream_t stream_ = nullptr;
    int previous_ = -1;
    StreamTimer timer_;
};

Backend* make_device_backend(int device) { return new DeviceBackend(device); }
struct Registrar {
    Registrar() { ughost::setup::deviceBackendFactory = &make_device_backend; }
} registrar;

}  // namespace
}  // namespace ug
