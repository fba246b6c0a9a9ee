// ptau_prepare.hip -- the inverse transform over GROUP POINTS that prepares a powers-of-tau file for phase 2 (setup_host.hpp:
// Backend::intt; include/ultragroth_hip.h: ug_ptau_prepare_run, ug_points_intt). For N = 2^p, omega = 5^((r - 1) / N) and points
// P_0 .. P_(N-1):  out[k] = (1 / N) sum_j omega^(-j k) P_j,  which is [L_k(tau)] X when P_j = [tau^j] X.
//
//   intt_scale_kernel    one lane per point: (1 / N) P_i by the bit walk of setup_dev.hpp, stored affine at the bit-reversed
//                        index. 1 / N = -(r - 1) / N mod r, so the walk is over 254 - p bits of the negated point. Indices from
//                        n_given on are infinity.
//   intt_stage_kernel    one launch per stage of the decimation-in-time radix-2 transform, one lane per butterfly: t = w b by the
//                        same walk (a twiddle of 1 -- the whole first stage, lane 0 of every block later -- skips it), a + t and
//                        a - t by two mixed additions of the affine a, both converted with ONE shared inversion. Points stay
//                        affine between the stages, in 64 / 128-byte records of the device's packed form; the last stage writes
//                        the file's records.
// The vectors of one call (the sections 12, 14 and 15 of a level) share every launch: blockIdx.y is the vector.
// A twiddle above r / 2 is the negated point times r - w, as setup_points.hip folds coefficients. xyzz_madd handles an
// accumulator at infinity, a doubling and a sum at infinity, so a = infinity is the only case decided here.
// Plain C++ and vector stores only. DESIGN.md section 5.10 has the registers and what was measured.
#include "setup_dev.hpp"
#include "stream_timer.hpp"
#include "setup_host.hpp"
#include "internal.hpp"

namespace ug {
namespace {

using namespace sdev;
using namespace ughost::setup;

struct Folded { u32 w[8]; };                     // a magnitude below 2^255; bit 255: the point is negated

// src: n_vec vectors of n_given records (packed device form); dst: n_vec vectors of 2^log_n
template <class Cfg>
__global__ __launch_bounds__(Cfg::BLOCK) void intt_scale_kernel(const u32* __restrict__ src, u32* __restrict__ dst, u32 log_n, u32 n_given, Folded c) {
    typedef typename Cfg::F F;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << log_n)) return;
    const u32 j = __brev(i) >> (32 - log_n);     // (log_n >= 1)
    u32* o = dst + (((u64)blockIdx.y << log_n) + j) * Cfg::AFF_WORDS;
    if (i >= n_given) { zero_record<Cfg::AFF_WORDS>(o); return; }
    F x, y;
    Cfg::load(src + ((u64)blockIdx.y * n_given + i) * Cfg::AFF_WORDS, x, y);
    if (affine_is_inf(x, y)) { zero_record<Cfg::AFF_WORDS>(o); return; }
    u32 s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = c.w[k];
    if (s[7] >> 31) y = neg<1>(y);
    s[7] &= 0x7fffffffu;
    const XYZZ<F> acc = walk_product(s, x, y);
    if (is_inf(acc)) { zero_record<Cfg::AFF_WORDS>(o); return; }      // (only a point outside the subgroup of order r gets here)
    F ax, ay;
    xyzz_to_affine(ax, ay, acc);
    Cfg::store_packed(o, ax, ay);
}

// data: n_vec vectors of 2^log_n records, in place. Stage s pairs records 2^s apart inside blocks of 2^(s+1); tw: 2^(log_n-1)
// folded twiddles omega^(-j), 8 words each, of which this stage reads every 2^(log_n-1-s)-th.
template <class Cfg, bool LAST>
__global__ __launch_bounds__(Cfg::BLOCK) void intt_stage_kernel(u32* __restrict__ data, const u32* __restrict__ tw, u32 log_n, u32 stage) {
    typedef typename Cfg::F F;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << (log_n - 1))) return;
    const u32 j = t & ((1u << stage) - 1);
    const u64 ia = ((u64)(t >> stage) << (stage + 1)) + j;
    u32* pa = data + (((u64)blockIdx.y << log_n) + ia) * Cfg::AFF_WORDS;
    u32* pb = pa + ((u64)Cfg::AFF_WORDS << stage);
    XYZZ<F> tv;
    {
        F bx, by;
        Cfg::load(pb, bx, by);
        if (affine_is_inf(bx, by)) {
            tv = xyzz_inf<F>();
        } else if (j == 0) {
            tv = xyzz_from_affine(bx, by);
        } else {
            u32 s[8];
            load8(s, tw + ((u64)j << (log_n - 1 - stage)) * 8);
            if (s[7] >> 31) by = neg<1>(by);
            s[7] &= 0x7fffffffu;
            tv = walk_product(s, bx, by);
        }
    }
    XYZZ<F> sum, dif;
    {
        F ax, ay;
        Cfg::load(pa, ax, ay);
        if (affine_is_inf(ax, ay)) {
            sum = tv;
            dif = xyzz_neg(tv);
        } else {
            sum = xyzz_madd(tv, ax, ay);
            dif = xyzz_neg(xyzz_madd(tv, ax, neg<1>(ay)));       // a - t = -(t - a)
        }
    }
    // both to affine with one inversion (column_points_kernel's ending, two results)
    const bool si = is_inf(sum), di = is_inf(dif);
    const F run = si ? field_one((F*)0) : sum.zzz;
    F irun = inv(di ? run : mulk<8>(run, dif.zzz));
    if (di) {
        zero_record<Cfg::AFF_WORDS>(pb);
    } else {
        const F izzz = mulk<8>(irun, run);
        irun = mulk<8>(irun, dif.zzz);
        const F izz = sqrk<8>(mulk<8>(izzz, dif.zz));
        const F ox = mulk<8>(dif.x, izz), oy = mulk<8>(dif.y, izzz);
        if (LAST) Cfg::store_mont(pb, ox, oy);
        else Cfg::store_packed(pb, canon(ox), canon(oy));
    }
    if (si) {
        zero_record<Cfg::AFF_WORDS>(pa);
    } else {
        const F izz = sqrk<8>(mulk<8>(irun, sum.zz));
        const F ox = mulk<8>(sum.x, izz), oy = mulk<8>(sum.y, irun);
        if (LAST) Cfg::store_mont(pa, ox, oy);
        else Cfg::store_packed(pa, canon(ox), canon(oy));
    }
}

template <class Cfg>
void intt_on_device(hipStream_t stream, StreamTimer& timer, int logN, int nVec, const uint8_t* const* in, u64 nGiven, uint8_t* const* out,
                    double* ms) {
    constexpr u64 REC = Cfg::AFF_WORDS * 4;
    const u64 N = 1ull << logN, half = N / 2;
    // every byte of the level is asked for before its first kernel: the inputs, the working vectors, the twiddles
    const u64 need = ((u64)nVec * nGiven + (u64)nVec * N) * REC + half * 32;
    size_t freeBytes = 0, totalBytes = 0;
    UG_HIP(hipMemGetInfo(&freeBytes, &totalBytes));
    if (need > freeBytes) throw std::invalid_argument("ptau: level " + std::to_string(logN) + " needs " + std::to_string(need) + " bytes on the device");
    std::vector<u32> tw;
    inttTwiddles(logN, tw);
    Folded c;
    inttScale(logN, c.w);
    DevBuf<u32> dSrc(std::max<u64>((u64)nVec * nGiven, 1) * Cfg::AFF_WORDS), dWork((u64)nVec * N * Cfg::AFF_WORDS), dTw(half * 8);
    for (int v = 0; v < nVec; v++)
        if (nGiven) UG_HIP(hipMemcpyAsync(dSrc.get() + (u64)v * nGiven * Cfg::AFF_WORDS, in[v], nGiven * REC, hipMemcpyHostToDevice, stream));
    UG_HIP(hipMemcpyAsync(dTw.get(), tw.data(), half * 32, hipMemcpyHostToDevice, stream));
    if (std::is_same<typename Cfg::F, Fq2>::value) convert_points_g2(dSrc.get(), (u64)nVec * nGiven, stream);
    else convert_points_g1(dSrc.get(), (u64)nVec * nGiven, stream);
    TimeSink scale, stages;
    {
        StreamTimer::Scope sc = timer.time(stream, &scale);
        hipLaunchKernelGGL(intt_scale_kernel<Cfg>, dim3(grid_for(N, Cfg::BLOCK), nVec), dim3(Cfg::BLOCK), 0, stream, dSrc.get(), dWork.get(), (u32)logN,
                           (u32)nGiven, c);
        UG_KERNEL_CHECK();
        sc.stop();
    }
    {
        StreamTimer::Scope sc = timer.time(stream, &stages);
        const dim3 grid(grid_for(half, Cfg::BLOCK), nVec), block(Cfg::BLOCK);
        for (int s = 0; s < logN; s++) {
            if (s == logN - 1) hipLaunchKernelGGL((intt_stage_kernel<Cfg, true>), grid, block, 0, stream, dWork.get(), dTw.get(), (u32)logN, (u32)s);
            else hipLaunchKernelGGL((intt_stage_kernel<Cfg, false>), grid, block, 0, stream, dWork.get(), dTw.get(), (u32)logN, (u32)s);
            UG_KERNEL_CHECK();
        }
        sc.stop();
    }
    for (int v = 0; v < nVec; v++) UG_HIP(hipMemcpyAsync(out[v], dWork.get() + (u64)v * N * Cfg::AFF_WORDS, N * REC, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipStreamSynchronize(stream));
    timer.resolve();
    if (ms) { ms[0] = scale.ms; ms[1] = stages.ms; }
}

}  // namespace

void device_points_intt(hipStream_t stream, StreamTimer& timer, bool g2, int logN, int nVec, const uint8_t* const* in, u64 nGiven,
                        uint8_t* const* out, double* ms) {
    if (ms) ms[0] = ms[1] = 0;
    if (inttTrivial(g2, logN, nVec, in, nGiven, out)) return;
    if (g2) intt_on_device<S2>(stream, timer, logN, nVec, in, nGiven, out, ms);
    else intt_on_device<S1>(stream, timer, logN, nVec, in, nGiven, out, ms);
}

}  // namespace ug
