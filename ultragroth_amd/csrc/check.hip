// check.hip -- is a zkey record a point at all? Field range, curve equation and (G2) subgroup membership, one point per lane.
//
// The prover multiplies whatever a .zkey hands it: convert_coords_kernel (msm.hip) reduces any 256-bit word into [0, q) and
// the group law of ec.hpp relies on its inputs being points of the order-r group. These kernels read the RAW records -- zkey
// format, Montgomery R = 2^256 -- before any conversion and say which is the first that breaks a rule, in this order:
//   1 UG_POINT_UNREDUCED     a coordinate (any of the four Fq components for G2) is >= q as a 256-bit integer. Tested on the
//                            raw words: the conversion would reduce the value and hide it.
//   2 UG_POINT_OFF_CURVE     y^2 != x^3 + 3 (G1),  y^2 != x^3 + 3/(9+u) over Fq2 (G2); canonical values compared.
//   3 UG_POINT_OFF_SUBGROUP  G2, level 2: [r]P != infinity. G1 has prime order r, but the twist has cofactor 2q - r: a point
//                            can be on it and outside the subgroup, and only a scalar multiple shows it.
// The all-zero record is the point at infinity and passes.
//
// [r]P is a double-and-add over the bits of r, a fixed scalar (254 bits, weight 101; the bits come from the kernel argument, read
// with scalar loads): every lane of a wave takes the same branch at every step, so 253 xyzz_dbl + 100 xyzz_madd run without divergence. xyzz_madd handles P + P and P + (-P); for
// a good point the last step IS the second case ([r-1]P + P). xyzz_dbl needs y != 0: no point of the curve has order 2, since
// both r and 2q - r are odd, and only points that passed rule 2 enter the ladder.
//
// Result: one 64-bit word, all ones = clean; every bad lane does atomicMin(word, index << 2 | reason), so the lowest bad index
// wins, and a lane reports the first rule its point breaks. A plain vector atomic: no early exit, no host read-back per launch.
// The mask form (check_points_mask) runs the same rules and stores one status byte per record instead, clean records included, so
// one pass answers for every point: batch verification drops every pi_b outside the subgroup after ONE call.
#include "dev_common.hpp"
#include "internal.hpp"
#include "../../include/ultragroth_hip.h"

namespace ug {

namespace {

struct CurveB {                       // kernel argument: wave-uniform, read with scalar loads
    u32 g1[NL], g2a[NL], g2b[NL];     // the curves' constant terms, device form, canonical
    u32 r[8];                         // the group order, for the ladder's bit tests
};

// raw 256-bit word >= q ?
__device__ __forceinline__ bool raw_ge_q(const u32* w) {
    bool ge = true;                                            // equal so far
#pragma unroll
    for (int i = 0; i < 8; i++) {                              // from the lowest word up: the highest difference decides
        const u32 qi = FqParams::q32[i];
        ge = w[i] > qi || (w[i] == qi && ge);
    }
    return ge;
}
// raw zkey coordinate below q -> canonical device form
__device__ __forceinline__ Fq coord(const u32* w) { return cond_sub_q(from_mont256<FqParams>(w)); }

// The two reporters. The kernels below hand every lane's verdict (0 = clean) to one of them; nothing else differs between the forms.
// FaultWord: one 64-bit word for the whole call, the lowest bad index wins (ug_points_check, the creation switch).
struct FaultWord {
    unsigned long long* fault;
    u64 index0;                       // the global index of the launch's first record
    __device__ __forceinline__ void operator()(u64 i, int reason) const {
        if (reason) atomicMin(fault, (unsigned long long)(((index0 + i) << 2) | (u64)reason));
    }
};
// StatusBytes: one byte per record of the launch, clean ones included (ug_points_check_mask): a plain vector store per lane.
struct StatusBytes {
    uint8_t* status;
    __device__ __forceinline__ void operator()(u64 i, int reason) const { status[i] = (uint8_t)reason; }
};

// The rules hand a lane's verdict to the reporter where it falls, so that the fault-word form compiles to what it was before the
// mask form existed (a constant reason at every site: the clean ones vanish).
template <class Report>
__global__ __launch_bounds__(256) void check_g1_kernel(const u32* __restrict__ pts, u64 n, CurveB k, Report report) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[16];
    load8(w, pts + i * 16); load8(w + 8, pts + i * 16 + 8);
    u32 o = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) o |= w[j];
    if (o == 0) { report(i, UG_POINT_OK); return; }            // infinity
    if (raw_ge_q(w) || raw_ge_q(w + 8)) { report(i, UG_POINT_UNREDUCED); return; }
    const Fq x = coord(w), y = coord(w + 8);
    const Fq rhs = add(mul(sqr(x), x), fp_from<FqParams>(k.g1));      // < 3q
    if (!equal(sqr(y), rhs)) report(i, UG_POINT_OFF_CURVE);
    else report(i, UG_POINT_OK);
}

// LADDER = false: rules 1-2, a memory-bound pass. LADDER = true: rule 3 as well, ~355 Fq2 group operations per point: the register
// picture of window_tables_kernel<G2Cfg> (an XYZZ point over Fq2 is 72 words, the formulas' temporaries as many again), so the
// same block of 128 and no occupancy demand that would force spills on the ladder's inner loop (DESIGN.md has the figures).
template <bool LADDER, class Report>
__global__ __launch_bounds__(LADDER ? 128 : 256) void check_g2_kernel(const u32* __restrict__ pts, u64 n, CurveB k, Report report) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[32];
    const u32* p = pts + i * 32;
    load8(w, p); load8(w + 8, p + 8); load8(w + 16, p + 16); load8(w + 24, p + 24);
    u32 o = 0;
#pragma unroll
    for (int j = 0; j < 32; j++) o |= w[j];
    if (o == 0) { report(i, UG_POINT_OK); return; }            // infinity
    if (raw_ge_q(w) || raw_ge_q(w + 8) || raw_ge_q(w + 16) || raw_ge_q(w + 24)) { report(i, UG_POINT_UNREDUCED); return; }
    Fq2 x, y, b;
    x.a = coord(w); x.b = coord(w + 8); y.a = coord(w + 16); y.b = coord(w + 24);
    b.a = fp_from<FqParams>(k.g2a); b.b = fp_from<FqParams>(k.g2b);
    const Fq2 lhs = canon(sqrk<1>(y)), rhs = canon(add(mulk<1>(sqrk<1>(x), x), b));      // (canonical inputs: components < q)
    u32 d = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) d |= (lhs.a.l[j] ^ rhs.a.l[j]) | (lhs.b.l[j] ^ rhs.b.l[j]);
    if (d) { report(i, UG_POINT_OFF_CURVE); return; }
    if (LADDER) {
        XYZZ<Fq2> acc = xyzz_from_affine(x, y);                // the top bit of r
#pragma unroll 1
        for (int bit = 252; bit >= 0; bit--) {
            acc = xyzz_dbl(acc);
            if ((k.r[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd(acc, x, y);
        }
        if (!is_inf(acc)) { report(i, UG_POINT_OFF_SUBGROUP); return; }
    }
    report(i, UG_POINT_OK);
}

const CurveB& curve_b() {
    static const CurveB k = [] {
        CurveB c;
        u32 w[8] = {3, 0, 0, 0, 0, 0, 0, 0};
        const Fq three = canon(from_normal<FqParams>(w));
        w[0] = 9;
        Fq2 xi;                                                // 9 + u
        xi.a = from_normal<FqParams>(w); xi.b = fp_one<FqParams>();
        const Fq2 b2 = canon(mul_fp(inv(xi), three));          // 3 / (9 + u)
        for (int i = 0; i < 8; i++) c.r[i] = FrParams::q32[i];
        for (int i = 0; i < NL; i++) { c.g1[i] = three.l[i]; c.g2a[i] = b2.a.l[i]; c.g2b[i] = b2.b.l[i]; }
        return c;
    }();
    return k;
}

template <class Report> void launch_checks(bool g2, const u32* pts, u64 n, int level, const Report& report, hipStream_t stream) {
    if (!n) return;
    const CurveB& k = curve_b();
    if (!g2)
        hipLaunchKernelGGL(check_g1_kernel<Report>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pts, n, k, report);
    else if (level < 2)
        hipLaunchKernelGGL((check_g2_kernel<false, Report>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pts, n, k, report);
    else
        hipLaunchKernelGGL((check_g2_kernel<true, Report>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, stream, pts, n, k, report);
    UG_KERNEL_CHECK();
}

}  // namespace

void check_points(bool g2, const u32* pts, u64 n, u64 index0, int level, unsigned long long* fault, hipStream_t stream) {
    launch_checks(g2, pts, n, level, FaultWord{fault, index0}, stream);
}
void check_points_mask(bool g2, const u32* pts, u64 n, int level, uint8_t* status, hipStream_t stream) {
    launch_checks(g2, pts, n, level, StatusBytes{status}, stream);
}

}  // namespace ug
