// setup_dev.hpp -- what the two device translation units of the setups share (setup.hip: the development setup; setup_points.hip:
// the point combinations of the phase-2 setup): compile-time loops, the curve configurations, the all-zero record, the per-lane
// double-and-add walk (ptau_prepare.hip's butterflies use it too).
#pragma once
#include "dev_common.hpp"

#include <type_traits>

namespace ug {
namespace sdev {

// compile-time loops: every index is a constant, so per-lane arrays stay in registers (a `#pragma unroll` the optimizer
// declines leaves them indexed at run time, i.e. in scratch)
template <int I, int N> struct Static {
    template <class Fn> static __device__ __forceinline__ void up(Fn&& f) { f(std::integral_constant<int, I>()); Static<I + 1, N>::up(f); }
    template <class Fn> static __device__ __forceinline__ void down(Fn&& f) { Static<I + 1, N>::down(f); f(std::integral_constant<int, I>()); }
};
template <int N> struct Static<N, N> {
    template <class Fn> static __device__ __forceinline__ void up(Fn&&) {}
    template <class Fn> static __device__ __forceinline__ void down(Fn&&) {}
};

// ---- curve configurations ----
struct S1 {
    typedef Fq F;
    static constexpr int AFF_WORDS = 16, KPL = 2, BLOCK = 128;
    static __device__ __forceinline__ void load(const u32* p, F& x, F& y) {
        x = ld_packed<FqParams>(p); y = ld_packed<FqParams>(p + 8);
    }
    static __device__ __forceinline__ void store_packed(u32* o, const F& x, const F& y) { st_packed(o, x); st_packed(o + 8, y); }
    static __device__ __forceinline__ void store_mont(u32* o, const F& x, const F& y) {
        u32 w[8];
        to_mont256(w, x); store8(o, w);
        to_mont256(w, y); store8(o + 8, w);
    }
};
struct S2 {
    typedef Fq2 F;
    static constexpr int AFF_WORDS = 32, KPL = 1, BLOCK = 64;
    static __device__ __forceinline__ void load(const u32* p, F& x, F& y) {
        x.a = ld_packed<FqParams>(p); x.b = ld_packed<FqParams>(p + 8); y.a = ld_packed<FqParams>(p + 16); y.b = ld_packed<FqParams>(p + 24);
    }
    static __device__ __forceinline__ void store_packed(u32* o, const F& x, const F& y) {
        st_packed(o, x.a); st_packed(o + 8, x.b); st_packed(o + 16, y.a); st_packed(o + 24, y.b);
    }
    static __device__ __forceinline__ void store_mont(u32* o, const F& x, const F& y) {
        u32 w[8];
        to_mont256(w, x.a); store8(o, w);
        to_mont256(w, x.b); store8(o + 8, w);
        to_mont256(w, y.a); store8(o + 16, w);
        to_mont256(w, y.b); store8(o + 24, w);
    }
};
template <int WORDS> __device__ __forceinline__ void zero_record(u32* o) {
    uint4* q = reinterpret_cast<uint4*>(o);
#pragma unroll
    for (int i = 0; i < WORDS / 4; i++) q[i] = make_uint4(0, 0, 0, 0);
}

template <class F> __device__ __forceinline__ bool affine_is_inf(const F& x, const F& y) { return limbs_all_zero(x) && limbs_all_zero(y); }

// ---- k * (x, y) by double-and-add, one lane ----
// s: the 8 plain words of k, 1 <= k < 2^255 (destroyed); (x, y) affine, canonical, not infinity. The words are shifted up until the
// top bit of k sits at bit 255, then one bit at a time: no register array is indexed by a run-time value. Every addition is a
// mixed one of the affine base. For a base of order r and k < r the accumulator never meets the base or its negative.
template <class F> __device__ __forceinline__ XYZZ<F> walk_product(u32 (&s)[8], const F& x, const F& y) {
    int top = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (s[i]) top = 32 * i + 31 - __clz(s[i]);
    const int wsh = 7 - (top >> 5), bsh = 31 - (top & 31);
#pragma unroll
    for (int k = 0; k < 7; k++) {
        if (k < wsh) {
#pragma unroll
            for (int i = 7; i > 0; i--) s[i] = s[i - 1];
            s[0] = 0;
        }
    }
    if (bsh) {
#pragma unroll
        for (int i = 7; i > 0; i--) s[i] = (s[i] << bsh) | (s[i - 1] >> (32 - bsh));
        s[0] <<= bsh;
    }
    XYZZ<F> acc = xyzz_from_affine(x, y);        // the top bit
#pragma unroll 1
    for (int b = 0; b < top; b++) {
#pragma unroll
        for (int i = 7; i > 0; i--) s[i] = (s[i] << 1) | (s[i - 1] >> 31);
        s[0] <<= 1;
        acc = xyzz_dbl(acc);
        if (s[7] >> 31) acc = xyzz_madd(acc, x, y);
    }
    return acc;
}

}  // namespace sdev
}  // namespace ug
