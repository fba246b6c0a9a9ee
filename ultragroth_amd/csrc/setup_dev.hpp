// setup_dev.hpp -- what the two device translation units of the setups share (setup.hip: the development setup; setup_points.hip:
// the point combinations of the phase-2 setup): compile-time loops, the curve configurations, the all-zero record, an owned
// device buffer.
#pragma once
#include "dev_common.hpp"

#include <type_traits>

namespace ug {
namespace sdev {

inline unsigned grid_for(u64 n, int block) { return (unsigned)((n + block - 1) / block); }

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

// ---- host side ----
template <class T> struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    explicit DevBuf(u64 n) { alloc(n); }
    void alloc(u64 n) { release(); if (n) UG_HIP(hipMalloc((void**)&p, n * sizeof(T))); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

}  // namespace sdev
}  // namespace ug
