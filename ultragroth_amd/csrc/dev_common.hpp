// dev_common.hpp -- shared device-side helpers: error handling, packed 32-byte element I/O.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <utility>
#include <type_traits>
#include <stdexcept>
#include <string>
#include "ec.hpp"

namespace ug {

struct HipError : public std::runtime_error {
    explicit HipError(const std::string& m) : std::runtime_error(m) {}
};

#define UG_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            throw ug::HipError(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr + \
                               " (" __FILE__ ":" + std::to_string(__LINE__) + ")");                \
    } while (0)

#define UG_KERNEL_CHECK() UG_HIP(hipGetLastError())

// blocks of `block` lanes that cover n
inline unsigned grid_for(u64 n, int block) { return (unsigned)((n + block - 1) / block); }

// An owned HIP event (move-only); timing = false: an ordering-only event (hipEventDisableTiming). A default one is empty.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    explicit Event(bool timing) { UG_HIP(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// Owned device memory: n elements of T (move-only, empty by default). The only owner of device memory in csrc: members and
// locals are DevBuf, kernels and kernel argument structs get the raw pointer (get()). A request for 0 elements allocates 4 bytes:
// a buffer that was allocated is never null. The destructor frees, and hipFree waits for the whole device: where the place of a
// free matters, release() says so at that place.
template <class T> struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    explicit DevBuf(size_t n) { alloc(n); }
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }      // (the old memory goes with o)
    ~DevBuf() { release(); }
    void alloc(size_t n) { release(); UG_HIP(hipMalloc((void**)&p, n ? n * sizeof(T) : 4)); }      // frees what it held first
    // for the callers that turn a failed allocation into a message of their own: false, and HIP's sticky error is cleared
    bool try_alloc(size_t n) {
        release();
        if (hipMalloc((void**)&p, n ? n * sizeof(T) : 4) == hipSuccess) return true;
        (void)hipGetLastError();
        p = nullptr;
        return false;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    T* get() const { return p; }
    T* take() { T* r = p; p = nullptr; return r; }      // gives up ownership
    void adopt(T* raw) { release(); p = raw; }          // ... and takes that of memory from hipMalloc (the C interface's void*)
};
// Pinned host memory, the same way.
template <class T> struct PinnedBuf {
    T* p = nullptr;
    PinnedBuf() = default;
    explicit PinnedBuf(size_t n) { alloc(n); }
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    ~PinnedBuf() { release(); }
    void alloc(size_t n) { release(); UG_HIP(hipHostMalloc((void**)&p, n ? n * sizeof(T) : 4, hipHostMallocDefault)); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    T* get() const { return p; }
};

// An event recorded INSIDE a stream capture so that every launch of the resulting graph records it again (timed spans of a
// captured launch sequence): an explicit event-record node behind the stream's current capture dependencies, which then becomes
// the stream's dependency. (hipEventRecordWithFlags(.., hipEventRecordExternal) is the same thing in one call on ROCm 7.2, but
// the runtime a PyTorch wheel bundles -- ROCm 7.0, the one a Python process ends up with -- refuses it: tools/probe_graph_events.hip.)
inline void record_in_capture(hipEvent_t ev, hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t g = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t n = 0;
    UG_HIP(hipStreamGetCaptureInfo_v2(stream, &st, &id, &g, &deps, &n));
    if (st != hipStreamCaptureStatusActive || !g) throw HipError("HIP error: the stream is not being captured (record_in_capture)");
    hipGraphNode_t node = nullptr;
    UG_HIP(hipGraphAddEventRecordNode(&node, g, deps, n, ev));
    UG_HIP(hipStreamUpdateCaptureDependencies(stream, &node, 1, hipStreamSetCaptureDependencies));
}

// Environment switches come in two kinds (the table in include/ultragroth_hip.h lists both):
//   tuning knobs        getenv(): every setting gives correct results, the default is the measured best
//   measurement switches  measure_env(): A/B switches of finished experiments and settings that give WRONG results (folded
//                       gathers). They exist only in a -DUG_MEASURE build (`make MEASURE=1` -> libultragroth_hip_measure.so);
//                       the product library reads none of them.
#ifdef UG_MEASURE
inline const char* measure_env(const char* name) { return getenv(name); }
#else
inline const char* measure_env(const char*) { return nullptr; }
#endif

// ---- 32-byte packed elements in HBM: two 16-byte vector accesses -----------------------------------
__device__ __forceinline__ void load8(u32* w, const u32* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void store8(u32* p, const u32* w) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// element stored as 32 bytes in device Montgomery form (value < 2^256, any representative)
template <class P> __device__ __forceinline__ Fp<P> ld_packed(const u32* p) {
    u32 w[8];
    load8(w, p);
    return unpack256<P>(w);
}
// a must be strict and < 2^256
template <class P> __device__ __forceinline__ void st_packed(u32* p, const Fp<P>& a) {
    u32 w[8];
    pack256(w, a);
    store8(p, w);
}

// Cheap range contraction: any weak a < 64 q  ->  strict, same residue, < 2.01 q.
// Quotient estimate from the top limb (bits 232..260) in fp32, chosen to never exceed the true
// quotient; 9 v_mad_u64_u32 for e*q, then one signed serial carry pass.
template <class P> __device__ __forceinline__ Fp<P> contract(const Fp<P>& a) {
    const float rcp = 1.0f / (float)(P::q[NL - 1] + 2);
    u32 e = (u32)((float)a.l[NL - 1] * rcp * 0.99999f);
    Fp<P> r;
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int64_t v = (int64_t)a.l[i] - (int64_t)((u64)e * P::q[i]) + carry;
        r.l[i] = (u32)v & MASK29;
        carry = v >> LB;
    }
    r.l[NL - 1] |= (u32)carry << LB;   // carry is 0 for in-range inputs; keeps the value if not
    return r;
}

// The sum of one row of a CSR coefficient matrix times the witness (hpoly.hip: rows r < domain: matrix A, the others: matrix B;
// r1cs.hip: one matrix of an .r1cs per triple). val: coef * 2^522 packed, wtns: plain 32-byte integers; the sum is w * coef in
// device Montgomery form, strict, < 2.01 q.
// The walk itself takes the number of sums as a parameter: with SUMS = 2 (the fold of zkey_verify.hip) an entry whose signal id
// is above `split` goes to acc[1], every other one to acc[0]; with SUMS = 1 there is one sum and `split` is not read.
template <int SUMS>
__device__ __forceinline__ void matvec_walk(u32 r, const u32* row_ptr, const u32* sig, const u32* val, const u32* wtns, u32 split, Fr (&acc)[SUMS]) {
    u32 s = row_ptr[r], e = row_ptr[r + 1];
#pragma unroll
    for (int a = 0; a < SUMS; a++) acc[a] = fp_zero<FrParams>();
    u32 since = 0;
    // four entries at a time: their signal ids first, then the four 32-byte witness gathers and the four coefficients all in
    // flight together, then the products (one entry per turn left every gather's latency -- a DRAM row miss -- exposed: 69 %
    // of the kernel's wave cycles were waits)
    for (u32 p = s; p < e; p += 4) {
        const u32 cnt = e - p < 4 ? e - p : 4;
        u32 sg[4], wr[4][8], vr[4][8];
#pragma unroll
        for (int k = 0; k < 4; k++) sg[k] = (u32)k < cnt ? sig[p + k] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((u32)k < cnt) { load8(wr[k], wtns + (size_t)sg[k] * 8); load8(vr[k], val + (size_t)(p + k) * 8); }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((u32)k < cnt) {
                const Fr term = mul(unpack256<FrParams>(wr[k]), unpack256<FrParams>(vr[k]));       // < 2q  (w: plain integer, any value < 2^256)
                if (SUMS == 2 && sg[k] > split) acc[SUMS - 1] = add(acc[SUMS - 1], term);
                else acc[0] = add(acc[0], term);
                if (++since == 24) {                                                                // keep below 64 q
#pragma unroll
                    for (int a = 0; a < SUMS; a++) acc[a] = contract(acc[a]);
                    since = 0;
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < SUMS; a++) acc[a] = contract(acc[a]);
}
__device__ __forceinline__ Fr matvec_row(u32 r, const u32* row_ptr, const u32* sig, const u32* val, const u32* wtns) {
    Fr acc[1];
    matvec_walk<1>(r, row_ptr, sig, val, wtns, 0, acc);
    return acc[0];
}

// ---- the same for a tile of VT witnesses (hpoly.hip: coef_matvec_vectors; r1cs.hip: r1cs_check_vectors) ----
// A lane still owns one row, and now sums it for a tile of VT witnesses: the row's signal ids and coefficients (36 bytes per entry,
// the larger part of the kernel's traffic) are read and unpacked ONCE per tile, only the 32-byte witness gathers are per witness.
// Every accumulator sees exactly the additions and contractions that matvec_row makes for its witness -- the same entries in the same
// order, contracted after every 24th --, so the sums are the same bytes. `live` witnesses of the tile exist (the last tile of a
// launch may be short); wtns is the tile's first witness, the next one wstride words on.
// (the loop over the witnesses of a tile, unrolled by construction: a rolled loop would index the accumulators at run time and put
// them into scratch memory)
template <int I, int N, class F> __device__ __forceinline__ void for_each_vector(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>()); for_each_vector<I + 1, N>(f); }
}
template <int VT>
__device__ __forceinline__ void matvec_row_vectors(Fr (&acc)[VT], u32 r, const u32* row_ptr, const u32* sig, const u32* val, const u32* wtns,
                                                   u64 wstride, int live) {
    u32 s = row_ptr[r], e = row_ptr[r + 1];
#pragma unroll
    for (int v = 0; v < VT; v++) acc[v] = fp_zero<FrParams>();
    u32 since = 0;                                             // additions since the last contraction: a multiple of 4 here
    for (u32 p = s; p < e; p += 4) {
        const u32 cnt = e - p < 4 ? e - p : 4;
        u32 sg[4];
        Fr vq[4];
#pragma unroll
        for (int k = 0; k < 4; k++) sg[k] = (u32)k < cnt ? sig[p + k] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 vr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((u32)k < cnt) load8(vr, val + (size_t)(p + k) * 8);
            vq[k] = unpack256<FrParams>(vr);
        }
        for_each_vector<0, VT>([&](auto vc) __attribute__((always_inline)) {
            constexpr int v = decltype(vc)::value;
            if (v < live) {
                const u32* w = wtns + (size_t)v * wstride;
                u32 wr[4][8];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if ((u32)k < cnt) load8(wr[k], w + (size_t)sg[k] * 8);
                }
                u32 sn = since;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if ((u32)k < cnt) {
                        acc[v] = add(acc[v], mul(unpack256<FrParams>(wr[k]), vq[k]));
                        if (++sn == 24) { acc[v] = contract(acc[v]); sn = 0; }
                    }
                }
            }
        });
        since = (since + cnt) % 24;
    }
#pragma unroll
    for (int v = 0; v < VT; v++) acc[v] = contract(acc[v]);
}

__host__ __device__ __forceinline__ u32 bit_reverse(u32 x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
    u32 r = 0;
    for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
#endif
}

}  // namespace ug
