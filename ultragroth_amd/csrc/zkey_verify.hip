// zkey_verify.hip -- the device side of the key check (zkey_verify_host.cpp, include/ultragroth_hip.h: ug_zkey_verify_run, ug_r1cs_fold).
//
// Two kernels are new. The fold is the witness check's row walk (matvec_walk, dev_common.hpp) with the random weights rho in the
// witness's place and two sums per matrix, stored as canonical plain integers where ug_schedule_build reads MSM scalars. The
// gather copies the odd records of the padded level of section 12, already in the device form, side by side. Everything else is
// the existing engine through its own interface: ug_bases_create_*, one ug_schedule rebuilt per scalar vector, ug_msm_g1 /
// ug_msm_batch. Every base set is used once: classic windows, no tables. A section's bases are freed before the next section is
// uploaded, so the peak of device memory is the slices with the fold's vectors, or H with the padded level -- not the whole key.
// An UltraGroth key (ug_ultra_zkey_verify_run) takes the same route with r1cs_fold_classes_kernel: a class byte per wire, three
// sums per matrix, eleven vectors; its two C sections stand under weights that the host gathers through the key's lists.
// The host part below is one evaluator (sumsOn) and one fold helper (foldOn) for both: the class count and the list of C sections
// come with the Inputs (zkey_verify.hpp), and a Groth16 key's one C section still reads the device's rho in place.
// No LDS, no scratch; plain C++ and vector stores only.
#include "dev_common.hpp"
#include "internal.hpp"
#include "setup_host.hpp"
#include "zkey_verify.hpp"

#include <algorithm>

namespace ug {

namespace {

__global__ __launch_bounds__(256) void r1cs_fold_kernel(R1csDev m, const u32* rho, u32 n_public, u32 domain, u32* out) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= domain) return;
    const size_t vec = (size_t)domain * 8;
    u32* row = out + (size_t)k * 8;
    u32 w[8];
    if (k < m.rows) {
#pragma unroll 1
        for (int t = 0; t < 3; t++) {
            Fr acc[2];
            matvec_walk<2>(k, m.row_ptr[t], m.sig[t], m.val[t], rho, n_public, acc);
            to_normal(w, acc[0]);
            store8(row + (size_t)t * vec, w);
            to_normal(w, acc[1]);
            store8(row + (size_t)(3 + t) * vec, w);
            if (t < 2) {                                            // a and b: one modular addition each
                to_normal(w, contract(add(acc[0], acc[1])));        // both < 2.01 q
                store8(row + (size_t)(6 + t) * vec, w);
            }
        }
        return;
    }
    // the public rows nConstraints + s carry A = {s: 1}: rho_s mod r in a^pub (and in a); every other value of the row is 0
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = 0;
#pragma unroll 1
    for (int v = 1; v < 8; v++)
        if (v != 6) store8(row + (size_t)v * vec, w);
    if (k - m.rows <= n_public) {
        load8(w, rho + (size_t)(k - m.rows) * 8);
        to_normal(w, from_normal<FrParams>(w));
    }
    store8(row, w);
    store8(row + 6 * vec, w);
}

// ---- the fold of an UltraGroth key: a class per wire (one byte: 0 public, 1 round, 2 final) read beside rho, three sums per matrix ----
// matvec_walk's loop with the class byte in the place of the `wire <= n_public` compare (a variant: matvec_walk<2> is as it was)
__device__ __forceinline__ void matvec_walk_classes(u32 r, const u32* row_ptr, const u32* sig, const u32* val, const u32* wtns,
                                                    const uint8_t* cls, Fr (&acc)[3]) {
    u32 s = row_ptr[r], e = row_ptr[r + 1];
#pragma unroll
    for (int a = 0; a < 3; a++) acc[a] = fp_zero<FrParams>();
    u32 since = 0;
    for (u32 p = s; p < e; p += 4) {
        const u32 cnt = e - p < 4 ? e - p : 4;
        u32 sg[4], cl[4], wr[4][8], vr[4][8];
#pragma unroll
        for (int k = 0; k < 4; k++) sg[k] = (u32)k < cnt ? sig[p + k] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((u32)k < cnt) { cl[k] = cls[sg[k]]; load8(wr[k], wtns + (size_t)sg[k] * 8); load8(vr[k], val + (size_t)(p + k) * 8); }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((u32)k < cnt) {
                const Fr term = mul(unpack256<FrParams>(wr[k]), unpack256<FrParams>(vr[k]));       // < 2q
                if (cl[k] == 0) acc[0] = add(acc[0], term);
                else if (cl[k] == 1) acc[1] = add(acc[1], term);
                else acc[2] = add(acc[2], term);
                if (++since == 24) {                                                                // keep below 64 q
#pragma unroll
                    for (int a = 0; a < 3; a++) acc[a] = contract(acc[a]);
                    since = 0;
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) acc[a] = contract(acc[a]);
}
// out: eleven vectors of `domain` plain canonical integers: vector 3 m + t is matrix t (A, B, C) over class m; 9 is a, 10 is b
__global__ __launch_bounds__(256) void r1cs_fold_classes_kernel(R1csDev m, const u32* rho, const uint8_t* cls, u32 n_public, u32 domain, u32* out) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= domain) return;
    const size_t vec = (size_t)domain * 8;
    u32* row = out + (size_t)k * 8;
    u32 w[8];
    if (k < m.rows) {
#pragma unroll 1
        for (int t = 0; t < 3; t++) {
            Fr acc[3];
            matvec_walk_classes(k, m.row_ptr[t], m.sig[t], m.val[t], rho, cls, acc);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                to_normal(w, acc[c]);
                store8(row + (size_t)(3 * c + t) * vec, w);
            }
            if (t < 2) {                                            // a and b: two modular additions each
                to_normal(w, contract(add(contract(add(acc[0], acc[1])), acc[2])));
                store8(row + (size_t)(9 + t) * vec, w);
            }
        }
        return;
    }
    // the public rows, as in r1cs_fold_kernel: rho_s mod r in a^pub and in a
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = 0;
#pragma unroll 1
    for (int v = 1; v < 11; v++)
        if (v != 9) store8(row + (size_t)v * vec, w);
    if (k - m.rows <= n_public) {
        load8(w, rho + (size_t)(k - m.rows) * 8);
        to_normal(w, from_normal<FrParams>(w));
    }
    store8(row, w);
    store8(row + 9 * vec, w);
}

// one lane per 16 bytes: four lanes copy one 64-byte record
__global__ __launch_bounds__(256) void points_take_every_kernel(uint4* dst, const uint4* src, u64 first, u64 step, u64 count) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 4) return;
    dst[i] = src[(first + (i >> 2) * step) * 4 + (i & 3)];
}

}  // namespace

void r1cs_fold(const R1csDev& m, const u32* rho, u32 n_public, u32 domain, u32* out, hipStream_t stream) {
    if (!domain) return;
    hipLaunchKernelGGL(r1cs_fold_kernel, dim3(grid_for(domain, 256)), dim3(256), 0, stream, m, rho, n_public, domain, out);
    UG_KERNEL_CHECK();
}
void r1cs_fold_classes(const R1csDev& m, const u32* rho, const uint8_t* cls, u32 n_public, u32 domain, u32* out, hipStream_t stream) {
    if (!domain) return;
    hipLaunchKernelGGL(r1cs_fold_classes_kernel, dim3(grid_for(domain, 256)), dim3(256), 0, stream, m, rho, cls, n_public, domain, out);
    UG_KERNEL_CHECK();
}
void points_take_every(u32* dst, const u32* src, u64 first, u64 step, u64 count, hipStream_t stream) {
    if (!count) return;
    hipLaunchKernelGGL(points_take_every_kernel, dim3(grid_for(count * 4, 256)), dim3(256), 0, stream, reinterpret_cast<uint4*>(dst),
                       reinterpret_cast<const uint4*>(src), first, step, count);
    UG_KERNEL_CHECK();
}

}  // namespace ug

// ---- the sums of the relations on one device, through the library's own interface ----------------------------------------------
namespace ughost {
namespace zkv {

namespace {

using ug::u64;

void must(int rc) { if (rc != UG_OK) throw std::runtime_error(std::string("zkey: ") + ug_last_error()); }

// whatever a failing step leaves behind is freed here
struct Dev {
    ug_ctx* c = nullptr;
    ug_r1cs* r = nullptr;
    ug_dvec *rho = nullptr, *sigma = nullptr, *fold = nullptr, *cls = nullptr, *rhoList = nullptr;
    ug_schedule* s = nullptr;
    ug_bases* set[4] = {nullptr, nullptr, nullptr, nullptr};
    u64 base = 0, peak = 0;
    ~Dev() {
        for (ug_bases*& b : set) drop(b);
        ug_schedule_destroy(s);
        ug_dvec_destroy(fold); ug_dvec_destroy(sigma); ug_dvec_destroy(rho); ug_dvec_destroy(cls); ug_dvec_destroy(rhoList);
        ug_r1cs_destroy(r);
        ug_ctx_destroy(c);
    }
    static void drop(ug_bases*& b) { if (b) ug_bases_destroy(b); b = nullptr; }
    u64 used() {
        uint64_t free = 0, total = 0;
        must(ug_ctx_mem_info(c, &free, &total));
        return total - free;
    }
    void sample() { const u64 u = used(); if (u > base) peak = std::max(peak, u - base); }
};

void openDevice(Dev& d, int device) {
    must(ug_ctx_create(&d.c, device));
    d.base = d.used();
}
// the circuit, the weights and the 3 K + 2 vectors of the fold on the device. cls null: a Groth16 key's two classes, eight vectors;
// cls a byte per wire: an UltraGroth key's three, eleven vectors, the bytes packed 32 to a vector element and gone after the kernel
void foldOn(Dev& d, const void* r1cs, uint64_t r1csSize, const uint8_t* rho, const uint8_t* cls, u64 M, uint32_t nPublic, uint32_t logN,
            double* kernelMs) {
    const u64 N = 1ull << logN, vectors = cls ? 11 : 8;
    must(ug_r1cs_create(d.c, r1cs, r1csSize, &d.r));
    must(ug_dvec_create(d.c, M, &d.rho));
    must(ug_dvec_upload(d.rho, rho, M));
    if (cls) {
        const u64 words = (M + 31) / 32;
        std::vector<uint8_t> padded(words * 32, 0);
        memcpy(padded.data(), cls, M);
        must(ug_dvec_create(d.c, words, &d.cls));
        must(ug_dvec_upload(d.cls, padded.data(), words));
    }
    must(ug_dvec_create(d.c, vectors * N, &d.fold));
    must(cls ? ug_r1cs_fold_classes_dvec(d.r, d.rho, d.cls, nPublic, logN, d.fold, kernelMs)
             : ug_r1cs_fold_dvec(d.r, d.rho, nPublic, logN, d.fold, kernelMs));
    d.sample();
    ug_r1cs_destroy(d.r);
    d.r = nullptr;
    ug_dvec_destroy(d.cls);
    d.cls = nullptr;
}

void sumsOn(int device, const Inputs& in, Sums& out, SumsStats& st) {
    ughost::setup::PhaseClock clock(st.ms);
    const u64 N = in.N, M = in.M, pub = in.pub;
    const int K = in.K;
    const u64 a = 3 * (u64)K * N, b = a + N;                         // where the fold's a and b start
    Dev d;
    openDevice(d, device);
    foldOn(d, in.r1cs, in.r1csSize, in.rho, in.cls, M, (uint32_t)(pub - 1), (uint32_t)in.logN, &st.foldKernelMs);
    must(ug_schedule_create(d.c, &d.s));
    clock.lap(0);

    // the slices: T, T2, aT, bT stay until the scalar side is done. Scalar i of a schedule built at `first` multiplies record i.
    must(ug_bases_create_g1(d.c, in.T, N, 0, &d.set[0]));
    must(ug_bases_create_g2(d.c, in.T2, N, 0, &d.set[1]));
    must(ug_bases_create_g1(d.c, in.aT, N, 0, &d.set[2]));
    must(ug_bases_create_g1(d.c, in.bT, N, 0, &d.set[3]));
    d.sample();
    must(ug_schedule_build(d.s, d.fold, a, N));                      // a
    must(ug_msm_g1(d.c, d.set[0], d.s, (int64_t)a, out.aT));
    {
        must(ug_schedule_build(d.s, d.fold, b, N));                  // b over T and, in G2, T2: one schedule, two base sets
        const ug_bases* both[2] = {d.set[0], d.set[1]};
        const int64_t shifts[2] = {(int64_t)b, (int64_t)b};
        void* outs[2] = {out.bT, out.bT2};
        must(ug_msm_batch(d.c, 2, both, d.s, shifts, outs));
    }
    for (int m = 0; m < K; m++) {                                    // K^m = MSM(a^m, bT) + MSM(b^m, aT) + MSM(c^m, T)
        uint8_t part[3][64];
        const ug_bases* over[3] = {d.set[3], d.set[2], d.set[0]};
        for (int v = 0; v < 3; v++) {
            const u64 first = (u64)(3 * m + v) * N;
            must(ug_schedule_build(d.s, d.fold, first, N));
            must(ug_msm_g1(d.c, over[v], d.s, (int64_t)first, part[v]));
        }
        const uint32_t colPtr[2] = {0, 3}, index[3] = {0, 1, 2};
        uint8_t ones[3][32] = {{1}, {1}, {1}};
        ughost::setup::PointSegs p;
        p.base[0] = part[0]; p.count = 3; p.n = 1;
        ughost::setup::hostBackend().combine(false, 1, colPtr, index, ones[0], p, out.k[m], nullptr);
    }
    d.sample();
    for (ug_bases*& bs : d.set) Dev::drop(bs);
    ug_dvec_destroy(d.fold);
    d.fold = nullptr;
    must(ug_schedule_trim(d.s));
    clock.lap(1);

    // the key's sections under rho, one at a time
    must(ug_schedule_build(d.s, d.rho, 0, M));
    struct Sec { const uint8_t* p; bool g2; uint8_t* out; };
    const Sec secs[3] = {{in.a, false, out.keyA}, {in.b1, false, out.keyB1}, {in.b2, true, out.keyB2}};
    for (const Sec& sc : secs) {
        must(sc.g2 ? ug_bases_create_g2(d.c, sc.p, M, 0, &d.set[0]) : ug_bases_create_g1(d.c, sc.p, M, 0, &d.set[0]));
        d.sample();
        must(sc.g2 ? ug_msm_g2(d.c, d.set[0], d.s, 0, sc.out) : ug_msm_g1(d.c, d.set[0], d.s, 0, sc.out));
        d.sample();
        Dev::drop(d.set[0]);
    }
    must(ug_schedule_build(d.s, d.rho, 0, pub));                     // rho^pub over IC
    must(ug_bases_create_g1(d.c, in.ic, pub, 0, &d.set[0]));
    must(ug_msm_g1(d.c, d.set[0], d.s, 0, out.keyIC));
    Dev::drop(d.set[0]);
    for (int i = 0; i < K - 1; i++) {                                // each C section under its weights
        const CSection& sc = in.c[i];
        memset(out.keyC[i], 0, 64);
        if (!sc.n) continue;
        if (sc.rhoFirst >= 0) {                                      // rho's own run, in place: record 0 is wire rhoFirst
            must(ug_schedule_build(d.s, d.rho, (u64)sc.rhoFirst, sc.n));
        } else {                                                     // the weights of a list's signals, gathered on the host
            must(ug_dvec_create(d.c, sc.n, &d.rhoList));
            must(ug_dvec_upload(d.rhoList, sc.weights, sc.n));
            must(ug_schedule_build(d.s, d.rhoList, 0, sc.n));
        }
        must(ug_bases_create_g1(d.c, sc.points, sc.n, sc.rhoFirst >= 0 ? (u64)sc.rhoFirst : 0, &d.set[0]));
        d.sample();
        must(ug_msm_g1(d.c, d.set[0], d.s, 0, out.keyC[i]));
        Dev::drop(d.set[0]);
        ug_dvec_destroy(d.rhoList);
        d.rhoList = nullptr;
    }
    clock.lap(2);

    // sigma over H and over the odd records of the padded level: one schedule, two base sets
    must(ug_dvec_create(d.c, N, &d.sigma));
    must(ug_dvec_upload(d.sigma, in.sigma, N));
    must(ug_schedule_build(d.s, d.sigma, 0, N));
    must(ug_bases_create_g1(d.c, in.h, N, 0, &d.set[0]));
    must(ug_bases_create_every_g1(d.c, in.top, 2 * N, 1, 2, 0, &d.set[1]));
    d.sample();
    {
        const ug_bases* both[2] = {d.set[0], d.set[1]};
        void* outs[2] = {out.keyH, out.hP};
        must(ug_msm_batch(d.c, 2, both, d.s, nullptr, outs));
    }
    d.sample();
    clock.lap(3);
    st.peakDeviceBytes = d.peak;
}

void foldDevice(int device, const void* r1cs, uint64_t r1csSize, const uint8_t* rho, const uint8_t* cls, uint32_t nPublic, uint32_t logN,
                uint8_t* out, double* kernelMs) {
    ug_r1cs_info info;
    must(ug_r1cs_parse_info(r1cs, r1csSize, &info));
    Dev d;
    openDevice(d, device);
    foldOn(d, r1cs, r1csSize, rho, cls, info.n_wires, nPublic, logN, kernelMs);
    must(ug_dvec_download(d.fold, out, 0, (cls ? 11ull : 8ull) << logN));
}

struct Register {
    Register() { deviceSums = sumsOn; deviceFold = foldDevice; }
} registerDevice;

}  // namespace
}  // namespace zkv
}  // namespace ughost
