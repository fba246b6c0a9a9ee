// r1cs.hip -- the witness check against a circuit's .r1cs, and the probe that says whether an .r1cs is the circuit of a zkey.
//
// A zkey holds the A and B matrices only (section 4; the prover sets c = a o b itself, hpoly.hip), so a witness that breaks a
// constraint gives a proof that never verifies and nothing says which constraint. The .r1cs has C. Its three matrices are kept
// as three CSR triples in CoefMatrix's form -- row_ptr, sig, val = coef * 2^522 packed -- so that matvec_row (dev_common.hpp)
// serves as it is: one lane sums the three rows of one constraint and compares (A.w)(B.w) with C.w, both fully reduced.
// The rules are the H block's: the witness is plain 32-byte integers, any value below 2^256, taken mod r by the product.
// No LDS; plain C++ and vector stores only.
#include "dev_common.hpp"
#include "internal.hpp"

namespace ug {

namespace {

// plain coefficients (as the file has them, below r) -> coef * 2^522, packed, in place: from_normal gives coef * 2^261 and the
// product with r2 = 2^522 another factor 2^261 (a zkey's section 4 stores coef * 2^512 instead: coef_gather_kernel, hpoly.hip)
__global__ void r1cs_coef_kernel(u32* val, u64 n) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    load8(w, val + i * 8);
    st_packed(val + i * 8, cond_sub_q(mul(from_normal<FrParams>(w), fp_from<FrParams>(FrParams::r2))));
}

__device__ __forceinline__ bool same_limbs(const Fr& x, const Fr& y) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= x.l[i] ^ y.l[i];
    return o == 0;
}

// One lane per constraint. words[0] counts the failing constraints, words[1] keeps ~(lowest failing index) under atomicMax
// (both start as 0, one memset); mask (optional): one byte per constraint, 0 holds, 1 fails.
// canon() on both sides: matvec_row leaves a representative below 2.01 q, the product one below 2 q, and a lazy representative
// of the same residue must not count as a failure.
__global__ __launch_bounds__(256) void r1cs_check_kernel(R1csDev m, const u32* wtns, unsigned long long* words, uint8_t* mask) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m.rows) return;
    const Fr a = matvec_row(k, m.row_ptr[0], m.sig[0], m.val[0], wtns);
    const Fr b = matvec_row(k, m.row_ptr[1], m.sig[1], m.val[1], wtns);
    const Fr lhs = canon(mul(a, b));                            // a, b < 2.01 q: (a/q)(b/q) < 169
    const Fr c = matvec_row(k, m.row_ptr[2], m.sig[2], m.val[2], wtns);
    const bool bad = !same_limbs(lhs, canon(c));
    if (mask) mask[k] = bad ? 1 : 0;
    if (bad) {
        atomicAdd(&words[0], 1ull);
        atomicMax(&words[1], ~(unsigned long long)k);
    }
}

// The same for the V witnesses of a batched pass: one lane per constraint and group of VT witnesses (blockIdx.y; the last group has
// live < VT), so a row's signal ids and coefficients are read once per group. The matrices one after the other -- a[VT], b[VT],
// lhs[v] = canon(mul(a, b)) in a's place, then c[VT] --: matvec_row_vectors gives every accumulator the additions and contractions
// of matvec_row for its witness, so failed, first and the status bytes of every witness are r1cs_check_kernel's, bit for bit.
// Witness v at wtns + v * wstride words; its two words at words + 2 v, its status bytes (optional) at mask + v * rows.
// VT = 1, 2 and 4 compile without scratch, at 159, 214 and 314 + 58 accumulation registers: four witnesses leave one wave per SIMD
// and measure 1.4x the time of two (profiles/registry_batch.txt), so launches take two per lane (r1cs_vectors_group).
template <int VT>
__global__ __launch_bounds__(256) void r1cs_check_vectors_kernel(R1csDev m, const u32* wtns, u64 wstride, int vectors, unsigned long long* words,
                                                                 uint8_t* mask) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m.rows) return;
    const int v0 = (int)blockIdx.y * VT, live = vectors - v0 < VT ? vectors - v0 : VT;
    const u32* w0 = wtns + (size_t)v0 * wstride;
    Fr lhs[VT], x[VT];
    matvec_row_vectors<VT>(lhs, k, m.row_ptr[0], m.sig[0], m.val[0], w0, wstride, live);
    matvec_row_vectors<VT>(x, k, m.row_ptr[1], m.sig[1], m.val[1], w0, wstride, live);
    for_each_vector<0, VT>([&](auto vc) __attribute__((always_inline)) {
        constexpr int v = decltype(vc)::value;
        lhs[v] = canon(mul(lhs[v], x[v]));                          // a, b < 2.01 q: (a/q)(b/q) < 169
    });
    matvec_row_vectors<VT>(x, k, m.row_ptr[2], m.sig[2], m.val[2], w0, wstride, live);
    for_each_vector<0, VT>([&](auto vc) __attribute__((always_inline)) {
        constexpr int v = decltype(vc)::value;
        if (v < live) {
            const bool bad = !same_limbs(lhs[v], canon(x[v]));
            if (mask) mask[(size_t)(v0 + v) * m.rows + k] = bad ? 1 : 0;
            if (bad) {
                atomicAdd(&words[2 * (v0 + v)], 1ull);
                atomicMax(&words[2 * (v0 + v) + 1], ~(unsigned long long)k);
            }
        }
    });
}

// the three values of constraint k as canonical plain integers: out[0..8) = A.w, [8..16) = B.w, [16..24) = C.w (one lane)
__global__ void r1cs_row_kernel(R1csDev m, const u32* wtns, u32 k, u32* out) {
    if (blockIdx.x || threadIdx.x || k >= m.rows) return;
#pragma unroll 1
    for (int t = 0; t < 3; t++) {
        u32 w[8];
        to_normal(w, matvec_row(k, m.row_ptr[t], m.sig[t], m.val[t], wtns));
        store8(out + t * 8, w);
    }
}

// The probe: is this .r1cs the circuit the zkey's coefficient matrix was made for? One lane per row r of the zkey's domain and
// matrix t (blockIdx.y: 0 = A, 1 = B); z: n_wires pseudo-random plain values below r.
//   r < rows (the constraints)                 zkey row . z  ==  r1cs row . z, both canonical
//   rows <= r <= rows + n_public, matrix A     zkey row . z  ==  z[r - rows]           (snarkjs' public rows)
//   every other row                            empty in the zkey
// *word takes the lowest failing key 2 r + t under atomicMin (starts as all ones): the lowest row, A before B on one row.
__global__ __launch_bounds__(256) void r1cs_match_kernel(R1csDev m, const u32* z_row_ptr, const u32* z_sig, const u32* z_val, u32 domain,
                                                         u32 n_public, const u32* z, unsigned long long* word) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 t = blockIdx.y;
    if (r >= domain) return;
    const u32 zr = t * domain + r;
    bool bad;
    if (r < m.rows) {
        const Fr x = canon(matvec_row(zr, z_row_ptr, z_sig, z_val, z));
        const Fr y = canon(matvec_row(r, m.row_ptr[t], m.sig[t], m.val[t], z));
        bad = !same_limbs(x, y);
    } else if (t == 0 && r - m.rows <= n_public) {
        const Fr x = canon(matvec_row(zr, z_row_ptr, z_sig, z_val, z));
        u32 w[8];
        load8(w, z + (size_t)(r - m.rows) * 8);
        bad = !same_limbs(x, canon(from_normal<FrParams>(w)));
    } else {
        bad = z_row_ptr[zr + 1] != z_row_ptr[zr];
    }
    if (bad) atomicMin(word, 2ull * r + t);
}

}  // namespace

void r1cs_convert_coefs(u32* val, u64 n, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(r1cs_coef_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, val, n);
    UG_KERNEL_CHECK();
}
void r1cs_check(const R1csDev& m, const u32* wtns, unsigned long long* words, uint8_t* mask, hipStream_t stream) {
    UG_HIP(hipMemsetAsync(words, 0, 16, stream));
    if (!m.rows) return;
    hipLaunchKernelGGL(r1cs_check_kernel, dim3(grid_for(m.rows, 256)), dim3(256), 0, stream, m, wtns, words, mask);
    UG_KERNEL_CHECK();
}
template <int VT>
static void launch_check_vectors(const R1csDev& m, const u32* wtns, u64 wstride, int vectors, unsigned long long* words, uint8_t* mask, hipStream_t stream) {
    hipLaunchKernelGGL(r1cs_check_vectors_kernel<VT>, dim3(grid_for(m.rows, 256), (unsigned)((vectors + VT - 1) / VT)), dim3(256), 0, stream, m, wtns,
                       wstride, vectors, words, mask);
}
int r1cs_vectors_group(int vectors) {
    int vt = vectors >= R1CS_VT ? R1CS_VT : 1;
    if (const char* e = getenv("UG_R1CS_VT")) vt = atoi(e);                // tuning knob: 1, 2 or 4 give the same bytes
    return vt >= 4 ? 4 : vt >= 2 ? 2 : 1;
}
void r1cs_check_vectors(const R1csDev& m, const u32* wtns, u64 wstride, int vectors, unsigned long long* words, uint8_t* mask, hipStream_t stream) {
    UG_HIP(hipMemsetAsync(words, 0, (size_t)16 * vectors, stream));
    if (!m.rows) return;
    switch (r1cs_vectors_group(vectors)) {
        case 4: launch_check_vectors<4>(m, wtns, wstride, vectors, words, mask, stream); break;
        case 2: launch_check_vectors<2>(m, wtns, wstride, vectors, words, mask, stream); break;
        default: launch_check_vectors<1>(m, wtns, wstride, vectors, words, mask, stream);
    }
    UG_KERNEL_CHECK();
}
void r1cs_row_values(const R1csDev& m, const u32* wtns, u32 k, u32* out24, hipStream_t stream) {
    hipLaunchKernelGGL(r1cs_row_kernel, dim3(1), dim3(64), 0, stream, m, wtns, k, out24);
    UG_KERNEL_CHECK();
}
void r1cs_match(const R1csDev& m, const CoefMatrix& zk, u32 n_public, const u32* z, unsigned long long* word, hipStream_t stream) {
    UG_HIP(hipMemsetAsync(word, 0xff, 8, stream));
    hipLaunchKernelGGL(r1cs_match_kernel, dim3(grid_for(zk.domain, 256), 2), dim3(256), 0, stream, m, zk.row_ptr.get(), zk.sig.get(), zk.val.get(), zk.domain,
                       n_public, z, word);
    UG_KERNEL_CHECK();
}

}  // namespace ug
