// pairing.hip -- the device pass of batch verification: one Miller loop per lane, then the trees of partial products.
//
// miller_batch_kernel   lane i: r_i A_i (128-bit ladder, then affine), f_i = miller(B_i, r_i A_i), and r_i times the proof's
//                       other G1 points as XYZZ records. The arithmetic is pairing.hpp, the host verifier's own.
// f12_tree_kernel       one level of the binary tree over the f_i: node j = node 2j * node 2j+1 of the level below, an odd last
// g1_tree_kernel        node copied up; the G1 twin adds. One launch per level; every level stays in HBM, so that a rejected
//                       batch can be searched from the root without the device.
//
// Registers: an Fq12 value is 108 words, a product holds three and a column sum. The coefficient loops of pairing.hpp are
// kept as loops, so the values are indexed at run time and live in private (scratch) memory; the column products (81
// multiply-adds for 18 words read) run from registers. Every kernel asks for one wave per SIMD -- the whole 512-entry
// file -- so that nothing else is pushed out; tools/kernel_regs.py prints what the compiler made of it
// (profiles/verify_batch.txt).
#include "dev_common.hpp"
#include "pairing_dev.hpp"

namespace ug {

using namespace pr;

namespace {

#define UG_ONE_WAVE __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))

__global__ UG_ONE_WAVE void miller_batch_kernel(PairingConsts kc, const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ g,
                                                const u32* __restrict__ r, int n, int k, u32* __restrict__ f_out, u32* __restrict__ g_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) return;
    u32 rw[4];
#pragma unroll
    for (int j = 0; j < 4; j++) rw[j] = r[i * 4 + j];
    batch_leaf(kc, a + i * G1_WORDS, b + i * G2_WORDS, g + i * k * G1_WORDS, k, rw, f_out + i * F12_WORDS, g_out + i * k * XYZZ_WORDS);
}

__global__ UG_ONE_WAVE void f12_tree_kernel(PairingConsts kc, const u32* __restrict__ src, int n_src, u32* __restrict__ dst) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ((size_t)n_src + 1) / 2) return;
    f12_node(kc, src + 2 * j * F12_WORDS, 2 * j + 1 < (size_t)n_src ? src + (2 * j + 1) * F12_WORDS : nullptr, dst + j * F12_WORDS);
}

__global__ __launch_bounds__(64) void g1_tree_kernel(const u32* __restrict__ src, int n_src, int k, u32* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (((size_t)n_src + 1) / 2) * k) return;
    const size_t j = t / k, s = t % k;
    g1_node(src + (2 * j * k + s) * XYZZ_WORDS, 2 * j + 1 < (size_t)n_src ? src + ((2 * j + 1) * k + s) * XYZZ_WORDS : nullptr,
            dst + (j * k + s) * XYZZ_WORDS);
}

struct DevBuf {
    u32* p = nullptr;
    explicit DevBuf(size_t words) { UG_HIP(hipMalloc(&p, words * sizeof(u32))); }
    ~DevBuf() { if (p) hipFree(p); }
    DevBuf(const DevBuf&) = delete;
};
struct Event {
    hipEvent_t e = nullptr;
    Event() { UG_HIP(hipEventCreate(&e)); }
    ~Event() { if (e) hipEventDestroy(e); }
    Event(const Event&) = delete;
};
unsigned blocks(size_t lanes) { return (unsigned)((lanes + 63) / 64); }

}  // namespace

void pairing_batch_device(int device, const PairingConsts& kc, PairingBatch& pb) {
    if (pb.n <= 0 || pb.n > PAIRING_PASS || (pb.k != 1 && pb.k != 2)) throw std::invalid_argument("pairing_batch_device: bad shape");
    UG_HIP(hipSetDevice(device));
    const size_t n = (size_t)pb.n, k = (size_t)pb.k, nodes = tree_nodes(n);
    DevBuf a(n * G1_WORDS), b(n * G2_WORDS), g(n * k * G1_WORDS), r(n * 4), f(nodes * F12_WORDS), s(nodes * k * XYZZ_WORDS);
    Event t0, t1, t2, t3;
    UG_HIP(hipMemcpy(a.p, pb.a, n * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(b.p, pb.b, n * G2_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(g.p, pb.g, n * k * G1_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipMemcpy(r.p, pb.r, n * 4 * sizeof(u32), hipMemcpyHostToDevice));
    UG_HIP(hipEventRecord(t0.e, nullptr));
    hipLaunchKernelGGL(miller_batch_kernel, dim3(blocks(n)), dim3(64), 0, nullptr, kc, a.p, b.p, g.p, r.p, pb.n, pb.k, f.p, s.p);
    UG_KERNEL_CHECK();
    UG_HIP(hipEventRecord(t1.e, nullptr));
    size_t off = 0;
    for (size_t m = n; m > 1; m = (m + 1) / 2) {                    // level of m nodes at `off` -> (m + 1) / 2 nodes behind it
        hipLaunchKernelGGL(f12_tree_kernel, dim3(blocks((m + 1) / 2)), dim3(64), 0, nullptr, kc, f.p + off * F12_WORDS, (int)m, f.p + (off + m) * F12_WORDS);
        UG_KERNEL_CHECK();
        off += m;
    }
    UG_HIP(hipEventRecord(t2.e, nullptr));
    off = 0;
    for (size_t m = n; m > 1; m = (m + 1) / 2) {
        hipLaunchKernelGGL(g1_tree_kernel, dim3(blocks(((m + 1) / 2) * k)), dim3(64), 0, nullptr, s.p + off * k * XYZZ_WORDS, (int)m, pb.k, s.p + (off + m) * k * XYZZ_WORDS);
        UG_KERNEL_CHECK();
        off += m;
    }
    UG_HIP(hipEventRecord(t3.e, nullptr));
    UG_HIP(hipMemcpy(pb.f_tree, f.p, nodes * F12_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    UG_HIP(hipMemcpy(pb.g_tree, s.p, nodes * k * XYZZ_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    float ms[3] = {0, 0, 0};
    UG_HIP(hipEventElapsedTime(&ms[0], t0.e, t1.e));
    UG_HIP(hipEventElapsedTime(&ms[1], t1.e, t2.e));
    UG_HIP(hipEventElapsedTime(&ms[2], t2.e, t3.e));
    for (int i = 0; i < 3; i++) pb.kernel_ms[i] = ms[i];
}

}  // namespace ug
