// point_check.cpp -- the point check of a file's records (setup_host.hpp: PointCheck) for the phase-2 setup, the .ptau preparation
// and the key check, and what the two readers of a prepared .ptau do with its slices before they trust them.
//
// device >= 0 goes through the library's own entry (ug_points_check uploads in bounded pieces and leaves nothing resident);
// device = -1 runs the rules of check.hip, in its order, on host threads.
#include "setup_host.hpp"

namespace ughost {
namespace setup {

using namespace ug;

namespace {

bool rawBelowQ(const uint8_t* le) {
    for (int i = 31; i >= 0; i--) {
        if (le[i] < BN254_Q_LE[i]) return true;
        if (le[i] > BN254_Q_LE[i]) return false;
    }
    return false;
}
Fq coordOf(const uint8_t* le) {
    u32 w[8];
    memcpy(w, le, 32);
    return cond_sub_q(from_mont256<FqParams>(w));
}
Fq fqSmall(u32 v) {
    u32 w[8] = {v};
    return cond_sub_q(from_normal<FqParams>(w));
}
bool sameFq(const Fq& a, const Fq& b) { return equal(a, b); }
int hostCheckOne(bool g2, const uint8_t* rec, int level) {
    const int coords = g2 ? 4 : 2;
    if (allZero(rec, 32 * coords)) return UG_POINT_OK;
    for (int c = 0; c < coords; c++)
        if (!rawBelowQ(rec + 32 * c)) return UG_POINT_UNREDUCED;
    if (!g2) {
        const Fq x = coordOf(rec), y = coordOf(rec + 32);
        return sameFq(sqr(y), add(mul(sqr(x), x), fqSmall(3))) ? UG_POINT_OK : UG_POINT_OFF_CURVE;
    }
    Fq2 x, y, xi;
    x.a = coordOf(rec); x.b = coordOf(rec + 32); y.a = coordOf(rec + 64); y.b = coordOf(rec + 96);
    xi.a = fqSmall(9); xi.b = fp_one<FqParams>();
    const Fq2 b = canon(mul_fp(inv(xi), fqSmall(3)));              // 3 / (9 + u)
    const Fq2 lhs = canon(sqrk<1>(y)), rhs = canon(add(mulk<1>(sqrk<1>(x), x), b));
    if (!sameFq(lhs.a, rhs.a) || !sameFq(lhs.b, rhs.b)) return UG_POINT_OFF_CURVE;
    if (level >= 2 && !is_inf(xyzz_mul_scalar(xyzz_from_affine(x, y), FrParams::q32, 254))) return UG_POINT_OFF_SUBGROUP;
    return UG_POINT_OK;
}
ug_point_fault hostCheck(bool g2, const uint8_t* rec, u64 n, int level) {
    const u64 size = g2 ? 128 : 64;
    std::vector<ug_point_fault> first((size_t)((n + 255) / 256), ug_point_fault{0, UG_POINT_OK});
    parallelFor(n, 256, [&](u64 lo, u64 hi) {
        for (u64 i = lo; i < hi; i++) {
            const int reason = hostCheckOne(g2, rec + i * size, level);
            if (reason) { first[(size_t)(lo / 256)] = ug_point_fault{i, reason}; return; }
        }
    });
    for (const ug_point_fault& f : first)
        if (f.reason) return f;
    return ug_point_fault{0, UG_POINT_OK};
}

}  // namespace

PointCheck::PointCheck(int device, int level) : device_(device), level_(level) {
    if (level_ && device_ >= 0 && ug_ctx_create(&ctx_, device_) != UG_OK) throw SetupError(ug_last_error());
}
PointCheck::~PointCheck() { if (ctx_) ug_ctx_destroy(ctx_); }
ug_point_fault PointCheck::find(bool g2, const uint8_t* rec, u64 n) const {
    ug_point_fault f{0, UG_POINT_OK};
    if (!level_ || !n) return f;
    if (device_ < 0) f = hostCheck(g2, rec, n, level_);
    else if (ug_points_check(ctx_, g2 ? 1 : 0, rec, n, level_, &f) != UG_OK) throw SetupError(ug_last_error());
    return f;
}
const char* PointCheck::reasonText(int reason) {
    return reason == UG_POINT_UNREDUCED ? "coordinate not below the field modulus"
         : reason == UG_POINT_OFF_CURVE ? "not on the curve" : "not in the subgroup of order r";
}
void PointCheck::operator()(bool g2, const uint8_t* rec, u64 n, u32 id, u64 first, u64 stride) const {
    const ug_point_fault f = find(g2, rec, n);
    if (f.reason) throw PtauError("section " + std::to_string(id) + " point " + std::to_string(first + stride * f.index) + ": " + reasonText(f.reason));
}

void gatherOddTop(const PtauSlices& sl, uint8_t* out) {
    parallelFor(sl.n, 4096, [&](u64 lo, u64 hi) {
        for (u64 k = lo; k < hi; k++) memcpy(out + k * 64, sl.top + (2 * k + 1) * 64, 64);
    });
}

void checkSlices(const PointCheck& check, const PtauSlices& sl, const uint8_t* hOdd) {
    const u64 N = sl.n;
    check(false, sl.tau1, N, 12, sl.first, 1);
    check(true, sl.tau2, N, 13, sl.first, 1);
    check(false, sl.alphaTau1, N, 14, sl.first, 1);
    check(false, sl.betaTau1, N, 15, sl.first, 1);
    check(false, hOdd, N, 12, sl.firstTop + 1, 2);
    check(false, sl.alpha1, 1, 4, 0, 1);
    check(false, sl.beta1, 1, 5, 0, 1);
    check(true, sl.beta2, 1, 6, 0, 1);
}

}  // namespace setup
}  // namespace ughost
