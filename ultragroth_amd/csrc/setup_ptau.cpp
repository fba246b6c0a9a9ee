// setup_ptau.cpp -- the phase-2 setup from a prepared powers-of-tau file (include/ultragroth_hip.h: ug_ptau_parse_info,
// ug_setup_ptau_*, ug_points_combine, ug_points_scale): what `snarkjs zkey new` does for a Groth16 circuit, then optionally one
// delta contribution. No trapdoor is known here. Out of scope: UltraGroth keys, contribution transcripts, beacons, verifying the
// .ptau's own ceremony.
//
// The .ptau reader is host_util.cpp's; the circuit, the column index, section 4, the headers and the JSON are setup_host.cpp's,
// shared, not copied. What is new is the order of work: a real setup has no scalars per wire, it combines POINTS per wire
// (Backend::combine) and multiplies the private C points and H by 1 / delta (Backend::scale). K_s is one combination over the
// three level-n slices side by side: an A term (k, s) names bT[k], a B term aT[k], a C term T[k].
#include "setup_host.hpp"

#include <algorithm>
#include <memory>

namespace ughost {
namespace setup {

using namespace ug;

namespace {

constexpr int PTAU_PHASES = UG_SETUP_PTAU_PHASES;

// ---- the point check on host threads (device = -1): the rules of check.hip, in its order ----
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
    bool zero = true;
    for (int i = 0; i < 32 * coords; i++) zero &= rec[i] == 0;
    if (zero) return UG_POINT_OK;
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

// the device's check, through the library's own entry (ug_points_check uploads in bounded pieces and leaves nothing resident)
PtauPointCheck::PtauPointCheck(int device, int level) : device_(device), level_(level) {
    if (level_ && device_ >= 0 && ug_ctx_create(&ctx_, device_) != UG_OK) throw SetupError(ug_last_error());
}
PtauPointCheck::~PtauPointCheck() { if (ctx_) ug_ctx_destroy(ctx_); }
ug_point_fault PtauPointCheck::find(bool g2, const uint8_t* rec, u64 n) const {
    ug_point_fault f{0, UG_POINT_OK};
    if (!level_ || !n) return f;
    if (device_ < 0) f = hostCheck(g2, rec, n, level_);
    else if (ug_points_check(ctx_, g2 ? 1 : 0, rec, n, level_, &f) != UG_OK) throw SetupError(ug_last_error());
    return f;
}
const char* PtauPointCheck::reasonText(int reason) {
    return reason == UG_POINT_UNREDUCED ? "coordinate not below the field modulus"
         : reason == UG_POINT_OFF_CURVE ? "not on the curve" : "not in the subgroup of order r";
}
void PtauPointCheck::operator()(bool g2, const uint8_t* rec, u64 n, u32 id, u64 first, u64 stride) const {
    const ug_point_fault f = find(g2, rec, n);
    if (f.reason) throw PtauError("section " + std::to_string(id) + " point " + std::to_string(first + stride * f.index) + ": " + reasonText(f.reason));
}

namespace {

void checkOptions(const ug_setup_ptau_options* o) {
    if (!o) throw SetupError("null options");
    if (o->size != sizeof(ug_setup_ptau_options)) throw SetupError("options struct of another size (" + std::to_string(o->size) + ")");
    if (o->validate > 2) throw SetupError("validate " + std::to_string(o->validate) + " is not 0, 1 or 2");
    if (o->contribute > 2) throw SetupError("contribute " + std::to_string(o->contribute) + " is not 0, 1 or 2");
    if (o->contribute == 1) {
        if (!belowR(o->delta)) throw SetupError("delta is not below the field modulus");
        bool zero = true;
        for (int i = 0; i < 32; i++) zero &= o->delta[i] == 0;
        if (zero) throw SetupError("delta is 0 mod r");
    }
}

// a delta and its inverse that are wiped when they go
struct Delta {
    uint8_t value[32], inverse[32];
    bool one = true;
    Delta() { memset(value, 0, 32); memset(inverse, 0, 32); value[0] = inverse[0] = 1; }
    ~Delta() { wipe(value); wipe(inverse); }
    static void wipe(uint8_t* p) {
        volatile uint8_t* v = p;
        for (int i = 0; i < 32; i++) v[i] = 0;
    }
    void set(const uint8_t* le) {
        memcpy(value, le, 32);
        Fr d = frFromPlain(value);
        Fr di = cond_sub_q(inv(d));
        frToPlain(inverse, di);
        one = equal(d, fp_one<FrParams>());
        volatile u32* w = d.l;
        for (int i = 0; i < NL; i++) w[i] = 0;
        w = di.l;
        for (int i = 0; i < NL; i++) w[i] = 0;
    }
    void draw() {                                // uniform below r, never 0
        uint8_t d[32];
        for (;;) {
            randomBytes(d, 32);
            d[31] &= 0x3f;
            bool zero = true;
            for (int i = 0; i < 32; i++) zero &= d[i] == 0;
            if (!zero && belowR(d)) break;
        }
        set(d);
        wipe(d);
    }
};

// K's columns: wire s lists its A terms (points bT, segment 2), its B terms (aT, segment 1) and its C terms (T, segment 0)
void mergedColumns(const ColMatrix cm[3], u64 M, u64 N, std::vector<u32>& colPtr, std::vector<u32>& index, std::vector<uint8_t>& coefs) {
    const u64 terms = cm[0].terms() + cm[1].terms() + cm[2].terms();
    if (terms > 0xfffffff0ull) throw SetupError("sizes that cannot be represented: more than 2^32 - 16 terms in A, B and C together");
    colPtr.assign((size_t)M + 1, 0);
    for (u64 s = 0; s < M; s++) {
        u64 n = 0;
        for (int m = 0; m < 3; m++) n += cm[m].colPtr[s + 1] - cm[m].colPtr[s];
        colPtr[s + 1] = colPtr[s] + (u32)n;
    }
    index.resize(terms);
    coefs.resize(terms * 32);
    const u32 seg[3] = {2, 1, 0};
    parallelFor(M, 4096, [&](u64 lo, u64 hi) {
        for (u64 s = lo; s < hi; s++) {
            u32 at = colPtr[s];
            for (int m = 0; m < 3; m++)
                for (u32 q = cm[m].colPtr[s]; q < cm[m].colPtr[s + 1]; q++, at++) {
                    index[at] = (u32)(seg[m] * N + cm[m].row[q]);
                    memcpy(&coefs[(size_t)at * 32], &cm[m].val[(size_t)q * 32], 32);
                }
        }
    });
}

u64 runPtau(const ug_setup_ptau_options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, int device, uint8_t* zkey,
            u64 zkeyCap, std::string* vkey, double ms[PTAU_PHASES], bool sizeOnly, u64* vkeyMax) {
    double t = nowMs();
    auto lap = [&](int phase) { const double n = nowMs(); ms[phase] += n - t; t = n; };
    for (int i = 0; i < PTAU_PHASES; i++) ms[i] = 0;
    checkOptions(opt);
    std::unique_ptr<BinFile> f;
    R1cs cs;
    loadCircuit(r1cs, r1csSize, f, cs.hdr);
    Plan p;
    planSizes(cs.hdr, opt->log_domain, p);
    // every rule of the .ptau before the constraints are walked, and before the first device byte
    if (!ptau) throw PtauError("null ptau buffer");
    std::unique_ptr<BinFile> pf;
    try {
        pf.reset(new BinFile(ptau, ptauSize, "ptau", 1));
    } catch (const std::exception& e) {
        throw PtauError(e.what());
    }
    const PtauHeader ph = loadPtauHeader(*pf);
    const PtauSlices sl = loadPtauSlices(*pf, ph, (u32)p.logN);
    loadR1cs(*f, cs);
    std::vector<u64> perPiece;
    countCoefs(cs, perPiece);
    u64 nCoefs = (u64)p.nPublic + 1;
    for (u64 n : perPiece) nCoefs += n;
    const Layout lay = makeLayout(p, nCoefs);
    if (vkeyMax) *vkeyMax = vkeyBound(p);
    if (sizeOnly) return lay.total;
    if (!zkey) throw SetupError("null zkey buffer");
    if (zkeyCap < lay.total) throw SetupError("the zkey buffer is too small: " + std::to_string(lay.total) + " bytes are needed");
    std::unique_ptr<Backend> owned;
    Backend& be = backendFor(device, owned);
    ColMatrix cm[3];
    std::vector<Piece> pieces;                   // (the backends cut their columns by the same rule: columnPieces)
    buildColumns(cs, p, cm, pieces);
    const u64 N = p.N, M = p.nVars, pub = (u64)p.nPublic + 1;
    // H's sources: the odd records of level n + 1, side by side
    uint8_t* hOut = zkey + lay.offsetOf(9);
    writeContainer(zkey, lay);
    parallelFor(N, 4096, [&](u64 lo, u64 hi) {
        for (u64 k = lo; k < hi; k++) memcpy(hOut + k * 64, sl.top + (2 * k + 1) * 64, 64);
    });
    lap(0);

    {
        const PtauPointCheck check(device, (int)opt->validate);
        check(false, sl.tau1, N, 12, sl.first, 1);
        check(true, sl.tau2, N, 13, sl.first, 1);
        check(false, sl.alphaTau1, N, 14, sl.first, 1);
        check(false, sl.betaTau1, N, 15, sl.first, 1);
        check(false, hOut, N, 12, sl.firstTop + 1, 2);
        check(false, sl.alpha1, 1, 4, 0, 1);
        check(false, sl.beta1, 1, 5, 0, 1);
        check(true, sl.beta2, 1, 6, 0, 1);
    }
    lap(1);

    double kms[2];
    PointSegs one;
    one.count = N; one.n = 1;
    std::vector<uint8_t> krec(M * 64);
    one.base[0] = sl.tau1;
    be.combine(false, M, cm[0].colPtr.data(), cm[0].row.data(), cm[0].val.data(), one, zkey + lay.offsetOf(5), kms);
    be.combine(false, M, cm[1].colPtr.data(), cm[1].row.data(), cm[1].val.data(), one, zkey + lay.offsetOf(6), kms);
    {
        std::vector<u32> colPtr, index;
        std::vector<uint8_t> coefs;
        mergedColumns(cm, M, N, colPtr, index, coefs);
        PointSegs three;
        three.count = N; three.n = 3;
        three.base[0] = sl.tau1; three.base[1] = sl.alphaTau1; three.base[2] = sl.betaTau1;
        be.combine(false, M, colPtr.data(), index.data(), coefs.data(), three, krec.data(), kms);
    }
    lap(2);
    one.base[0] = sl.tau2;
    be.combine(true, M, cm[1].colPtr.data(), cm[1].row.data(), cm[1].val.data(), one, zkey + lay.offsetOf(7), kms);
    lap(3);

    Delta delta;
    if (opt->contribute == 1) delta.set(opt->delta);
    else if (opt->contribute == 2) delta.draw();
    if (!delta.one) {                            // the private C points and H, one launch: (1 / delta) * each
        const u64 nc = M - pub;
        std::vector<uint8_t> in((nc + N) * 64), out((nc + N) * 64);
        if (nc) memcpy(in.data(), &krec[pub * 64], nc * 64);
        memcpy(in.data() + nc * 64, hOut, N * 64);
        be.scale(delta.inverse, in.data(), nc + N, out.data(), kms);
        if (nc) memcpy(&krec[pub * 64], out.data(), nc * 64);
        memcpy(hOut, out.data() + nc * 64, N * 64);
    }
    lap(4);

    HeaderPoints hp;
    memset(&hp, 0, sizeof hp);
    {
        uint8_t sc[2][32];
        memset(sc, 0, sizeof sc);
        sc[0][0] = 1;                            // gamma = 1: the generator
        memcpy(sc[1], delta.value, 32);
        uint8_t g1[2][64], g2[2][128];
        hostBackend().generatorMul(false, sc[0], 2, 0, g1[0], nullptr);
        hostBackend().generatorMul(true, sc[0], 2, 0, g2[0], nullptr);
        Delta::wipe(sc[1]);
        memcpy(hp.g1[0], sl.alpha1, 64); memcpy(hp.g1[1], sl.beta1, 64); memcpy(hp.g1[3], g1[1], 64);
        memcpy(hp.g2[0], sl.beta2, 128); memcpy(hp.g2[1], g2[0], 128); memcpy(hp.g2[3], g2[1], 128);
    }
    finishKey(cs, p, lay, perPiece, hp, krec, zkey, vkey);
    lap(5);
    return lay.total;
}

std::string prefixed(const std::string& m) {
    return m.rfind("setup: ", 0) == 0 || m.rfind("r1cs: ", 0) == 0 || m.rfind("ptau: ", 0) == 0 ? m : "setup: " + m;
}

void checkColumns(const u32* colPtr, u64 nCols, const u32* index, const uint8_t* coefs, u64 nPoints) {
    if (nCols > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 columns");
    if (!colPtr || colPtr[0] != 0) throw SetupError("col_ptr does not start at 0");
    for (u64 c = 0; c < nCols; c++)
        if (colPtr[c + 1] < colPtr[c]) throw SetupError("col_ptr descends at column " + std::to_string(c));
    const u64 terms = colPtr[nCols];
    if (terms > 0xfffffff0ull) throw SetupError("sizes that cannot be represented: more than 2^32 - 16 terms");
    if (terms && (!index || !coefs)) throw SetupError("null buffer");
    for (u64 t = 0; t < terms; t++) {
        if (index[t] >= nPoints) throw SetupError("term " + std::to_string(t) + ": point " + std::to_string(index[t]) + " out of range");
        if (!belowR(coefs + t * 32)) throw SetupError("coefficient " + std::to_string(t) + " is not below the field modulus");
    }
}

}  // namespace
}  // namespace setup
}  // namespace ughost

// =====================================================================================================================
using namespace ughost::setup;

#define PTAU_TRY try {
#define PTAU_CATCH                                                                         \
    } catch (std::exception& e) { copyErr(error_msg, error_msg_maxsize, prefixed(e.what()).c_str()); return UG_ERROR; } \
    catch (...) { copyErr(error_msg, error_msg_maxsize, "setup: unknown error"); return UG_ERROR; }   \
    return UG_OK;

extern "C" {

int ug_ptau_parse_info(const void* ptau, uint64_t ptau_size, ug_ptau_info* out, char* error_msg, unsigned long long error_msg_maxsize) {
    PTAU_TRY
    if (!ptau || !out) throw PtauError("null buffer");
    std::unique_ptr<ughost::BinFile> f;
    try {
        f.reset(new ughost::BinFile(ptau, ptau_size, "ptau", 1));
    } catch (const std::exception& e) {
        throw PtauError(e.what());
    }
    const ughost::PtauHeader h = ughost::loadPtauHeader(*f);
    out->power = h.power; out->ceremony_power = h.ceremonyPower; out->prepared = h.prepared ? 1 : 0;
    out->max_log_domain = 0;
    if (h.prepared)                              // the largest n whose slices the sections hold
        for (u32 n = std::min<u32>(h.power, MAX_LOG_DOMAIN); n >= 1; n--) {
            try { ughost::loadPtauSlices(*f, h, n); out->max_log_domain = n; break; } catch (const std::exception&) {}
        }
    PTAU_CATCH
}

int ug_setup_ptau_size(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                       uint64_t* zkey_bytes, uint64_t* vkey_bytes_max, char* error_msg, unsigned long long error_msg_maxsize) {
    PTAU_TRY
    double ms[PTAU_PHASES];
    u64 vmax = 0;
    const u64 total = runPtau(opt, r1cs, r1cs_size, ptau, ptau_size, -1, nullptr, 0, nullptr, ms, true, &vmax);
    if (zkey_bytes) *zkey_bytes = total;
    if (vkey_bytes_max) *vkey_bytes_max = vmax;
    PTAU_CATCH
}

int ug_setup_ptau_run(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                      int device, void* zkey, uint64_t zkey_capacity, uint64_t* zkey_bytes, char* vkey_json, uint64_t vkey_capacity,
                      uint64_t* vkey_bytes, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    PTAU_TRY
    double ms[PTAU_PHASES];
    std::string vkey;
    const u64 total = runPtau(opt, r1cs, r1cs_size, ptau, ptau_size, device, (uint8_t*)zkey, zkey_capacity, &vkey, ms, false, nullptr);
    if (zkey_bytes) *zkey_bytes = total;
    if (vkey_bytes) *vkey_bytes = vkey.size();
    if (vkey_json) {
        if (vkey_capacity < vkey.size() + 1) throw SetupError("the verification-key buffer is too small: " + std::to_string(vkey.size() + 1) + " bytes are needed");
        memcpy(vkey_json, vkey.c_str(), vkey.size() + 1);
    }
    if (phase_ms) for (int i = 0; i < PTAU_PHASES; i++) phase_ms[i] = ms[i];
    PTAU_CATCH
}

int ug_points_combine(int device, int g2, const uint32_t* col_ptr, uint64_t n_cols, const uint32_t* index, const void* coefs,
                      const void* points, uint64_t n_points, void* out, double* kernel_ms, char* error_msg,
                      unsigned long long error_msg_maxsize) {
    PTAU_TRY
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
    if (!n_cols) return UG_OK;
    if (!out || (n_points && !points)) throw SetupError("null buffer");
    if (n_points > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
    checkColumns(col_ptr, n_cols, index, (const uint8_t*)coefs, n_points);
    PointSegs pts;
    pts.base[0] = (const uint8_t*)points; pts.count = n_points; pts.n = 1;      // (no points: checkColumns has refused every term)
    std::unique_ptr<Backend> owned;
    backendFor(device, owned).combine(g2 != 0, n_cols, col_ptr, index, (const uint8_t*)coefs, pts, (uint8_t*)out, kernel_ms);
    PTAU_CATCH
}

int ug_points_scale(int device, const void* scalar, const void* points, uint64_t n, void* out, double* kernel_ms, char* error_msg,
                    unsigned long long error_msg_maxsize) {
    PTAU_TRY
    if (kernel_ms) kernel_ms[0] = 0;
    if (!scalar || (n && (!points || !out))) throw SetupError("null buffer");
    if (!belowR((const uint8_t*)scalar)) throw SetupError("scalar is not below the field modulus");
    if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
    if (!n) return UG_OK;
    std::unique_ptr<Backend> owned;
    backendFor(device, owned).scale((const uint8_t*)scalar, (const uint8_t*)points, n, (uint8_t*)out, kernel_ms);
    PTAU_CATCH
}

}  // extern "C"
