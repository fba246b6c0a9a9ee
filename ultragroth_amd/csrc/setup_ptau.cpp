// setup_ptau.cpp -- the phase-2 setup from a prepared powers-of-tau file (include/ultragroth_hip.h: ug_ptau_parse_info,
// ug_setup_ptau_*, ug_points_combine, ug_points_scale, ug_points_ratio_mask): what `snarkjs zkey new` does for a Groth16 circuit, then optionally one
// delta contribution; and the same for an UltraGroth key (ug_ultra_setup_ptau_*, ug_points_scale_segments): two deltas, the C points
// in two sections by the caller's lists. No trapdoor is known here. Out of scope: contribution transcripts, beacons, verifying the
// .ptau's own ceremony.
//
// The .ptau reader is host_util.cpp's, the point check point_check.cpp's; the circuit, the column index, section 4, the headers and the JSON are setup_host.cpp's,
// shared, not copied. What is new is the order of work: a real setup has no scalars per wire, it combines POINTS per wire
// (Backend::combine) and multiplies the private C points and H by 1 / delta (Backend::scale; an UltraGroth key: C1 by 1 / delta_round,
// C2 and H by 1 / delta_final, gathered through the lists, Backend::scaleSegments). K_s is one combination over the three level-n
// slices side by side: an A term (k, s) names bT[k], a B term aT[k], a C term T[k].
#include "setup_host.hpp"

#include <algorithm>
#include <memory>

namespace ughost {
namespace setup {

using namespace ug;

namespace {

constexpr int PTAU_PHASES = UG_SETUP_PTAU_PHASES;

// what a run reads of either options struct; ultra: null for a Groth16 key
struct Request {
    u32 logDomain, validate, contribute;
    const uint8_t* deltaRound;                   // (an UltraGroth key only)
    const uint8_t* deltaFinal;
    const ug_ultra_setup_ptau_options* ultra;
};

// the contribution rule of both options structs: a given delta (contribute = 1) is below r and not 0, under the struct's name for it
struct NamedDelta { const char* name; const uint8_t* v; };
void checkContribution(u32 contribute, std::initializer_list<NamedDelta> deltas) {
    if (contribute > 2) throw SetupError("contribute " + std::to_string(contribute) + " is not 0, 1 or 2");
    if (contribute != 1) return;
    for (const NamedDelta& d : deltas) {
        if (!belowR(d.v)) throw SetupError(std::string(d.name) + " is not below the field modulus");
        if (allZero(d.v, 32)) throw SetupError(std::string(d.name) + " is 0 mod r");
    }
}
// every rule of the options, then what a run reads of them
Request requestOf(const ug_setup_ptau_options* o) {
    checkOptionsHead<SetupError>(o, 0, 2, "0, 1 or 2");
    checkContribution(o->contribute, {{"delta", o->delta}});
    return {o->log_domain, o->validate, o->contribute, nullptr, o->delta, nullptr};
}
Request requestOf(const ug_ultra_setup_ptau_options* o) {
    checkOptionsHead<SetupError>(o, 0, 2, "0, 1 or 2");
    checkContribution(o->contribute, {{"delta_round", o->delta_round}, {"delta_final", o->delta_final}});
    return {o->log_domain, o->validate, o->contribute, o->delta_round, o->delta_final, o};
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
    void draw() {
        uint8_t d[32];
        drawNonZeroScalar(d);
        set(d);
        wipe(d);
    }
    void contribute(u32 how, const uint8_t* given) {
        if (how == 1) set(given);
        else if (how == 2) draw();
    }
};

}  // namespace

// K's columns: column i is wire s = wires ? wires[i] : first + i, which lists its A terms (points bT, segment 2), its B terms (aT,
// segment 1) and its C terms (T, segment 0)
void mergedColumns(const ColMatrix cm[3], const u32* wires, u64 first, u64 M, u64 N, std::vector<u32>& colPtr, std::vector<u32>& index,
                   std::vector<uint8_t>& coefs) {
    auto wire = [&](u64 i) { return wires ? (u64)wires[i] : first + i; };
    colPtr.assign((size_t)M + 1, 0);
    u64 terms = 0;
    for (u64 i = 0; i < M; i++) {
        const u64 s = wire(i);
        for (int m = 0; m < 3; m++) terms += cm[m].colPtr[s + 1] - cm[m].colPtr[s];
        if (terms > 0xfffffff0ull) throw SetupError("sizes that cannot be represented: more than 2^32 - 16 terms in A, B and C together");
        colPtr[i + 1] = (u32)terms;
    }
    index.resize(terms);
    coefs.resize(terms * 32);
    const u32 seg[3] = {2, 1, 0};
    parallelFor(M, 4096, [&](u64 lo, u64 hi) {
        for (u64 i = lo; i < hi; i++) {
            const u64 s = wire(i);
            u32 at = colPtr[i];
            for (int m = 0; m < 3; m++)
                for (u32 q = cm[m].colPtr[s]; q < cm[m].colPtr[s + 1]; q++, at++) {
                    index[at] = (u32)(seg[m] * N + cm[m].row[q]);
                    memcpy(&coefs[(size_t)at * 32], &cm[m].val[(size_t)q * 32], 32);
                }
        }
    });
}

namespace {

u64 runPtau(const Request& rq, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, int device, uint8_t* zkey,
            u64 zkeyCap, std::string* vkey, double ms[PTAU_PHASES], bool sizeOnly, u64* vkeyMax) {
    PhaseClock clock(ms);
    std::unique_ptr<BinFile> f;
    R1cs cs;
    loadCircuit(r1cs, r1csSize, f, cs.hdr);
    Plan p;
    planSizes(cs.hdr, rq.logDomain, p);
    if (rq.ultra) planLists(p, rq.ultra->rand_indx, rq.ultra->round_signals, rq.ultra->n_round, rq.ultra->final_signals, rq.ultra->n_final);
    // every rule of the .ptau before the constraints are walked, and before the first device byte
    const std::unique_ptr<BinFile> pf = openBinFile(ptau, ptauSize, "ptau", "ptau: ", "null ptau buffer");
    const PtauHeader ph = loadPtauHeader(*pf);
    const PtauSlices sl = loadPtauSlices(*pf, ph, (u32)p.logN);
    loadR1cs(*f, cs);
    std::vector<u64> perPiece;
    const Layout lay = makeLayout(p, (u64)p.nPublic + 1 + countCoefs(cs, perPiece));
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
    uint8_t* hOut = zkey + lay.offsetOf(p.ultra ? 12 : 9);
    writeContainer(zkey, lay);
    gatherOddTop(sl, hOut);
    clock.lap(0);

    checkSlices(PointCheck(device, (int)rq.validate), sl, hOut);
    clock.lap(1);

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
        mergedColumns(cm, nullptr, 0, M, N, colPtr, index, coefs);
        PointSegs three;
        three.count = N; three.n = 3;
        three.base[0] = sl.tau1; three.base[1] = sl.alphaTau1; three.base[2] = sl.betaTau1;
        be.combine(false, M, colPtr.data(), index.data(), coefs.data(), three, krec.data(), kms);
    }
    clock.lap(2);
    one.base[0] = sl.tau2;
    be.combine(true, M, cm[1].colPtr.data(), cm[1].row.data(), cm[1].val.data(), one, zkey + lay.offsetOf(7), kms);
    clock.lap(3);

    Delta delta, deltaRound;                     // (the final delta: the only one of a Groth16 key)
    delta.contribute(rq.contribute, rq.deltaFinal);
    if (p.ultra) {                               // C1, C2 and H, one launch: the gather through the lists and (1 / its delta) * each
        deltaRound.contribute(rq.contribute, rq.deltaRound);
        ScaleSeg segs[3];
        segs[0].scalar = deltaRound.inverse; segs[0].src = krec.data(); segs[0].nSrc = M;
        segs[0].index = p.roundSignals.data(); segs[0].count = p.roundSignals.size(); segs[0].out = zkey + lay.offsetOf(8);
        segs[1].scalar = delta.inverse; segs[1].src = krec.data(); segs[1].nSrc = M;
        segs[1].index = p.finalSignals.data(); segs[1].count = p.finalSignals.size(); segs[1].out = zkey + lay.offsetOf(9);
        segs[2].scalar = delta.inverse; segs[2].src = hOut; segs[2].nSrc = N; segs[2].count = N; segs[2].out = hOut;
        be.scaleSegments(segs, 3, kms);
    } else if (!delta.one) {                     // the private C points and H, one launch: (1 / delta) * each
        const u64 nc = M - pub;
        std::vector<uint8_t> in((nc + N) * 64), out((nc + N) * 64);
        if (nc) memcpy(in.data(), &krec[pub * 64], nc * 64);
        memcpy(in.data() + nc * 64, hOut, N * 64);
        be.scale(delta.inverse, in.data(), nc + N, out.data(), kms);
        if (nc) memcpy(&krec[pub * 64], out.data(), nc * 64);
        memcpy(hOut, out.data() + nc * 64, N * 64);
    }
    clock.lap(4);

    HeaderPoints hp;
    memset(&hp, 0, sizeof hp);
    {
        uint8_t sc[3][32];
        memset(sc, 0, sizeof sc);
        sc[0][0] = 1;                            // gamma = 1: the generator
        memcpy(sc[1], delta.value, 32);
        memcpy(sc[2], deltaRound.value, 32);
        uint8_t g1[3][64], g2[3][128];
        const u64 nsc = p.ultra ? 3 : 2;
        hostBackend().generatorMul(false, sc[0], nsc, 0, g1[0], nullptr);
        hostBackend().generatorMul(true, sc[0], nsc, 0, g2[0], nullptr);
        Delta::wipe(sc[1]);
        Delta::wipe(sc[2]);
        memcpy(hp.g1[0], sl.alpha1, 64); memcpy(hp.g1[1], sl.beta1, 64); memcpy(hp.g1[3], g1[1], 64);
        memcpy(hp.g2[0], sl.beta2, 128); memcpy(hp.g2[1], g2[0], 128); memcpy(hp.g2[3], g2[1], 128);
        if (p.ultra) { memcpy(hp.g1[2], g1[2], 64); memcpy(hp.g2[2], g2[2], 128); }
    }
    finishKey(cs, p, lay, perPiece, hp, krec, zkey, vkey, p.ultra);
    clock.lap(5);
    return lay.total;
}

// the size entry and the run entry of either protocol
template <class Options>
int sizeEntry(const Options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, uint64_t* zkeyBytes, uint64_t* vkeyBytesMax,
              char* errorMsg, unsigned long long errorMsgMax) {
    return guarded(SETUP_RULE, errorMsg, errorMsgMax, [&] {
        double ms[PTAU_PHASES] = {0};
        u64 vmax = 0;
        const u64 total = runPtau(requestOf(opt), r1cs, r1csSize, ptau, ptauSize, -1, nullptr, 0, nullptr, ms, true, &vmax);
        if (zkeyBytes) *zkeyBytes = total;
        if (vkeyBytesMax) *vkeyBytesMax = vmax;
    });
}
template <class Options>
int runEntry(const Options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, int device, void* zkey, u64 zkeyCap,
             uint64_t* zkeyBytes, char* vkeyJson, u64 vkeyCap, uint64_t* vkeyBytes, double* phaseMs, char* errorMsg,
             unsigned long long errorMsgMax) {
    return guarded(SETUP_RULE, errorMsg, errorMsgMax, [&] {
        double ms[PTAU_PHASES] = {0};
        std::string vkey;
        const u64 total = runPtau(requestOf(opt), r1cs, r1csSize, ptau, ptauSize, device, (uint8_t*)zkey, zkeyCap, &vkey, ms, false, nullptr);
        if (zkeyBytes) *zkeyBytes = total;
        copyVkey(vkey, vkeyJson, vkeyCap, vkeyBytes);
        if (phaseMs) for (int i = 0; i < PTAU_PHASES; i++) phaseMs[i] = ms[i];
    });
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

extern "C" {

int ug_ptau_parse_info(const void* ptau, uint64_t ptau_size, ug_ptau_info* out, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (!out) throw PtauError("null buffer");
        const std::unique_ptr<ughost::BinFile> f = ughost::openBinFile(ptau, ptau_size, "ptau", "ptau: ", "null buffer");
        const ughost::PtauHeader h = ughost::loadPtauHeader(*f);
        out->power = h.power; out->ceremony_power = h.ceremonyPower; out->prepared = h.prepared ? 1 : 0;
        out->max_log_domain = 0;
        if (h.prepared)                              // the largest n whose slices the sections hold
            for (u32 n = std::min<u32>(h.power, MAX_LOG_DOMAIN); n >= 1; n--) {
                try { ughost::loadPtauSlices(*f, h, n); out->max_log_domain = n; break; } catch (const std::exception&) {}
            }
    });
}

int ug_setup_ptau_size(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                       uint64_t* zkey_bytes, uint64_t* vkey_bytes_max, char* error_msg, unsigned long long error_msg_maxsize) {
    return sizeEntry(opt, r1cs, r1cs_size, ptau, ptau_size, zkey_bytes, vkey_bytes_max, error_msg, error_msg_maxsize);
}

int ug_setup_ptau_run(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                      int device, void* zkey, uint64_t zkey_capacity, uint64_t* zkey_bytes, char* vkey_json, uint64_t vkey_capacity,
                      uint64_t* vkey_bytes, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    return runEntry(opt, r1cs, r1cs_size, ptau, ptau_size, device, zkey, zkey_capacity, zkey_bytes, vkey_json, vkey_capacity, vkey_bytes, phase_ms,
                    error_msg, error_msg_maxsize);
}

int ug_ultra_setup_ptau_size(const ug_ultra_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                             uint64_t ptau_size, uint64_t* zkey_bytes, uint64_t* vkey_bytes_max, char* error_msg,
                             unsigned long long error_msg_maxsize) {
    return sizeEntry(opt, r1cs, r1cs_size, ptau, ptau_size, zkey_bytes, vkey_bytes_max, error_msg, error_msg_maxsize);
}

int ug_ultra_setup_ptau_run(const ug_ultra_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                            uint64_t ptau_size, int device, void* zkey, uint64_t zkey_capacity, uint64_t* zkey_bytes, char* vkey_json,
                            uint64_t vkey_capacity, uint64_t* vkey_bytes, double* phase_ms, char* error_msg,
                            unsigned long long error_msg_maxsize) {
    return runEntry(opt, r1cs, r1cs_size, ptau, ptau_size, device, zkey, zkey_capacity, zkey_bytes, vkey_json, vkey_capacity, vkey_bytes, phase_ms,
                    error_msg, error_msg_maxsize);
}

int ug_points_combine(int device, int g2, const uint32_t* col_ptr, uint64_t n_cols, const uint32_t* index, const void* coefs,
                      const void* points, uint64_t n_points, void* out, double* kernel_ms, char* error_msg,
                      unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
        if (!n_cols) return;
        if (!out || (n_points && !points)) throw SetupError("null buffer");
        if (n_points > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        checkColumns(col_ptr, n_cols, index, (const uint8_t*)coefs, n_points);
        PointSegs pts;
        pts.base[0] = (const uint8_t*)points; pts.count = n_points; pts.n = 1;      // (no points: checkColumns has refused every term)
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).combine(g2 != 0, n_cols, col_ptr, index, (const uint8_t*)coefs, pts, (uint8_t*)out, kernel_ms);
    });
}

int ug_points_scale(int device, const void* scalar, const void* points, uint64_t n, void* out, double* kernel_ms, char* error_msg,
                    unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) kernel_ms[0] = 0;
        if (!scalar || (n && (!points || !out))) throw SetupError("null buffer");
        if (!belowR((const uint8_t*)scalar)) throw SetupError("scalar is not below the field modulus");
        if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        if (!n) return;
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).scale((const uint8_t*)scalar, (const uint8_t*)points, n, (uint8_t*)out, kernel_ms);
    });
}

int ug_points_ratio_mask(int device, const void* x, const void* y, uint64_t n, const void* q, uint64_t max_blocks, void* record_mask,
                         void* block_mask, ug_ratio_report* out, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (out) memset(out, 0, sizeof *out);
        if (!q || !out || (n && (!x || !y || !record_mask || !block_mask))) throw SetupError("null buffer");
        if (n > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        if (allZero((const uint8_t*)q, 128)) throw SetupError("q is the point at infinity");
        std::unique_ptr<Backend> owned;
        RatioOut r;
        backendFor(device, owned).ratio((const uint8_t*)x, (const uint8_t*)y, n, (const uint8_t*)q, max_blocks, r);
        if (n) memcpy(block_mask, r.blockBad.data(), (size_t)r.blocks);
        uint8_t* o = (uint8_t*)record_mask;
        for (size_t b = 0; b < r.resolved.size(); b++) {         // (a short last block gives only the records it has)
            const u64 count = std::min<u64>(RATIO_BLOCK, n - r.resolved[b] * RATIO_BLOCK);
            memcpy(o, &r.recordBad[b * RATIO_BLOCK], (size_t)count);
            o += count;
        }
        out->blocks = r.blocks; out->bad_blocks = r.badBlocks; out->resolved_blocks = r.resolvedBlocks; out->bad_records = r.badRecords;
        out->resolved_records = (uint64_t)(o - (uint8_t*)record_mask);
        out->exact = r.exact ? 1 : 0;
        const std::vector<u64> listed = r.listed(n, UG_RATIO_LISTED);
        out->n_listed = (uint32_t)listed.size();
        for (size_t i = 0; i < listed.size(); i++) out->index[i] = listed[i];
        out->kernel_ms[0] = r.ms[0]; out->kernel_ms[1] = r.ms[1];
    });
}

int ug_points_scale_segments(int device, int n_segments, const ug_scale_segment* segments, const void* points, uint64_t n_points,
                             void* out, double* kernel_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) kernel_ms[0] = 0;
        if (n_segments < 0 || n_segments > MAX_SCALE_SEGS) throw SetupError(std::to_string(n_segments) + " segments: at most " + std::to_string(MAX_SCALE_SEGS));
        if (n_segments && !segments) throw SetupError("null buffer");
        if (n_points > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
        ScaleSeg segs[MAX_SCALE_SEGS];
        u64 total = 0;
        for (int s = 0; s < n_segments; s++) {
            const ug_scale_segment& g = segments[s];
            if (!g.scalar) throw SetupError("null buffer");
            if (!belowR((const uint8_t*)g.scalar)) throw SetupError("segment " + std::to_string(s) + ": scalar is not below the field modulus");
            if (g.count > 0xffffffffull) throw SetupError("sizes that cannot be represented: more than 2^32 - 1 points");
            if (!g.index && g.count > n_points) throw SetupError("segment " + std::to_string(s) + ": " + std::to_string(g.count) + " records of " + std::to_string(n_points));
            if (g.index)
                for (u64 i = 0; i < g.count; i++)
                    if (g.index[i] >= n_points)
                        throw SetupError("segment " + std::to_string(s) + " index " + std::to_string(i) + ": point " + std::to_string(g.index[i]) + " out of range");
            segs[s].scalar = (const uint8_t*)g.scalar; segs[s].src = (const uint8_t*)points; segs[s].nSrc = n_points;
            segs[s].index = g.index; segs[s].count = g.count; segs[s].out = (uint8_t*)out + total * 64;
            total += g.count;
        }
        if (!total) return;
        if (!out || !points) throw SetupError("null buffer");
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).scaleSegments(segs, n_segments, kernel_ms);
    });
}

}  // extern "C"
