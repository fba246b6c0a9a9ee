// zkey_verify_host.cpp -- is this Groth16 key the one its circuit and a prepared powers-of-tau file give under ONE delta?
// (include/ultragroth_hip.h: ug_zkey_verify_run, ug_r1cs_fold). No trapdoor and no delta is known here. Out of scope: who
// contributed -- section 10's transcript, beacons, the .ptau's own ceremony. An UltraGroth key (ug_ultra_zkey_verify_run,
// ug_r1cs_fold_classes) goes through the same run(): three weight classes and two deltas, each C section under its own
// (DESIGN.md section 5.12). What differs between the protocols is a description filled in once the header is read (Protocol).
//
// Making the key again costs a point combination per wire. The check draws a 128-bit weight rho_s per wire and moves the weights
// to the SCALAR side: sum_s rho_s A_s = sum_k (A rho)_k T[k], so one sparse matrix-vector product over Fr (the fold) and a few
// MSMs over the level-n slices stand against one MSM over each section of the key; H needs no matrix at all. The relations and
// their soundness are in DESIGN.md section 5.11; the notation is ug_setup_ptau_run's.
//
// ug_zkey_locate_run / ug_ultra_zkey_locate_run go through the same run() and, once the verdict is known, name the wrong records
// of every failing point section (locateSections): sections 5, 6, 7 against the combination of the circuit's
// columns by bytes, section 3, the C sections and H against their delta-free counterparts through Backend::ratio.
//
// This file is the host layer and the host twin (device = -1): the files' rules, the point check, relation 0 (header) and
// relation 1 (section 4, through setup_host.cpp's own writer), the weights, the pairings (pairing.hpp, host threads wherever the
// sums were made) and the verdict. The sums (twelve, fourteen for an UltraGroth key) come from host threads here or from the
// device (zkey_verify.hip), as canonical affine records, so the two agree byte for byte.
#include "zkey_verify.hpp"
#include "pairing.hpp"
#include "setup_host.hpp"

#include <sys/random.h>

#include <algorithm>
#include <cerrno>
#include <future>
#include <memory>

namespace ughost {
namespace zkv {

using namespace ug;
using namespace ug::pr;
using namespace ughost::setup;

DeviceSums deviceSums = nullptr;
DeviceFold deviceFold = nullptr;

namespace {

constexpr int PHASES = UG_ZKEY_VERIFY_PHASES;

struct ZkeyError : public std::invalid_argument {
    explicit ZkeyError(const std::string& m) : std::invalid_argument("zkey: " + m) {}
};
struct R1csRefusal : public std::invalid_argument {
    explicit R1csRefusal(const std::string& m) : std::invalid_argument("r1cs: " + m) {}
};

// a loader's text under the prefix of the file it read: a shared helper's "setup: " goes, the three files' own prefixes stay
constexpr PrefixRule R1CS_RULE = {"r1cs: ", {"r1cs: ", "ptau: ", "zkey: "}, true};
constexpr PrefixRule ZKEY_RULE = {"zkey: ", {"r1cs: ", "ptau: ", "zkey: "}, true};
// body() with its refusals under the rule
template <class Body> void under(const PrefixRule& rule, Body&& body) {
    try {
        body();
    } catch (const std::exception& e) {
        throw std::invalid_argument(underPrefix(rule, e.what()));
    }
}

// ---- the weights: fresh from the OS for every call, never derived from the inputs (as verifier_api.cpp's batch scalars) ----
void drawWeights(std::vector<uint8_t>& out, u64 n) {
    out.assign((size_t)n * 32, 0);
    parallelFor(n, 1 << 16, [&](u64 lo, u64 hi) {
        std::vector<uint8_t> raw((size_t)(hi - lo) * 16);
        size_t got = 0;
        while (got < raw.size()) {
            const ssize_t w = getrandom(raw.data() + got, raw.size() - got, 0);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) throw std::runtime_error("zkey: getrandom failed");
            got += (size_t)w;
        }
        for (u64 i = lo; i < hi; i++) memcpy(&out[(size_t)i * 32], &raw[(size_t)(i - lo) * 16], 16);
    });
}

// ---- the fold on host threads: the witness check's row walk with rho in the witness's place and one sum per class and matrix ----
// K classes of wires: cls null is a Groth16 key's two (wire s is public, class 0, when s <= nPublic), cls a byte per wire an
// UltraGroth key's three (0 public, 1 round, anything else final). out: 3 K + 2 vectors of N plain canonical integers: vector
// 3 m + t is matrix t (A, B, C) over class m, 3 K is a and 3 K + 1 is b (over all wires)
int foldVectors(int K) { return 3 * K + 2; }
void hostFold(const R1cs& cs, const uint8_t* rho, const uint8_t* cls, u32 nPublic, u64 N, uint8_t* out) {
    const int K = cls ? 3 : 2;
    const u64 M = cs.hdr.nWires, rows = cs.hdr.nConstraints;
    std::vector<Fr> w((size_t)M);
    parallelFor(M, 4096, [&](u64 lo, u64 hi) {
        for (u64 s = lo; s < hi; s++) w[(size_t)s] = frFromPlain(rho + s * 32);
    });
    memset(out, 0, (size_t)N * 32 * foldVectors(K));
    auto at = [&](int v, u64 k) { return out + ((size_t)v * N + k) * 32; };
    parallelFor(N, 1024, [&](u64 lo, u64 hi) {
        for (u64 k = lo; k < hi; k++) {
            if (k >= rows) {                         // a public row carries A = {s: 1}: rho_s in a^pub and in a
                if (k - rows <= nPublic) { frToPlain(at(0, k), w[(size_t)(k - rows)]); memcpy(at(3 * K, k), at(0, k), 32); }
                continue;
            }
            for (int t = 0; t < 3; t++) {
                const R1csMatrix& m = cs.m[t];
                Fr acc[MAX_CLASSES] = {fp_zero<FrParams>(), fp_zero<FrParams>(), fp_zero<FrParams>()};
                for (u32 q = m.rowPtr[k]; q < m.rowPtr[k + 1]; q++) {
                    const u32 s = m.sig[q];
                    const int side = cls ? std::min<int>(cls[s], 2) : s > nPublic ? 1 : 0;
                    acc[side] = frAdd(acc[side], frMul(frFromPlain(&m.val[(size_t)q * 32]), w[s]));
                }
                Fr all = acc[0];
                for (int c = 0; c < K; c++) {
                    frToPlain(at(3 * c + t, k), acc[c]);
                    if (c) all = frAdd(all, acc[c]);
                }
                if (t < 2) frToPlain(at(3 * K + t, k), all);
            }
        }
    });
}

// ---- an MSM on host threads: hostCombine with few columns, then one column of unit terms over their sums ----
void sumRecords(bool g2, const uint8_t* recs, u64 n, uint8_t* out) {
    std::vector<u32> colPtr = {0, (u32)n}, index((size_t)n);
    std::vector<uint8_t> ones((size_t)n * 32, 0);
    for (u64 i = 0; i < n; i++) { index[(size_t)i] = (u32)i; ones[(size_t)i * 32] = 1; }
    PointSegs p;
    p.base[0] = recs; p.count = n; p.n = 1;
    hostBackend().combine(g2, 1, colPtr.data(), index.data(), ones.data(), p, out, nullptr);
}
void hostMsm(bool g2, const uint8_t* scalars, const PointSegs& pts, uint8_t* out) {
    const u64 n = pts.total(), rec = g2 ? 128 : 64;
    if (!n) { memset(out, 0, rec); return; }
    const u64 cols = std::min<u64>(n, 1024);
    std::vector<u32> colPtr((size_t)cols + 1), index((size_t)n);
    for (u64 c = 0; c <= cols; c++) colPtr[(size_t)c] = (u32)(n * c / cols);
    for (u64 i = 0; i < n; i++) index[(size_t)i] = (u32)i;
    std::vector<uint8_t> part((size_t)(cols * rec));
    hostBackend().combine(g2, cols, colPtr.data(), index.data(), scalars, pts, part.data(), nullptr);
    sumRecords(g2, part.data(), cols, out);
}
void hostMsm(bool g2, const uint8_t* scalars, const uint8_t* points, u64 n, uint8_t* out) {
    PointSegs p;
    p.base[0] = points; p.count = n; p.n = 1;
    hostMsm(g2, scalars, p, out);
}

void hostSums(const Inputs& in, const uint8_t* hOdd, Sums& out, SumsStats& st) {
    PhaseClock clock(st.ms);
    const double t0 = nowMs();
    const u64 N = in.N, M = in.M, pub = in.pub;
    const int K = in.K;
    std::vector<uint8_t> f((size_t)N * 32 * foldVectors(K));
    hostFold(*in.cs, in.rho, in.cls, (u32)(pub - 1), N, f.data());
    st.foldKernelMs = nowMs() - t0;
    clock.lap(0);
    auto vec = [&](int v) { return f.data() + (size_t)v * N * 32; };
    hostMsm(false, vec(3 * K), in.T, N, out.aT);
    hostMsm(false, vec(3 * K + 1), in.T, N, out.bT);
    hostMsm(true, vec(3 * K + 1), in.T2, N, out.bT2);
    PointSegs three;                             // [a^m | b^m | c^m] over [bT | aT | T]
    three.count = N; three.n = 3;
    three.base[0] = in.bT; three.base[1] = in.aT; three.base[2] = in.T;
    for (int m = 0; m < K; m++) hostMsm(false, vec(3 * m), three, out.k[m]);
    clock.lap(1);
    hostMsm(false, in.rho, in.a, M, out.keyA);
    hostMsm(false, in.rho, in.b1, M, out.keyB1);
    hostMsm(true, in.rho, in.b2, M, out.keyB2);
    hostMsm(false, in.rho, in.ic, pub, out.keyIC);
    for (int i = 0; i < K - 1; i++) hostMsm(false, in.c[i].weights, in.c[i].points, in.c[i].n, out.keyC[i]);
    clock.lap(2);
    hostMsm(false, in.sigma, in.h, N, out.keyH);
    hostMsm(false, in.sigma, hOdd, N, out.hP);
    clock.lap(3);
}

// ---- pairings (pairing.hpp, host threads) ----
const FinalExpConsts& consts() { static const FinalExpConsts c = final_exp_consts(); return c; }
G1A g1Of(const uint8_t* rec) {                  // (pairing.hpp's record forms; a file's records sit at any alignment)
    u32 w[16];
    memcpy(w, rec, 64);
    return g1_from_record(w, false);
}
G2A g2Of(const uint8_t* rec) {
    u32 w[32];
    memcpy(w, rec, 128);
    return g2_from_record(w);
}
G1A g1Generator() { return G1A{f1_small(1), f1_small(2), false}; }
G2A g2Generator() {
    u32 w[32];
    generatorWords(true, w);
    auto c = [&](int i) { return F1{cond_sub_q(unpack256<FqParams>(w + 8 * i))}; };
    return G2A{F2{c(0), c(1)}, F2{c(2), c(3)}, false};
}
// e(p1, q1) == e(p2, q2); a pair with a point at infinity counts as one (every point is in its group of order r)
bool samePairing(const G1A& p1, const G2A& q1, const G1A& p2, const G2A& q2) {
    F12 acc = f12_one(), hard;
    if (pair_live(p1, q1)) acc = f12_mul(consts(), acc, miller(consts(), q1, p1));
    if (pair_live(p2, q2)) acc = f12_mul(consts(), acc, miller(consts(), q2, G1A{p2.x, -p2.y, false}));
    return final_exp_is_one(consts(), acc, hard);
}

// ---- the two protocols as data: filled in once the header is read, read by everything after it ----
struct HeaderPoint { const char* name; const uint8_t* p; bool g2; };
struct Protocol {
    int K = 2;                                   // weight classes: K - 1 deltas and K - 1 C sections, C section i (id 8 + i) under delta i
    std::vector<HeaderPoint> header;             // section 2's points in the point check's order, under the point check's names
    const uint8_t *delta1[MAX_C_SECTIONS] = {}, *delta2[MAX_C_SECTIONS] = {};      // the last is H's (the final delta)
    u64 cCount[MAX_C_SECTIONS] = {0, 0};         // records of each C section
    const char* cTail[MAX_C_SECTIONS] = {"", ""};
    u32 hId = 9;
    const char* hTail = "";
};
Protocol protocolOf(const ZkeyHeader& zh, bool ultra, u64 M, u64 pub) {
    Protocol p;
    p.header = {{"alpha1", zh.alpha1, false}, {"beta1", zh.beta1, false}, {"beta2", zh.beta2, true}, {"gamma2", zh.gamma2, true}};
    if (!ultra) {                                // public | private; one delta
        p.header.insert(p.header.end(), {{"delta1", zh.delta1, false}, {"delta2", zh.delta2, true}});
        p.delta1[0] = zh.delta1; p.delta2[0] = zh.delta2;
        p.cCount[0] = M - pub; p.cTail[0] = " under the key's delta";
        p.hTail = " under the key's delta";
        return p;
    }
    p.K = 3;                                     // public | the key's round list | its final list; a delta for each list
    p.header.insert(p.header.end(), {{"delta_c1_1", zh.roundDelta1, false}, {"delta_c1_2", zh.roundDelta2, true},
                                     {"delta_c2_1", zh.delta1, false}, {"delta_c2_2", zh.delta2, true}});
    p.delta1[0] = zh.roundDelta1; p.delta2[0] = zh.roundDelta2;
    p.delta1[1] = zh.delta1; p.delta2[1] = zh.delta2;
    p.cCount[0] = zh.numIndexesC1; p.cTail[0] = " under the key's round delta";
    p.cCount[1] = zh.numIndexesC2; p.cTail[1] = " under the key's final delta";
    p.hId = 12; p.hTail = " under the key's final delta";
    return p;
}

// ---- the point check of the key, with ug_zkey_check's messages ----
void checkKeyPoints(const PointCheck& check, const Protocol& pr, const Inputs& in) {
    for (const HeaderPoint& hp : pr.header) {
        uint8_t rec[128];                        // (the header's points sit at any alignment)
        memcpy(rec, hp.p, hp.g2 ? 128 : 64);
        const ug_point_fault f = check.find(hp.g2, rec, 1);
        if (f.reason) throw ZkeyError(std::string("header point ") + hp.name + ": " + PointCheck::reasonText(f.reason));
    }
    struct Sec { u32 id; bool g2; const uint8_t* p; u64 n; };
    std::vector<Sec> secs = {{3, false, in.ic, in.pub}, {5, false, in.a, in.M}, {6, false, in.b1, in.M}, {7, true, in.b2, in.M}};
    for (int i = 0; i < pr.K - 1; i++) secs.push_back({8 + (u32)i, false, in.c[i].points, in.c[i].n});
    secs.push_back({pr.hId, false, in.h, in.N});
    for (const Sec& s : secs) {
        const ug_point_fault f = check.find(s.g2, s.p, s.n);
        if (f.reason)
            throw ZkeyError("section " + std::to_string(s.id) + " point " + std::to_string(f.index) + ": " + PointCheck::reasonText(f.reason));
    }
}

struct Verdict {
    u32 failed = 0;
    int first = 0;
    std::string message;
    void fail(int section, const std::string& m) {
        if (!failed) { first = section; message = m; }
        failed |= 1u << section;
    }
};

const uint8_t* sectionOf(const BinFile& f, u32 id, u64 need) {
    if (f.sectionSize(id) < need) throw ZkeyError("Section " + std::to_string(id) + " is shorter than the header implies");
    return f.sectionData(id);
}

// ---- naming the wrong records of the sections that failed ----
struct Locate {
    u32 maxListed, maxBlocks;                    // (the defaults are in place)
    ug_zkey_locate_report* out;
};
ug_zkey_locate_section* newEntry(const Locate& lc, u32 id, u32 method, u64 records) {
    if (lc.out->n_sections >= UG_ZKEY_LOCATE_SECTIONS) throw ZkeyError("internal: more failing point sections than a report holds");
    ug_zkey_locate_section* e = &lc.out->section[lc.out->n_sections++];
    e->section = id; e->method = method; e->records = records;
    e->blocks = (records + RATIO_BLOCK - 1) / RATIO_BLOCK;
    return e;
}
// Every section in `failed` that holds points, in the order 3, 5, 6, 7, the C sections, H; one section's expected records at a
// time. list[i]: the signals of an UltraGroth key's C section i (a Groth16 key's C section is the wires from pub on).
void locateSections(const Locate& lc, u32 failed, const Protocol& pr, const Inputs& in, const uint8_t* gamma2, const R1cs& cs, const Plan& plan,
                    const uint8_t* hOdd, const std::vector<u32>* list, bool ultra, int device) {
    const int nC = pr.K - 1;
    u32 pointSections = (1u << 3) | (1u << 5) | (1u << 6) | (1u << 7) | (1u << pr.hId);
    for (int i = 0; i < nC; i++) pointSections |= 1u << (8 + i);
    if (!(failed & pointSections)) return;
    const double t0 = nowMs();
    const u64 M = in.M, N = in.N;
    std::unique_ptr<Backend> owned;
    Backend& be = backendFor(device, owned);
    ColMatrix cm[3];
    bool haveColumns = false;
    auto columns = [&] {
        if (haveColumns) return;
        std::vector<Piece> pieces;
        buildColumns(cs, plan, cm, pieces);
        haveColumns = true;
    };
    // A, B1, B2 do not depend on a delta: the expected records themselves, compared by bytes
    auto byBytes = [&](u32 id, bool g2, int m, const uint8_t* slice, const uint8_t* have) {
        if (!(failed >> id & 1) || !M) return;
        columns();
        const u64 rec = g2 ? 128 : 64;
        std::vector<uint8_t> want((size_t)(M * rec));
        PointSegs one;
        one.count = N; one.n = 1; one.base[0] = slice;
        be.combine(g2, M, cm[m].colPtr.data(), cm[m].row.data(), cm[m].val.data(), one, want.data(), nullptr);
        ug_zkey_locate_section* e = newEntry(lc, id, UG_LOCATE_BYTES, M);
        e->exact = 1;
        u64 lastBlock = ~0ull;
        for (u64 i = 0; i < M; i++) {
            if (!memcmp(&want[(size_t)(i * rec)], have + i * rec, (size_t)rec)) continue;
            e->bad_records++;
            if (i / RATIO_BLOCK != lastBlock) { lastBlock = i / RATIO_BLOCK; e->bad_blocks++; }
            if (e->n_listed < lc.maxListed) e->index[e->n_listed++] = i;
        }
        e->resolved_blocks = e->bad_blocks;
    };
    // X_s d = Y_s for a d nobody knows: the ratio test against d's G2 point
    auto byRatio = [&](u32 id, const uint8_t* have, const uint8_t* expect, u64 n, const uint8_t* q) {
        uint8_t qrec[128];                       // (the header's points sit at any alignment)
        memcpy(qrec, q, 128);
        if (allZero(qrec, 128)) return;
        RatioOut r;
        be.ratio(have, expect, n, qrec, lc.maxBlocks, r);
        ug_zkey_locate_section* e = newEntry(lc, id, UG_LOCATE_RATIO, n);
        e->bad_blocks = r.badBlocks; e->resolved_blocks = r.resolvedBlocks; e->bad_records = r.badRecords;
        e->exact = r.exact ? 1 : 0;
        const std::vector<u64> listed = r.listed(n, lc.maxListed);
        e->n_listed = (u32)listed.size();
        for (size_t i = 0; i < listed.size(); i++) e->index[i] = listed[i];
        e->kernel_ms[0] = r.ms[0]; e->kernel_ms[1] = r.ms[1];
    };
    // K_s of n wires (a list, or a run from `first`): setup_ptau.cpp's combination over [T | aT | bT], before any delta
    auto byRatioK = [&](u32 id, const uint8_t* have, const u32* wires, u64 first, u64 n, const uint8_t* q) {
        if (!(failed >> id & 1) || !n) return;
        columns();
        std::vector<u32> colPtr, index;
        std::vector<uint8_t> coefs, k((size_t)n * 64);
        mergedColumns(cm, wires, first, n, N, colPtr, index, coefs);
        PointSegs three;
        three.count = N; three.n = 3;
        three.base[0] = in.T; three.base[1] = in.aT; three.base[2] = in.bT;
        be.combine(false, n, colPtr.data(), index.data(), coefs.data(), three, k.data(), nullptr);
        byRatio(id, have, k.data(), n, q);
    };
    byRatioK(3, in.ic, nullptr, 0, in.pub, gamma2);
    byBytes(5, false, 0, in.T, in.a);
    byBytes(6, false, 1, in.T, in.b1);
    byBytes(7, true, 1, in.T2, in.b2);
    for (int i = 0; i < nC; i++)
        byRatioK(8 + (u32)i, in.c[i].points, ultra ? list[i].data() : nullptr, in.pub, in.c[i].n, pr.delta2[i]);
    if (failed >> pr.hId & 1) byRatio(pr.hId, in.h, hOdd, N, pr.delta2[nC - 1]);
    lc.out->locate_ms = nowMs() - t0;
}

// what a run reads of either options struct; ultra: null for a Groth16 key; locate: null for a verify entry
struct Request {
    u32 validate;
    const ug_ultra_zkey_verify_options* ultra;
    const Locate* locate = nullptr;
};
Request checkOptions(const ug_zkey_verify_options* o) {
    checkOptionsHead<ZkeyError>(o, 1, 2, "1 or 2");
    return {o->validate, nullptr};
}
Request checkOptions(const ug_ultra_zkey_verify_options* o) {
    checkOptionsHead<ZkeyError>(o, 1, 2, "1 or 2");
    if (o->check_spec > 1) throw ZkeyError("check_spec " + std::to_string(o->check_spec) + " is not 0 or 1");
    if (o->check_spec && ((o->n_round && !o->round_signals) || (o->n_final && !o->final_signals))) throw ZkeyError("null signal list");
    return {o->validate, o};
}

// 0: valid, UG_ZKEY_INVALID: *v says which sections fail (bits 2 - 9, 2 - 12 for an UltraGroth key); a refusal is an exception
int run(const Request& rq, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, const void* zkey, u64 zkeySize, int device,
        ug_zkey_verify_report* rep, double ms[PHASES], Verdict& v) {
    PhaseClock clock(ms);
    const bool ultra = rq.ultra != nullptr;
    if (device >= 0 && !deviceSums) throw ZkeyError("this program has no device path: use device = -1 (host threads)");
    // ---- every size and header rule of the three files, before the first device byte ----
    std::unique_ptr<BinFile> rf;
    R1cs cs;
    under(R1CS_RULE, [&] { loadCircuit(r1cs, r1csSize, rf, cs.hdr); });
    const u64 M = cs.hdr.nWires, nPublic = (u64)cs.hdr.nPubOut + cs.hdr.nPubIn, pub = nPublic + 1;
    if (pub > M) throw R1csRefusal("nPubOut + nPubIn + 1 exceeds nWires");
    const u64 rows = (u64)cs.hdr.nConstraints + pub;

    const std::unique_ptr<BinFile> zf = openBinFile(zkey, zkeySize, "zkey", "zkey: ", "null zkey buffer");
    ZkeyHeader zh;
    under(ZKEY_RULE, [&] {
        if (!ultra) {                            // (the UltraGroth loader has its own "zkey file is not ultragroth" for a Groth16 key)
            if (zf->sectionSize(1) < 4) throw ZkeyError("section 1 is too short");
            u32 protocol = 0;
            memcpy(&protocol, zf->sectionData(1), 4);
            if (protocol == 1337) throw ZkeyError("protocol 1337 keys are not checked");
        }
        zh = loadZkeyHeader(*zf, ultra);
    });
    if (!zh.rIsBn254) throw ZkeyError("zkey curve not supported");
    if (memcmp(zf->sectionData(2) + 4, BN254_Q_LE, 32) != 0) throw ZkeyError("header: q is not the BN254 base modulus");
    if (zh.nVars != M) throw ZkeyError("header: nVars " + std::to_string(zh.nVars) + ", the circuit has " + std::to_string(M) + " wires");
    if (zh.nPublic != nPublic) throw ZkeyError("header: nPublic " + std::to_string(zh.nPublic) + ", the circuit has " + std::to_string(nPublic));
    const u64 N = zh.domainSize;
    int logN = 0;
    while (logN < MAX_LOG_DOMAIN && (1ull << logN) < N) logN++;
    if (N < 2 || (1ull << logN) != N)
        throw ZkeyError("header: domain " + std::to_string(N) + " is not a power of two from 2 to 2^" + std::to_string(MAX_LOG_DOMAIN));
    if (N < rows) throw ZkeyError("header: domain " + std::to_string(N) + " is too small for the circuit's " + std::to_string(rows) + " rows");
    const Protocol pr = protocolOf(zh, ultra, M, pub);
    const int nC = pr.K - 1;
    Inputs in;
    in.K = pr.K;
    in.M = M; in.N = N; in.pub = pub; in.logN = logN;
    in.r1cs = r1cs; in.r1csSize = r1csSize; in.cs = &cs;
    const uint8_t* coefs = nullptr;
    const uint8_t* lists[MAX_C_SECTIONS] = {nullptr, nullptr};       // an UltraGroth key's own lists: sections 10, 11
    u64 keyCoefs = 0;
    under(ZKEY_RULE, [&] {
        in.ic = sectionOf(*zf, 3, pub * 64);
        coefs = sectionOf(*zf, 4, 4);
        u32 n32 = 0;
        memcpy(&n32, coefs, 4);
        keyCoefs = n32;
        coefs = sectionOf(*zf, 4, 4 + keyCoefs * 44) + 4;
        in.a = sectionOf(*zf, 5, M * 64);
        in.b1 = sectionOf(*zf, 6, M * 64);
        in.b2 = sectionOf(*zf, 7, M * 128);
        for (int i = 0; i < nC; i++) { in.c[i].n = pr.cCount[i]; in.c[i].points = sectionOf(*zf, 8 + i, pr.cCount[i] * 64); }
        if (ultra)
            for (int i = 0; i < nC; i++) lists[i] = sectionOf(*zf, 10 + i, pr.cCount[i] * 4);
        in.h = sectionOf(*zf, pr.hId, N * 64);
    });
    Plan plan;
    std::vector<u32> list[MAX_C_SECTIONS];
    under(ZKEY_RULE, [&] {
        planSizes(cs.hdr, (u32)logN, plan);
        if (!ultra) return;
        // the key's own rounds: rand_indx public, the lists a partition of the private signals (planLists' rules and texts)
        for (int i = 0; i < nC; i++) {
            list[i].resize((size_t)pr.cCount[i]);
            if (pr.cCount[i]) memcpy(list[i].data(), lists[i], (size_t)pr.cCount[i] * 4);
        }
        planLists(plan, zh.randIndx, list[0].data(), pr.cCount[0], list[1].data(), pr.cCount[1]);
        in.cls = plan.cls.data();
    });

    const std::unique_ptr<BinFile> pf = openBinFile(ptau, ptauSize, "ptau", "ptau: ", "null ptau buffer");
    const PtauHeader ph = loadPtauHeader(*pf);
    const PtauSlices sl = loadPtauSlices(*pf, ph, (u32)logN);
    in.T = sl.tau1; in.T2 = sl.tau2; in.aT = sl.alphaTau1; in.bT = sl.betaTau1; in.top = sl.top;
    under(R1CS_RULE, [&] { loadR1cs(*rf, cs); });
    std::vector<uint8_t> hOdd((size_t)N * 64);  // H's sources side by side (the host twin's bases, and what the point check reads)
    gatherOddTop(sl, hOdd.data());
    clock.lap(0);

    // ---- every point of the key and of the slices, before any relation: a bad point is a refusal, not a verdict ----
    {
        const PointCheck check(device, (int)rq.validate);
        checkSlices(check, sl, hOdd.data());
        checkKeyPoints(check, pr, in);
    }
    rep->subgroup_checked = rq.validate >= 2 ? 1 : 0;
    clock.lap(1);

    std::vector<uint8_t> rho, sigma, rhoList[MAX_C_SECTIONS];
    drawWeights(rho, M);
    drawWeights(sigma, N);
    in.rho = rho.data(); in.sigma = sigma.data();
    if (!ultra) {                                // the private wires are rho's own run from wire pub on
        in.c[0].weights = rho.data() + pub * 32; in.c[0].rhoFirst = (int64_t)pub;
    } else {                                     // the weights of a list's signals, in the list's order (a host step: 32 bytes per private signal)
        for (int i = 0; i < nC; i++) {
            rhoList[i].resize((size_t)pr.cCount[i] * 32);
            for (u64 j = 0; j < pr.cCount[i]; j++) memcpy(&rhoList[i][(size_t)j * 32], &rho[(size_t)list[i][(size_t)j] * 32], 32);
            in.c[i].weights = rhoList[i].data();
        }
    }
    clock.lap(2);

    // ---- relation 0: the header ----
    const G1A g1 = g1Generator();
    const G2A g2 = g2Generator();
    const G2A gamma2 = g2Of(zh.gamma2);
    G1A d1[MAX_C_SECTIONS];
    G2A d2[MAX_C_SECTIONS];
    for (int i = 0; i < nC; i++) { d1[i] = g1Of(pr.delta1[i]); d2[i] = g2Of(pr.delta2[i]); }
    {
        bool same[MAX_C_SECTIONS] = {true, true};    // delta i's G1 and G2 points are one delta: the last on this thread, beside the others
        std::future<bool> other[MAX_C_SECTIONS];
        for (int i = 0; i < nC - 1; i++) other[i] = std::async(std::launch::async, [&, i] { return samePairing(d1[i], g2, g1, d2[i]); });
        same[nC - 1] = samePairing(d1[nC - 1], g2, g1, d2[nC - 1]);
        for (int i = 0; i < nC - 1; i++) same[i] = other[i].get();
        // the rules in each protocol's own order: the first that holds is the message
        std::vector<std::pair<bool, const char*>> rules = {{memcmp(zh.alpha1, sl.alpha1, 64) != 0, "alpha1 is not the powers of tau's"},
                                                           {memcmp(zh.beta1, sl.beta1, 64) != 0, "beta1 is not the powers of tau's"},
                                                           {memcmp(zh.beta2, sl.beta2, 128) != 0, "beta2 is not the powers of tau's"}};
        if (!ultra)
            rules.insert(rules.end(), {{d1[0].inf, "delta1 is the point at infinity"},
                                       {d2[0].inf, "delta2 is the point at infinity"},
                                       {gamma2.inf, "gamma2 is the point at infinity"},
                                       {!same[0], "delta1 and delta2 are not the same delta"}});
        else
            rules.insert(rules.end(), {{gamma2.inf, "gamma2 is the point at infinity"},
                                       {d1[0].inf || d2[0].inf, "delta_c1 is the point at infinity"},
                                       {d1[1].inf || d2[1].inf, "delta_c2 is the point at infinity"},
                                       {!same[0], "delta_c1's G1 and G2 points are not the same delta"},
                                       {!same[1], "delta_c2's G1 and G2 points are not the same delta"}});
        for (const auto& r : rules)
            if (r.first) { v.fail(2, std::string("zkey: header: ") + r.second); break; }
    }
    // ---- relation 1: section 4 is the one setup_host.cpp writes for this circuit ----
    {
        std::vector<u64> perPiece;
        const u64 nCoefs = pub + countCoefs(cs, perPiece);
        std::vector<uint8_t> want((size_t)nCoefs * 44);
        writeCoefs(cs, plan, perPiece, want.data());
        const u64 common = std::min(nCoefs, keyCoefs);
        u64 bad = common;
        for (u64 i = 0; i < common; i++)
            if (memcmp(&want[(size_t)i * 44], coefs + i * 44, 44) != 0) { bad = i; break; }
        if (bad < common || nCoefs != keyCoefs || zf->sectionSize(4) != 4 + keyCoefs * 44)
            v.fail(4, "zkey: section 4 record " + std::to_string(bad) + ": does not match the circuit");
    }
    // ---- an UltraGroth key's rounds against a spec, where one is given ----
    if (ultra && rq.ultra->check_spec) {
        const ug_ultra_zkey_verify_options* o = rq.ultra;
        const u32* want[MAX_C_SECTIONS] = {o->round_signals, o->final_signals};
        const u64 wantCount[MAX_C_SECTIONS] = {o->n_round, o->n_final};
        if (zh.randIndx != o->rand_indx) v.fail(2, "zkey: header: rand_indx does not match the spec");
        for (int i = 0; i < nC; i++)
            if (pr.cCount[i] != wantCount[i] || (pr.cCount[i] && memcmp(list[i].data(), want[i], (size_t)pr.cCount[i] * 4) != 0))
                v.fail(10 + i, "zkey: section " + std::to_string(10 + i) + ": does not match the spec");
    }
    clock.lap(0);

    // ---- the sums of the remaining relations ----
    Sums s;
    memset(&s, 0, sizeof s);
    SumsStats st;
    if (device < 0) hostSums(in, hOdd.data(), s, st);
    else deviceSums(device, in, s, st);
    for (int i = 0; i < 4; i++) ms[3 + i] += st.ms[i];
    rep->fold_kernel_ms = st.foldKernelMs;
    rep->peak_device_bytes = st.peakDeviceBytes;
    clock.restart();

    const char* const TEXT = ": does not match the circuit and the powers of tau";
    auto secFail = [&](u32 id, const char* tail) { v.fail((int)id, "zkey: section " + std::to_string(id) + TEXT + tail); };
    // e(key's sum, its divisor) == e(the slices' sum, g2): section 3 under gamma, C section i under delta i, H under the last delta
    const G1A keyIC = g1Of(s.keyIC), kPub = g1Of(s.k[0]), keyH = g1Of(s.keyH), hP = g1Of(s.hP);
    auto rel3 = std::async(std::launch::async, [&] { return samePairing(keyIC, gamma2, kPub, g2); });
    std::future<bool> relC[MAX_C_SECTIONS];
    for (int i = 0; i < nC; i++)                 // (an empty section: both sums are infinity and the relation holds)
        relC[i] = std::async(std::launch::async, [&, i] { return samePairing(g1Of(s.keyC[i]), d2[i], g1Of(s.k[1 + i]), g2); });
    auto relH = std::async(std::launch::async, [&] { return samePairing(keyH, d2[nC - 1], hP, g2); });
    if (memcmp(s.keyA, s.aT, 64) != 0) secFail(5, "");
    if (memcmp(s.keyB1, s.bT, 64) != 0) secFail(6, "");
    if (memcmp(s.keyB2, s.bT2, 128) != 0) secFail(7, "");
    bool okC[MAX_C_SECTIONS] = {true, true};
    const bool ok3 = rel3.get();
    for (int i = 0; i < nC; i++) okC[i] = relC[i].get();
    const bool okH = relH.get();
    if (!ok3) secFail(3, "");
    for (int i = 0; i < nC; i++)
        if (!okC[i]) secFail(8 + (u32)i, pr.cTail[i]);
    if (!okH) secFail(pr.hId, pr.hTail);
    clock.lap(7);
    rep->failed_sections = v.failed;
    rep->first_failed = v.first;
    // ---- the verdict stands; a locate entry now names the wrong records of the point sections that failed ----
    if (rq.locate && v.failed) locateSections(*rq.locate, v.failed, pr, in, zh.gamma2, cs, plan, hOdd.data(), list, ultra, device);
    return v.failed ? UG_ZKEY_INVALID : UG_OK;
}

// the report and phase copy-out of a verify entry
template <class Options>
int verifyEntry(const Options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, const void* zkey, u64 zkeySize, int device,
                ug_zkey_verify_report* out, double* phaseMs, char* errorMsg, unsigned long long errorMsgMax) {
    ug_zkey_verify_report rep;
    memset(&rep, 0, sizeof rep);
    double ms[PHASES] = {0};
    int rc = UG_ERROR;
    if (guarded(ZKEY_RULE, errorMsg, errorMsgMax, [&] {
            Verdict v;
            rc = run(checkOptions(opt), r1cs, r1csSize, ptau, ptauSize, zkey, zkeySize, device, &rep, ms, v);
            copyErr(errorMsg, errorMsgMax, v.message.c_str());
        }) != UG_OK) {
        memset(&rep, 0, sizeof rep);              // (a refusal reports nothing)
        rc = UG_ERROR;
    }
    if (out) *out = rep;
    if (phaseMs) for (int i = 0; i < PHASES; i++) phaseMs[i] = ms[i];
    return rc;
}

// A locate entry: the verify entry's call with the options' common fields, then the located report. vopt: the verify options the
// locate options stand for (their size is the verify struct's own, so checkOptions' rules and texts are the verify entry's).
template <class LocateOptions, class VerifyOptions>
int locateEntry(const LocateOptions* opt, VerifyOptions vopt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, const void* zkey,
                u64 zkeySize, int device, ug_zkey_verify_report* out, ug_zkey_locate_report* located, double* phaseMs, char* errorMsg,
                unsigned long long errorMsgMax) {
    ug_zkey_verify_report rep;
    memset(&rep, 0, sizeof rep);
    double ms[PHASES] = {0};
    int rc = UG_ERROR;
    if (located) memset(located, 0, sizeof *located);
    if (guarded(ZKEY_RULE, errorMsg, errorMsgMax, [&] {
            if (!opt) throw ZkeyError("null options");
            if (opt->size != sizeof(LocateOptions)) throw ZkeyError("options struct of another size (" + std::to_string(opt->size) + ")");
            if (!located) throw ZkeyError("null locate report");
            if (opt->max_listed > UG_ZKEY_LOCATE_LISTED)
                throw ZkeyError("max_listed " + std::to_string(opt->max_listed) + " exceeds " + std::to_string(UG_ZKEY_LOCATE_LISTED));
            const Locate lc = {opt->max_listed ? opt->max_listed : 16, opt->max_blocks ? opt->max_blocks : (u32)RATIO_MAX_BLOCKS, located};
            vopt.size = sizeof vopt;
            Request rq = checkOptions(&vopt);
            rq.locate = &lc;
            Verdict v;
            rc = run(rq, r1cs, r1csSize, ptau, ptauSize, zkey, zkeySize, device, &rep, ms, v);
            copyErr(errorMsg, errorMsgMax, v.message.c_str());
        }) != UG_OK) {
        memset(&rep, 0, sizeof rep);              // (a refusal reports nothing)
        if (located) memset(located, 0, sizeof *located);
        rc = UG_ERROR;
    }
    if (out) *out = rep;
    if (phaseMs) for (int i = 0; i < PHASES; i++) phaseMs[i] = ms[i];
    return rc;
}

// a fold entry: the circuit parsed and planned, then the fold on host threads or the device. K = 2 (cls null) hands out the first
// six of its eight vectors, K = 3 all eleven
int foldEntry(const void* r1cs, u64 r1csSize, const void* rho, const void* cls, int K, u32 logDomain, int device, void* out, double* kernelMs,
              char* errorMsg, unsigned long long errorMsgMax) {
    return guarded(R1CS_RULE, errorMsg, errorMsgMax, [&] {
        if (kernelMs) *kernelMs = 0;
        if (!r1cs || !rho || (K == 3 && !cls) || !out) throw R1csRefusal("null buffer");
        const std::unique_ptr<BinFile> f = openBinFile(r1cs, r1csSize, "r1cs", "r1cs: ", "null buffer");
        R1cs cs;
        loadR1cs(*f, cs);
        const u64 nPublic = (u64)cs.hdr.nPubOut + cs.hdr.nPubIn;
        if (nPublic + 1 > cs.hdr.nWires) throw R1csRefusal("nPubOut + nPubIn + 1 exceeds nWires");
        const uint8_t* c = (const uint8_t*)cls;
        for (u64 s = 0; c && s < cs.hdr.nWires; s++)
            if (c[s] > 2) throw R1csRefusal("class " + std::to_string(c[s]) + " of wire " + std::to_string(s) + " is not 0, 1 or 2");
        Plan p;
        planSizes(cs.hdr, logDomain, p);
        std::vector<uint8_t> all;
        uint8_t* dst = (uint8_t*)out;
        if (K == 2) { all.resize((size_t)p.N * 32 * foldVectors(2)); dst = all.data(); }
        double ms = 0;
        if (device < 0) {
            const double t0 = nowMs();
            hostFold(cs, (const uint8_t*)rho, c, (u32)nPublic, p.N, dst);
            ms = nowMs() - t0;
        } else {
            if (!deviceFold) throw R1csRefusal("this program has no device path: use device = -1 (host threads)");
            deviceFold(device, r1cs, r1csSize, (const uint8_t*)rho, c, (u32)nPublic, (u32)p.logN, dst, &ms);
        }
        if (K == 2) memcpy(out, all.data(), (size_t)p.N * 32 * 6);
        if (kernelMs) *kernelMs = ms;
    });
}

}  // namespace
}  // namespace zkv
}  // namespace ughost

// =====================================================================================================================
using namespace ughost::zkv;

extern "C" {

int ug_zkey_verify_run(const ug_zkey_verify_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                       const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, double* phase_ms, char* error_msg,
                       unsigned long long error_msg_maxsize) {
    return verifyEntry(opt, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, out, phase_ms, error_msg, error_msg_maxsize);
}

int ug_ultra_zkey_verify_run(const ug_ultra_zkey_verify_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                             uint64_t ptau_size, const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, double* phase_ms,
                             char* error_msg, unsigned long long error_msg_maxsize) {
    return verifyEntry(opt, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, out, phase_ms, error_msg, error_msg_maxsize);
}

int ug_zkey_locate_run(const ug_zkey_locate_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                       const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, ug_zkey_locate_report* located,
                       double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    ug_zkey_verify_options v;
    memset(&v, 0, sizeof v);
    if (opt) v.validate = opt->validate;
    return locateEntry(opt, v, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, out, located, phase_ms, error_msg, error_msg_maxsize);
}

int ug_ultra_zkey_locate_run(const ug_ultra_zkey_locate_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                             uint64_t ptau_size, const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out,
                             ug_zkey_locate_report* located, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    ug_ultra_zkey_verify_options v;
    memset(&v, 0, sizeof v);
    if (opt) {
        v.validate = opt->validate; v.check_spec = opt->check_spec; v.rand_indx = opt->rand_indx;
        v.round_signals = opt->round_signals; v.n_round = opt->n_round;
        v.final_signals = opt->final_signals; v.n_final = opt->n_final;
    }
    return locateEntry(opt, v, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, out, located, phase_ms, error_msg, error_msg_maxsize);
}

int ug_r1cs_fold(const void* r1cs, uint64_t r1cs_size, const void* rho, uint32_t log_domain, int device, void* out, double* kernel_ms,
                 char* error_msg, unsigned long long error_msg_maxsize) {
    return foldEntry(r1cs, r1cs_size, rho, nullptr, 2, log_domain, device, out, kernel_ms, error_msg, error_msg_maxsize);
}

int ug_r1cs_fold_classes(const void* r1cs, uint64_t r1cs_size, const void* rho, const void* cls, uint32_t log_domain, int device, void* out,
                         double* kernel_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    return foldEntry(r1cs, r1cs_size, rho, cls, 3, log_domain, device, out, kernel_ms, error_msg, error_msg_maxsize);
}

}  // extern "C"
