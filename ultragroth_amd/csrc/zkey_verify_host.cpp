// zkey_verify_host.cpp -- is this Groth16 key the one its circuit and a prepared powers-of-tau file give under ONE delta?
// (include/ultragroth_hip.h: ug_zkey_verify_run, ug_r1cs_fold). No trapdoor and no delta is known here. Out of scope: who
// contributed -- section 10's transcript, beacons, the .ptau's own ceremony. UltraGroth keys have an entry of their own at the end
// of this file (ug_ultra_zkey_verify_run, ug_r1cs_fold_classes): the same check with three weight classes and two deltas.
//
// Making the key again costs a point combination per wire. The check draws a 128-bit weight rho_s per wire and moves the weights
// to the SCALAR side: sum_s rho_s A_s = sum_k (A rho)_k T[k], so one sparse matrix-vector product over Fr (the fold) and a few
// MSMs over the level-n slices stand against one MSM over each section of the key; H needs no matrix at all. The relations and
// their soundness are in DESIGN.md section 5.11; the notation is ug_setup_ptau_run's.
//
// This file is the host layer and the host twin (device = -1): the files' rules, the point check, relation 0 (header) and
// relation 1 (section 4, through setup_host.cpp's own writer), the weights, the pairings (pairing.hpp, host threads wherever the
// sums were made) and the verdict. The twelve sums come from host threads here or from the device (zkey_verify.hip), as
// canonical affine records, so the two agree byte for byte.
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
DeviceSums deviceUltraSums = nullptr;
DeviceFoldClasses deviceFoldClasses = nullptr;

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

// ---- the fold on host threads: the witness check's row walk with rho in the witness's place and two sums per matrix ----
// out8: eight vectors of N plain canonical integers: a^pub, b^pub, c^pub, a^priv, b^priv, c^priv, a, b
void hostFold(const R1cs& cs, const uint8_t* rho, u32 nPublic, u64 N, uint8_t* out8) {
    const u64 M = cs.hdr.nWires, rows = cs.hdr.nConstraints;
    std::vector<Fr> w((size_t)M);
    parallelFor(M, 4096, [&](u64 lo, u64 hi) {
        for (u64 s = lo; s < hi; s++) w[(size_t)s] = frFromPlain(rho + s * 32);
    });
    memset(out8, 0, (size_t)N * 32 * 8);
    auto at = [&](int v, u64 k) { return out8 + ((size_t)v * N + k) * 32; };
    parallelFor(N, 1024, [&](u64 lo, u64 hi) {
        for (u64 k = lo; k < hi; k++) {
            if (k >= rows) {
                if (k - rows <= nPublic) { frToPlain(at(0, k), w[(size_t)(k - rows)]); memcpy(at(6, k), at(0, k), 32); }
                continue;
            }
            for (int t = 0; t < 3; t++) {
                const R1csMatrix& m = cs.m[t];
                Fr acc[2] = {fp_zero<FrParams>(), fp_zero<FrParams>()};
                for (u32 q = m.rowPtr[k]; q < m.rowPtr[k + 1]; q++) {
                    const int side = m.sig[q] > nPublic ? 1 : 0;
                    acc[side] = frAdd(acc[side], frMul(frFromPlain(&m.val[(size_t)q * 32]), w[m.sig[q]]));
                }
                frToPlain(at(t, k), acc[0]);
                frToPlain(at(3 + t, k), acc[1]);
                if (t < 2) frToPlain(at(6 + t, k), frAdd(acc[0], acc[1]));
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
    std::vector<uint8_t> f((size_t)N * 32 * 8);
    hostFold(*in.cs, in.rho, (u32)(pub - 1), N, f.data());
    st.foldKernelMs = nowMs() - t0;
    clock.lap(0);
    auto vec = [&](int v) { return f.data() + (size_t)v * N * 32; };
    hostMsm(false, vec(6), in.T, N, out.aT);
    hostMsm(false, vec(7), in.T, N, out.bT);
    hostMsm(true, vec(7), in.T2, N, out.bT2);
    PointSegs three;                             // [a^m | b^m | c^m] over [bT | aT | T]
    three.count = N; three.n = 3;
    three.base[0] = in.bT; three.base[1] = in.aT; three.base[2] = in.T;
    hostMsm(false, vec(0), three, out.kPub);
    hostMsm(false, vec(3), three, out.kPriv);
    clock.lap(1);
    hostMsm(false, in.rho, in.a, M, out.keyA);
    hostMsm(false, in.rho, in.b1, M, out.keyB1);
    hostMsm(true, in.rho, in.b2, M, out.keyB2);
    hostMsm(false, in.rho, in.ic, pub, out.keyIC);
    hostMsm(false, in.rho + pub * 32, in.c, M - pub, out.keyC);
    clock.lap(2);
    hostMsm(false, in.sigma, in.h, N, out.keyH);
    hostMsm(false, in.sigma, hOdd, N, out.hP);
    clock.lap(3);
}

// ---- pairings (pairing.hpp, host threads) ----
const FinalExpConsts& consts() { static const FinalExpConsts c = final_exp_consts(); return c; }
F1 coord(const uint8_t* le) {
    u32 w[8];
    memcpy(w, le, 32);
    return F1{cond_sub_q(from_mont256<FqParams>(w))};
}
G1A g1Of(const uint8_t* rec) {
    if (allZero(rec, 64)) return G1A{f1_zero(), f1_zero(), true};
    return G1A{coord(rec), coord(rec + 32), false};
}
G2A g2Of(const uint8_t* rec) {
    if (allZero(rec, 128)) return g2_inf();
    return G2A{F2{coord(rec), coord(rec + 32)}, F2{coord(rec + 64), coord(rec + 96)}, false};
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

// ---- the point check of the key, with ug_zkey_check's messages ----
const char* const HEADER_NAMES[6] = {"alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"};
void checkKeyPoints(const PointCheck& check, const ZkeyHeader& h, const Inputs& in) {
    const uint8_t* hp[6] = {h.alpha1, h.beta1, h.beta2, h.gamma2, h.delta1, h.delta2};
    const bool hg2[6] = {false, false, true, true, false, true};
    for (int i = 0; i < 6; i++) {
        uint8_t rec[128];                        // (the header's points sit at any alignment)
        memcpy(rec, hp[i], hg2[i] ? 128 : 64);
        const ug_point_fault f = check.find(hg2[i], rec, 1);
        if (f.reason) throw ZkeyError(std::string("header point ") + HEADER_NAMES[i] + ": " + PointCheck::reasonText(f.reason));
    }
    struct Sec { u32 id; bool g2; const uint8_t* p; u64 n; };
    const Sec secs[6] = {{3, false, in.ic, in.pub}, {5, false, in.a, in.M}, {6, false, in.b1, in.M}, {7, true, in.b2, in.M},
                         {8, false, in.c, in.M - in.pub}, {9, false, in.h, in.N}};
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

void checkOptions(const ug_zkey_verify_options* o) {
    checkOptionsHead<ZkeyError>(o, 1, 2, "1 or 2");
}

// 0: valid, UG_ZKEY_INVALID: *v says which sections fail; a refusal is an exception
int run(const ug_zkey_verify_options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, const void* zkey, u64 zkeySize,
        int device, ug_zkey_verify_report* rep, double ms[PHASES], Verdict& v) {
    PhaseClock clock(ms);
    checkOptions(opt);
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
        if (zf->sectionSize(1) < 4) throw ZkeyError("section 1 is too short");
        u32 protocol = 0;
        memcpy(&protocol, zf->sectionData(1), 4);
        if (protocol == 1337) throw ZkeyError("protocol 1337 keys are not checked");
        zh = loadZkeyHeader(*zf, false);
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
    Inputs in;
    in.M = M; in.N = N; in.pub = pub; in.logN = logN;
    in.r1cs = r1cs; in.r1csSize = r1csSize; in.cs = &cs;
    const uint8_t* coefs = nullptr;
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
        in.c = sectionOf(*zf, 8, (M - pub) * 64);
        in.h = sectionOf(*zf, 9, N * 64);
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
        const PointCheck check(device, (int)opt->validate);
        checkSlices(check, sl, hOdd.data());
        checkKeyPoints(check, zh, in);
    }
    rep->subgroup_checked = opt->validate >= 2 ? 1 : 0;
    clock.lap(1);

    std::vector<uint8_t> rho, sigma;
    drawWeights(rho, M);
    drawWeights(sigma, N);
    in.rho = rho.data(); in.sigma = sigma.data();
    clock.lap(2);

    // ---- relation 0: the header ----
    const G1A g1 = g1Generator();
    const G2A g2 = g2Generator();
    const G1A delta1 = g1Of(zh.delta1);
    const G2A delta2 = g2Of(zh.delta2), gamma2 = g2Of(zh.gamma2);
    auto deltaPair = std::async(std::launch::async, [&] { return samePairing(delta1, g2, g1, delta2); });
    {
        const char* what = nullptr;
        if (memcmp(zh.alpha1, sl.alpha1, 64) != 0) what = "alpha1 is not the powers of tau's";
        else if (memcmp(zh.beta1, sl.beta1, 64) != 0) what = "beta1 is not the powers of tau's";
        else if (memcmp(zh.beta2, sl.beta2, 128) != 0) what = "beta2 is not the powers of tau's";
        else if (delta1.inf) what = "delta1 is the point at infinity";
        else if (delta2.inf) what = "delta2 is the point at infinity";
        else if (gamma2.inf) what = "gamma2 is the point at infinity";
        else if (!deltaPair.get()) what = "delta1 and delta2 are not the same delta";
        if (what) v.fail(2, std::string("zkey: header: ") + what);
        if (deltaPair.valid()) deltaPair.get();
    }
    // ---- relation 1: section 4 is the one setup_host.cpp writes for this circuit ----
    {
        std::vector<u64> perPiece;
        const u64 nCoefs = pub + countCoefs(cs, perPiece);
        Plan p;
        planSizes(cs.hdr, (u32)logN, p);
        std::vector<uint8_t> want((size_t)nCoefs * 44);
        writeCoefs(cs, p, perPiece, want.data());
        const u64 common = std::min(nCoefs, keyCoefs);
        u64 bad = common;
        for (u64 i = 0; i < common; i++)
            if (memcmp(&want[(size_t)i * 44], coefs + i * 44, 44) != 0) { bad = i; break; }
        if (bad < common || nCoefs != keyCoefs || zf->sectionSize(4) != 4 + keyCoefs * 44)
            v.fail(4, "zkey: section 4 record " + std::to_string(bad) + ": does not match the circuit");
    }
    clock.lap(0);

    // ---- the sums of relations 2 - 7 ----
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
    auto secFail = [&](int id, bool delta) { v.fail(id, "zkey: section " + std::to_string(id) + TEXT + (delta ? " under the key's delta" : "")); };
    const G1A keyIC = g1Of(s.keyIC), kPub = g1Of(s.kPub), keyC = g1Of(s.keyC), kPriv = g1Of(s.kPriv), keyH = g1Of(s.keyH), hP = g1Of(s.hP);
    auto rel3 = std::async(std::launch::async, [&] { return samePairing(keyIC, gamma2, kPub, g2); });
    auto rel8 = std::async(std::launch::async, [&] { return samePairing(keyC, delta2, kPriv, g2); });
    auto rel9 = std::async(std::launch::async, [&] { return samePairing(keyH, delta2, hP, g2); });
    if (memcmp(s.keyA, s.aT, 64) != 0) secFail(5, false);
    if (memcmp(s.keyB1, s.bT, 64) != 0) secFail(6, false);
    if (memcmp(s.keyB2, s.bT2, 128) != 0) secFail(7, false);
    const bool ok3 = rel3.get(), ok8 = rel8.get(), ok9 = rel9.get();
    if (!ok3) secFail(3, false);
    if (!ok8) secFail(8, true);
    if (!ok9) secFail(9, true);
    clock.lap(7);
    rep->failed_sections = v.failed;
    rep->first_failed = v.first;
    return v.failed ? UG_ZKEY_INVALID : UG_OK;
}

// ================================================ an UltraGroth key (protocol 1337) ================================================
// The same check with two deltas: the wires fall in three classes -- public, the key's own round list, its own final list -- the
// fold keeps three sums per matrix, and each C section stands under its own delta. DESIGN.md section 5.12.

// out11: eleven vectors of N plain canonical integers: vector 3 m + t is matrix t over class m (pub, round, final); 9 is a, 10 is b
void hostFoldClasses(const R1cs& cs, const uint8_t* rho, const uint8_t* cls, u32 nPublic, u64 N, uint8_t* out11) {
    const u64 M = cs.hdr.nWires, rows = cs.hdr.nConstraints;
    std::vector<Fr> w((size_t)M);
    parallelFor(M, 4096, [&](u64 lo, u64 hi) {
        for (u64 s = lo; s < hi; s++) w[(size_t)s] = frFromPlain(rho + s * 32);
    });
    memset(out11, 0, (size_t)N * 32 * 11);
    auto at = [&](int v, u64 k) { return out11 + ((size_t)v * N + k) * 32; };
    parallelFor(N, 1024, [&](u64 lo, u64 hi) {
        for (u64 k = lo; k < hi; k++) {
            if (k >= rows) {
                if (k - rows <= nPublic) { frToPlain(at(0, k), w[(size_t)(k - rows)]); memcpy(at(9, k), at(0, k), 32); }
                continue;
            }
            for (int t = 0; t < 3; t++) {
                const R1csMatrix& m = cs.m[t];
                Fr acc[3] = {fp_zero<FrParams>(), fp_zero<FrParams>(), fp_zero<FrParams>()};
                for (u32 q = m.rowPtr[k]; q < m.rowPtr[k + 1]; q++) {
                    const int side = cls[m.sig[q]] == 0 ? 0 : cls[m.sig[q]] == 1 ? 1 : 2;
                    acc[side] = frAdd(acc[side], frMul(frFromPlain(&m.val[(size_t)q * 32]), w[m.sig[q]]));
                }
                for (int c = 0; c < 3; c++) frToPlain(at(3 * c + t, k), acc[c]);
                if (t < 2) frToPlain(at(9 + t, k), frAdd(frAdd(acc[0], acc[1]), acc[2]));
            }
        }
    });
}

void hostUltraSums(const Inputs& in, const uint8_t* hOdd, Sums& out, SumsStats& st) {
    PhaseClock clock(st.ms);
    const double t0 = nowMs();
    const u64 N = in.N, M = in.M, pub = in.pub;
    std::vector<uint8_t> f((size_t)N * 32 * 11);
    hostFoldClasses(*in.cs, in.rho, in.cls, (u32)(pub - 1), N, f.data());
    st.foldKernelMs = nowMs() - t0;
    clock.lap(0);
    auto vec = [&](int v) { return f.data() + (size_t)v * N * 32; };
    hostMsm(false, vec(9), in.T, N, out.aT);
    hostMsm(false, vec(10), in.T, N, out.bT);
    hostMsm(true, vec(10), in.T2, N, out.bT2);
    PointSegs three;                             // [a^m | b^m | c^m] over [bT | aT | T]
    three.count = N; three.n = 3;
    three.base[0] = in.bT; three.base[1] = in.aT; three.base[2] = in.T;
    hostMsm(false, vec(0), three, out.kPub);
    hostMsm(false, vec(3), three, out.kPriv);
    hostMsm(false, vec(6), three, out.kFinal);
    clock.lap(1);
    hostMsm(false, in.rho, in.a, M, out.keyA);
    hostMsm(false, in.rho, in.b1, M, out.keyB1);
    hostMsm(true, in.rho, in.b2, M, out.keyB2);
    hostMsm(false, in.rho, in.ic, pub, out.keyIC);
    hostMsm(false, in.rhoRound, in.c, in.n1, out.keyC);
    hostMsm(false, in.rhoFinal, in.c2, in.n2, out.keyC2);
    clock.lap(2);
    hostMsm(false, in.sigma, in.h, N, out.keyH);
    hostMsm(false, in.sigma, hOdd, N, out.hP);
    clock.lap(3);
}

void checkOptions(const ug_ultra_zkey_verify_options* o) {
    checkOptionsHead<ZkeyError>(o, 1, 2, "1 or 2");
    if (o->check_spec > 1) throw ZkeyError("check_spec " + std::to_string(o->check_spec) + " is not 0 or 1");
    if (o->check_spec && ((o->n_round && !o->round_signals) || (o->n_final && !o->final_signals))) throw ZkeyError("null signal list");
}

// run() for protocol 1337; the report's failed_sections has bits 2 - 12
int runUltra(const ug_ultra_zkey_verify_options* opt, const void* r1cs, u64 r1csSize, const void* ptau, u64 ptauSize, const void* zkey,
             u64 zkeySize, int device, ug_zkey_verify_report* rep, double ms[PHASES], Verdict& v) {
    PhaseClock clock(ms);
    checkOptions(opt);
    if (device >= 0 && !deviceUltraSums) throw ZkeyError("this program has no device path: use device = -1 (host threads)");
    // ---- every size and header rule of the three files, before the first device byte ----
    std::unique_ptr<BinFile> rf;
    R1cs cs;
    under(R1CS_RULE, [&] { loadCircuit(r1cs, r1csSize, rf, cs.hdr); });
    const u64 M = cs.hdr.nWires, nPublic = (u64)cs.hdr.nPubOut + cs.hdr.nPubIn, pub = nPublic + 1;
    if (pub > M) throw R1csRefusal("nPubOut + nPubIn + 1 exceeds nWires");
    const u64 rows = (u64)cs.hdr.nConstraints + pub;

    const std::unique_ptr<BinFile> zf = openBinFile(zkey, zkeySize, "zkey", "zkey: ", "null zkey buffer");
    ZkeyHeader zh;
    under(ZKEY_RULE, [&] { zh = loadZkeyHeader(*zf, true); });      // ("zkey file is not ultragroth" for a Groth16 key)
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
    const u64 n1 = zh.numIndexesC1, n2 = zh.numIndexesC2;
    Inputs in;
    in.ultra = true;
    in.M = M; in.N = N; in.pub = pub; in.logN = logN; in.n1 = n1; in.n2 = n2;
    in.r1cs = r1cs; in.r1csSize = r1csSize; in.cs = &cs;
    const uint8_t *coefs = nullptr, *list1 = nullptr, *list2 = nullptr;
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
        in.c = sectionOf(*zf, 8, n1 * 64);
        in.c2 = sectionOf(*zf, 9, n2 * 64);
        list1 = sectionOf(*zf, 10, n1 * 4);
        list2 = sectionOf(*zf, 11, n2 * 4);
        in.h = sectionOf(*zf, 12, N * 64);
    });
    // the key's own rounds: rand_indx public, the lists a partition of the private signals (planLists' rules and texts)
    Plan plan;
    std::vector<u32> roundList((size_t)n1), finalList((size_t)n2);
    if (n1) memcpy(roundList.data(), list1, (size_t)n1 * 4);
    if (n2) memcpy(finalList.data(), list2, (size_t)n2 * 4);
    under(ZKEY_RULE, [&] {
        planSizes(cs.hdr, (u32)logN, plan);
        planLists(plan, zh.randIndx, roundList.data(), n1, finalList.data(), n2);
    });
    in.cls = plan.cls.data();

    const std::unique_ptr<BinFile> pf = openBinFile(ptau, ptauSize, "ptau", "ptau: ", "null ptau buffer");
    const PtauHeader ph = loadPtauHeader(*pf);
    const PtauSlices sl = loadPtauSlices(*pf, ph, (u32)logN);
    in.T = sl.tau1; in.T2 = sl.tau2; in.aT = sl.alphaTau1; in.bT = sl.betaTau1; in.top = sl.top;
    under(R1CS_RULE, [&] { loadR1cs(*rf, cs); });
    std::vector<uint8_t> hOdd((size_t)N * 64);
    gatherOddTop(sl, hOdd.data());
    clock.lap(0);

    // ---- every point of the key and of the slices, before any relation ----
    {
        const PointCheck check(device, (int)opt->validate);
        checkSlices(check, sl, hOdd.data());
        const uint8_t* hp[8] = {zh.alpha1, zh.beta1, zh.beta2, zh.gamma2, zh.roundDelta1, zh.roundDelta2, zh.delta1, zh.delta2};
        const bool hg2[8] = {false, false, true, true, false, true, false, true};
        const char* const names[8] = {"alpha1", "beta1", "beta2", "gamma2", "delta_c1_1", "delta_c1_2", "delta_c2_1", "delta_c2_2"};
        for (int i = 0; i < 8; i++) {
            uint8_t rec[128];
            memcpy(rec, hp[i], hg2[i] ? 128 : 64);
            const ug_point_fault f = check.find(hg2[i], rec, 1);
            if (f.reason) throw ZkeyError(std::string("header point ") + names[i] + ": " + PointCheck::reasonText(f.reason));
        }
        struct Sec { u32 id; bool g2; const uint8_t* p; u64 n; };
        const Sec secs[7] = {{3, false, in.ic, pub}, {5, false, in.a, M}, {6, false, in.b1, M}, {7, true, in.b2, M},
                             {8, false, in.c, n1}, {9, false, in.c2, n2}, {12, false, in.h, N}};
        for (const Sec& s : secs) {
            const ug_point_fault f = check.find(s.g2, s.p, s.n);
            if (f.reason)
                throw ZkeyError("section " + std::to_string(s.id) + " point " + std::to_string(f.index) + ": " + PointCheck::reasonText(f.reason));
        }
    }
    rep->subgroup_checked = opt->validate >= 2 ? 1 : 0;
    clock.lap(1);

    std::vector<uint8_t> rho, sigma;
    drawWeights(rho, M);
    drawWeights(sigma, N);
    // the weights of a list's signals, in the list's order (a host step: 32 bytes per private signal)
    std::vector<uint8_t> rhoRound((size_t)n1 * 32), rhoFinal((size_t)n2 * 32);
    for (u64 i = 0; i < n1; i++) memcpy(&rhoRound[(size_t)i * 32], &rho[(size_t)roundList[(size_t)i] * 32], 32);
    for (u64 i = 0; i < n2; i++) memcpy(&rhoFinal[(size_t)i * 32], &rho[(size_t)finalList[(size_t)i] * 32], 32);
    in.rho = rho.data(); in.sigma = sigma.data(); in.rhoRound = rhoRound.data(); in.rhoFinal = rhoFinal.data();
    clock.lap(2);

    // ---- step 0: the header ----
    const G1A g1 = g1Generator();
    const G2A g2 = g2Generator();
    const G1A dr1 = g1Of(zh.roundDelta1), df1 = g1Of(zh.delta1);
    const G2A dr2 = g2Of(zh.roundDelta2), df2 = g2Of(zh.delta2), gamma2 = g2Of(zh.gamma2);
    {
        auto roundPair = std::async(std::launch::async, [&] { return samePairing(dr1, g2, g1, dr2); });
        const bool finalPair = samePairing(df1, g2, g1, df2);
        const bool roundOk = roundPair.get();
        const char* what = nullptr;
        if (memcmp(zh.alpha1, sl.alpha1, 64) != 0) what = "alpha1 is not the powers of tau's";
        else if (memcmp(zh.beta1, sl.beta1, 64) != 0) what = "beta1 is not the powers of tau's";
        else if (memcmp(zh.beta2, sl.beta2, 128) != 0) what = "beta2 is not the powers of tau's";
        else if (gamma2.inf) what = "gamma2 is the point at infinity";
        else if (dr1.inf || dr2.inf) what = "delta_c1 is the point at infinity";
        else if (df1.inf || df2.inf) what = "delta_c2 is the point at infinity";
        else if (!roundOk) what = "delta_c1's G1 and G2 points are not the same delta";
        else if (!finalPair) what = "delta_c2's G1 and G2 points are not the same delta";
        if (what) v.fail(2, std::string("zkey: header: ") + what);
    }
    // ---- step 1: section 4 ----
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
    // ---- step 2: the lists against a spec, where one is given ----
    if (opt->check_spec) {
        if (zh.randIndx != opt->rand_indx) v.fail(2, "zkey: header: rand_indx does not match the spec");
        if (n1 != opt->n_round || (n1 && memcmp(roundList.data(), opt->round_signals, (size_t)n1 * 4) != 0)) v.fail(10, "zkey: section 10: does not match the spec");
        if (n2 != opt->n_final || (n2 && memcmp(finalList.data(), opt->final_signals, (size_t)n2 * 4) != 0)) v.fail(11, "zkey: section 11: does not match the spec");
    }
    clock.lap(0);

    Sums s;
    memset(&s, 0, sizeof s);
    SumsStats st;
    if (device < 0) hostUltraSums(in, hOdd.data(), s, st);
    else deviceUltraSums(device, in, s, st);
    for (int i = 0; i < 4; i++) ms[3 + i] += st.ms[i];
    rep->fold_kernel_ms = st.foldKernelMs;
    rep->peak_device_bytes = st.peakDeviceBytes;
    clock.restart();

    const char* const TEXT = ": does not match the circuit and the powers of tau";
    auto secFail = [&](int id, const char* tail) { v.fail(id, "zkey: section " + std::to_string(id) + TEXT + tail); };
    const G1A keyIC = g1Of(s.keyIC), kPub = g1Of(s.kPub), keyC1 = g1Of(s.keyC), kRound = g1Of(s.kPriv), keyC2 = g1Of(s.keyC2), kFinal = g1Of(s.kFinal),
              keyH = g1Of(s.keyH), hP = g1Of(s.hP);
    auto rel3 = std::async(std::launch::async, [&] { return samePairing(keyIC, gamma2, kPub, g2); });
    auto rel8 = std::async(std::launch::async, [&] { return samePairing(keyC1, dr2, kRound, g2); });
    auto rel9 = std::async(std::launch::async, [&] { return samePairing(keyC2, df2, kFinal, g2); });
    auto rel12 = std::async(std::launch::async, [&] { return samePairing(keyH, df2, hP, g2); });
    if (memcmp(s.keyA, s.aT, 64) != 0) secFail(5, "");
    if (memcmp(s.keyB1, s.bT, 64) != 0) secFail(6, "");
    if (memcmp(s.keyB2, s.bT2, 128) != 0) secFail(7, "");
    const bool ok3 = rel3.get(), ok8 = rel8.get(), ok9 = rel9.get(), ok12 = rel12.get();
    if (!ok3) secFail(3, "");
    if (!ok8) secFail(8, " under the key's round delta");       // (an empty list: both sums are infinity and the relation holds)
    if (!ok9) secFail(9, " under the key's final delta");
    if (!ok12) secFail(12, " under the key's final delta");
    clock.lap(7);
    rep->failed_sections = v.failed;
    rep->first_failed = v.first;
    return v.failed ? UG_ZKEY_INVALID : UG_OK;
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
    ug_zkey_verify_report rep;
    memset(&rep, 0, sizeof rep);
    double ms[UG_ZKEY_VERIFY_PHASES] = {0};
    int rc = UG_ERROR;
    if (guarded(ZKEY_RULE, error_msg, error_msg_maxsize, [&] {
            Verdict v;
            rc = run(opt, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, &rep, ms, v);
            copyErr(error_msg, error_msg_maxsize, v.message.c_str());
        }) != UG_OK) {
        memset(&rep, 0, sizeof rep);              // (a refusal reports nothing)
        rc = UG_ERROR;
    }
    if (out) *out = rep;
    if (phase_ms) for (int i = 0; i < UG_ZKEY_VERIFY_PHASES; i++) phase_ms[i] = ms[i];
    return rc;
}

int ug_r1cs_fold(const void* r1cs, uint64_t r1cs_size, const void* rho, uint32_t log_domain, int device, void* out, double* kernel_ms,
                 char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(R1CS_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) *kernel_ms = 0;
        if (!r1cs || !rho || !out) throw R1csRefusal("null buffer");
        const std::unique_ptr<ughost::BinFile> f = ughost::openBinFile(r1cs, r1cs_size, "r1cs", "r1cs: ", "null buffer");
        ughost::R1cs cs;
        ughost::loadR1cs(*f, cs);
        const uint64_t nPublic = (uint64_t)cs.hdr.nPubOut + cs.hdr.nPubIn;
        if (nPublic + 1 > cs.hdr.nWires) throw R1csRefusal("nPubOut + nPubIn + 1 exceeds nWires");
        Plan p;
        planSizes(cs.hdr, log_domain, p);
        std::vector<uint8_t> all((size_t)p.N * 32 * 8);
        double ms = 0;
        if (device < 0) {
            const double t0 = nowMs();
            hostFold(cs, (const uint8_t*)rho, (uint32_t)nPublic, p.N, all.data());
            ms = nowMs() - t0;
        } else {
            if (!deviceFold) throw R1csRefusal("this program has no device path: use device = -1 (host threads)");
            deviceFold(device, r1cs, r1cs_size, (const uint8_t*)rho, (uint32_t)nPublic, (uint32_t)p.logN, all.data(), &ms);
        }
        memcpy(out, all.data(), (size_t)p.N * 32 * 6);
        if (kernel_ms) *kernel_ms = ms;
    });
}

int ug_ultra_zkey_verify_run(const ug_ultra_zkey_verify_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                             uint64_t ptau_size, const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, double* phase_ms,
                             char* error_msg, unsigned long long error_msg_maxsize) {
    ug_zkey_verify_report rep;
    memset(&rep, 0, sizeof rep);
    double ms[UG_ZKEY_VERIFY_PHASES] = {0};
    int rc = UG_ERROR;
    if (guarded(ZKEY_RULE, error_msg, error_msg_maxsize, [&] {
            Verdict v;
            rc = runUltra(opt, r1cs, r1cs_size, ptau, ptau_size, zkey, zkey_size, device, &rep, ms, v);
            copyErr(error_msg, error_msg_maxsize, v.message.c_str());
        }) != UG_OK) {
        memset(&rep, 0, sizeof rep);              // (a refusal reports nothing)
        rc = UG_ERROR;
    }
    if (out) *out = rep;
    if (phase_ms) for (int i = 0; i < UG_ZKEY_VERIFY_PHASES; i++) phase_ms[i] = ms[i];
    return rc;
}

int ug_r1cs_fold_classes(const void* r1cs, uint64_t r1cs_size, const void* rho, const void* cls, uint32_t log_domain, int device, void* out,
                         double* kernel_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(R1CS_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) *kernel_ms = 0;
        if (!r1cs || !rho || !cls || !out) throw R1csRefusal("null buffer");
        const std::unique_ptr<ughost::BinFile> f = ughost::openBinFile(r1cs, r1cs_size, "r1cs", "r1cs: ", "null buffer");
        ughost::R1cs cs;
        ughost::loadR1cs(*f, cs);
        const uint64_t nPublic = (uint64_t)cs.hdr.nPubOut + cs.hdr.nPubIn;
        if (nPublic + 1 > cs.hdr.nWires) throw R1csRefusal("nPubOut + nPubIn + 1 exceeds nWires");
        const uint8_t* c = (const uint8_t*)cls;
        for (uint64_t s = 0; s < cs.hdr.nWires; s++)
            if (c[s] > 2) throw R1csRefusal("class " + std::to_string(c[s]) + " of wire " + std::to_string(s) + " is not 0, 1 or 2");
        Plan p;
        planSizes(cs.hdr, log_domain, p);
        double ms = 0;
        if (device < 0) {
            const double t0 = nowMs();
            hostFoldClasses(cs, (const uint8_t*)rho, c, (uint32_t)nPublic, p.N, (uint8_t*)out);
            ms = nowMs() - t0;
        } else {
            if (!deviceFoldClasses) throw R1csRefusal("this program has no device path: use device = -1 (host threads)");
            deviceFoldClasses(device, r1cs, r1cs_size, (const uint8_t*)rho, c, (uint32_t)nPublic, (uint32_t)p.logN, (uint8_t*)out, &ms);
        }
        if (kernel_ms) *kernel_ms = ms;
    });
}

}  // extern "C"
