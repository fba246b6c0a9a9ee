// ptau_prepare_host.cpp -- preparing a powers-of-tau file for phase 2 (include/ultragroth_hip.h: ug_ptau_prepare_*, ug_points_intt):
// sections 12 - 15, the Lagrange forms, from sections 2 - 5, the powers; and the check that a file's sections 12 - 15 are those of
// its own powers, which ug_setup_ptau_run takes on trust. What `snarkjs powersoftau prepare phase2` does. Out of scope:
// contribution transcripts, beacons, verifying the ceremony's own contributions.
//
// The reader is host_util.cpp's (loadPtauHeader, loadPtauPowers, loadPtauLagrange), the point check is point_check.cpp's. The one
// heavy step, an inverse transform whose elements are points, sits behind Backend::intt: host threads (setup_host.cpp) or kernels
// (ptau_prepare.hip). A level p is one call of it over the first 2^p records; sections 12, 14 and 15 of a level go in one call.
#include "setup_host.hpp"

#include <algorithm>
#include <memory>

namespace ughost {
namespace setup {

using namespace ug;

namespace {

constexpr int PREP_PHASES = UG_PTAU_PREPARE_PHASES;
constexpr u32 MAX_INTT_LOG = 28;                 // the two-adicity of r
const u32 LAGRANGE_IDS[4] = {12, 13, 14, 15};
const u64 LAGRANGE_REC[4] = {64, 128, 64, 64};

bool isLagrange(u32 id) { return id >= 12 && id <= 15; }

// the prepared file: the sections that are kept, in the input's order (payload sizes after the cut), then 12 - 15
struct Prepared {
    PtauHeader hdr;
    PtauPowers pw;
    bool cut = false;
    std::vector<std::pair<u32, Section>> kept;
    u64 records[4] = {0, 0, 0, 0};               // of sections 12 - 15
    u64 offset[4] = {0, 0, 0, 0};                // of their payloads in the output
    u64 total = 0;
};

void checkOptions(const ug_ptau_prepare_options* o) {
    checkOptionsHead<SetupError>(o, 0, 2, "0, 1 or 2");
    if (o->mode > 1) throw SetupError("mode " + std::to_string(o->mode) + " is not 0 or 1");
}

// every rule that needs no point
void plan(const ug_ptau_prepare_options* opt, const void* ptau, u64 ptauSize, std::unique_ptr<BinFile>& f, Prepared& p) {
    checkOptions(opt);
    f = openBinFile(ptau, ptauSize, "ptau", "ptau: ", "null ptau buffer");
    p.hdr = loadPtauHeader(*f);
    if (opt->mode == 1 && opt->power && opt->power != p.hdr.power)
        throw PtauError("power " + std::to_string(opt->power) + ": a check is of the file's own power " + std::to_string(p.hdr.power));
    // section 12's padded level is a transform of 2^(power+1) points, and r - 1 has only 28 factors of 2
    if (opt->power <= p.hdr.power && (opt->power ? opt->power : p.hdr.power) >= MAX_INTT_LOG)
        throw PtauError("power " + std::to_string(MAX_INTT_LOG) + ": the padded level of section 12 would need a root of unity of order 2^" +
                        std::to_string(MAX_INTT_LOG + 1) + ", which the field does not have; cut the file with a power of " +
                        std::to_string(MAX_INTT_LOG - 1) + " or below");
    p.pw = loadPtauPowers(*f, p.hdr, opt->power);
    p.cut = p.pw.power != p.hdr.power;
    const u64 n = p.pw.n;
    const u64 cutBytes[4] = {(2 * n - 1) * 64, n * 128, n * 64, n * 64};
    u64 at = 12;
    for (const auto& s : f->inOrder()) {
        if (isLagrange(s.first)) continue;
        Section sec = s.second;
        if (p.cut && s.first >= 2 && s.first <= 5) sec.size = std::min(sec.size, cutBytes[s.first - 2]);
        p.kept.emplace_back(s.first, sec);
        at += 12 + sec.size;
    }
    p.records[0] = 4 * n - 1;
    p.records[1] = p.records[2] = p.records[3] = 2 * n - 1;
    for (int i = 0; i < 4; i++) {
        p.offset[i] = at + 12;
        at += 12 + p.records[i] * LAGRANGE_REC[i];
    }
    p.total = at;
}

// the container and every copied section; the header's power is the cut one
void writeKept(const Prepared& p, uint8_t* out) {
    uint8_t* o = out;
    putBytes(o, "ptau", 4); put32(o, 1); put32(o, (u32)p.kept.size() + 4);
    bool headerDone = false;
    for (const auto& s : p.kept) {
        put32(o, s.first); put64(o, s.second.size);
        const uint8_t* src = s.second.start;
        uint8_t* dst = o;
        constexpr u64 G = 1 << 24;
        parallelFor(s.second.size, G, [&](u64 lo, u64 hi) { memcpy(dst + lo, src + lo, hi - lo); });
        if (s.first == 1 && !headerDone && s.second.size >= 40) {
            const u32 power = p.pw.power;
            memcpy(dst + 36, &power, 4);
            headerDone = true;
        }
        o += s.second.size;
    }
    for (int i = 0; i < 4; i++) { put32(o, LAGRANGE_IDS[i]); put64(o, p.records[i] * LAGRANGE_REC[i]); o += p.records[i] * LAGRANGE_REC[i]; }
}

// the first record of `n` that differs, or n
u64 firstMismatch(const uint8_t* a, const uint8_t* b, u64 n, u64 rec) {
    if (!memcmp(a, b, n * rec)) return n;
    for (u64 i = 0; i < n; i++)
        if (memcmp(a + i * rec, b + i * rec, rec)) return i;
    return n;
}

u64 runPrepare(const ug_ptau_prepare_options* opt, const void* ptau, u64 ptauSize, int device, uint8_t* out, u64 outCap, double ms[PREP_PHASES],
               bool sizeOnly) {
    for (int i = 0; i < PREP_PHASES; i++) ms[i] = 0;
    PhaseClock clock(ms);
    std::unique_ptr<BinFile> f;
    Prepared p;
    plan(opt, ptau, ptauSize, f, p);
    const bool check = opt->mode == 1;
    PtauLagrange own;
    if (check) own = loadPtauLagrange(*f, p.hdr);
    if (sizeOnly) return check ? 0 : p.total;
    if (!check) {
        if (!out) throw SetupError("null output buffer");
        if (outCap < p.total) throw SetupError("the output buffer is too small: " + std::to_string(p.total) + " bytes are needed");
    }
    std::unique_ptr<Backend> owned;
    Backend& be = backendFor(device, owned);
    if (!check) writeKept(p, out);
    clock.lap(0);

    const u64 n = p.pw.n;
    {
        const PointCheck pointCheck(device, (int)opt->validate);
        pointCheck(false, p.pw.tau1, 2 * n - 1, 2, 0, 1);
        pointCheck(true, p.pw.tau2, n, 3, 0, 1);
        pointCheck(false, p.pw.alphaTau1, n, 4, 0, 1);
        pointCheck(false, p.pw.betaTau1, n, 5, 0, 1);
    }
    clock.lap(1);

    // where a level's records go: the output's sections, or (a check) a scratch level that is compared and dropped
    u64 bad[4] = {~0ull, ~0ull, ~0ull, ~0ull};   // the first mismatch of each section
    std::vector<uint8_t> scratch[4];
    auto target = [&](int sec, u64 first, u64 count) -> uint8_t* {
        if (!check) return out + p.offset[sec] + first * LAGRANGE_REC[sec];
        scratch[sec].resize(count * LAGRANGE_REC[sec]);
        return scratch[sec].data();
    };
    double compareMs = 0;                        // (the comparisons run between the levels; their time goes to the last phase)
    auto compare = [&](int sec, u64 first, u64 count) {
        if (!check || bad[sec] != ~0ull) return;
        const double t0 = nowMs();
        const u64 i = firstMismatch(scratch[sec].data(), own.sec[sec] + first * LAGRANGE_REC[sec], count, LAGRANGE_REC[sec]);
        if (i < count) bad[sec] = first + i;
        compareMs += nowMs() - t0;
    };
    auto lapLevels = [&](int phase) {
        clock.lap(phase);
        ms[phase] -= compareMs; ms[PREP_PHASES - 1] += compareMs;
        compareMs = 0;
    };
    auto refuse = [&](int sec) {
        if (bad[sec] != ~0ull)
            throw PtauError("section " + std::to_string(LAGRANGE_IDS[sec]) + " point " + std::to_string(bad[sec]) + ": does not match the powers");
    };
    double kms[2];
    for (u32 level = 0; level <= p.pw.power + 1; level++) {
        const u64 N = 1ull << level, first = N - 1;
        if (level <= p.pw.power) {
            const uint8_t* in[3] = {p.pw.tau1, p.pw.alphaTau1, p.pw.betaTau1};
            uint8_t* o[3] = {target(0, first, N), target(2, first, N), target(3, first, N)};
            be.intt(false, (int)level, 3, in, N, o, kms);
            compare(0, first, N); compare(2, first, N); compare(3, first, N);
        } else {                                 // the padded level: infinity in place of the power the ceremony does not have
            const uint8_t* in[1] = {p.pw.tau1};
            uint8_t* o[1] = {target(0, first, N)};
            be.intt(false, (int)level, 1, in, N - 1, o, kms);
            compare(0, first, N);
        }
    }
    lapLevels(2);
    refuse(0);
    for (u32 level = 0; level <= p.pw.power; level++) {
        const u64 N = 1ull << level, first = N - 1;
        const uint8_t* in[1] = {p.pw.tau2};
        uint8_t* o[1] = {target(1, first, N)};
        be.intt(true, (int)level, 1, in, N, o, kms);
        compare(1, first, N);
    }
    lapLevels(3);
    for (int sec = 1; sec < 4; sec++) refuse(sec);
    clock.lap(4);
    return check ? 0 : p.total;
}

}  // namespace
}  // namespace setup
}  // namespace ughost

// =====================================================================================================================
using namespace ughost::setup;

extern "C" {

int ug_ptau_prepare_size(const ug_ptau_prepare_options* opt, const void* ptau, uint64_t ptau_size, uint64_t* out_bytes, char* error_msg,
                         unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        double ms[PREP_PHASES];
        const u64 total = runPrepare(opt, ptau, ptau_size, -1, nullptr, 0, ms, true);
        if (out_bytes) *out_bytes = total;
    });
}

int ug_ptau_prepare_run(const ug_ptau_prepare_options* opt, const void* ptau, uint64_t ptau_size, int device, void* out, uint64_t out_capacity,
                        uint64_t* out_bytes, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        double ms[PREP_PHASES];
        const u64 total = runPrepare(opt, ptau, ptau_size, device, (uint8_t*)out, out_capacity, ms, false);
        if (out_bytes) *out_bytes = total;
        if (phase_ms) for (int i = 0; i < PREP_PHASES; i++) phase_ms[i] = ms[i];
    });
}

int ug_points_intt(int device, int g2, int log_n, const void* points, uint64_t n_given, void* out, double* kernel_ms, char* error_msg,
                   unsigned long long error_msg_maxsize) {
    return guarded(SETUP_RULE, error_msg, error_msg_maxsize, [&] {
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
        if (log_n < 0 || (u32)log_n > MAX_INTT_LOG) throw SetupError("log_n " + std::to_string(log_n) + " is not in 0 .. " + std::to_string(MAX_INTT_LOG));
        if (n_given > (1ull << log_n)) throw SetupError(std::to_string(n_given) + " points are more than 2^" + std::to_string(log_n));
        if (!out || (n_given && !points)) throw SetupError("null buffer");
        const uint8_t* in[1] = {(const uint8_t*)points};
        uint8_t* o[1] = {(uint8_t*)out};
        std::unique_ptr<Backend> owned;
        backendFor(device, owned).intt(g2 != 0, log_n, 1, in, n_given, o, kernel_ms);
    });
}

}  // extern "C"
