// ug_api.hip -- implementation of the inner C-ABI declared in include/ultragroth_hip.h.
// Owns device memory, the stream and the reusable workspaces; translates between the reference's byte
// formats and the device forms; catches every exception at the boundary.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <exception>
#include "dev_common.hpp"
#include "internal.hpp"
#include "host_util.hpp"
#include "../../include/ultragroth_hip.h"

using namespace ug;

namespace {
thread_local std::string g_last_error;
int fail(const std::string& msg) { g_last_error = msg; return UG_ERROR; }
#define UG_TRY try {
#define UG_CATCH                                                       \
    } catch (const std::exception& e) { return fail(e.what()); }       \
    catch (...) { return fail("unknown error"); }                      \
    return UG_OK;
}  // namespace

// Host -> HBM copies of large caller buffers (the witness of every proof: 512 MiB at 2^24; the zkey sections at create:
// 9.4 GB). The caller's memory is pageable (the reference's API hands over plain pointers, src/prover.h:127-138; a zkey
// file is an mmap, src/fileloader.cpp:23-51), and one hipMemcpy from pageable memory runs at about half the PCIe rate
// (measured 27 GB/s). Here LANES host threads each copy 8 MiB chunks into their own pinned buffers and queue the DMA on
// their own stream, DEPTH chunks deep, so page-touching memcpy and DMA overlap; `after` (optional) is queued behind each
// chunk's DMA on the same stream, e.g. the conversion kernel for that chunk's records. Blocking: returns when every
// chunk and every `after` has completed.
struct StagedUploader {
    static constexpr size_t CHUNK = (size_t)8 << 20;
    static constexpr int MAX_LANES = 8, DEPTH = 2;
    static constexpr size_t MIN_BYTES = (size_t)32 << 20;      // below this a plain copy is as fast
    struct Lane { hipStream_t stream = nullptr; PinnedBuf<uint8_t> buf[DEPTH]; Event done[DEPTH]; };
    Lane lanes[MAX_LANES];
    int n_lanes = 0;
    std::mutex turn;            // one upload at a time: the lanes' pinned buffers are the uploader's (a witness staged for the
                                // next proof from a second host thread meets the uploads of the running one here)
    typedef std::function<void(size_t offset, size_t bytes, hipStream_t stream)> After;
    void init() {
        if (n_lanes) return;
        int want = 4;
        if (const char* e = getenv("ULTRAGROTH_UPLOAD_THREADS")) want = atoi(e);
        want = want < 1 ? 1 : want > MAX_LANES ? MAX_LANES : want;
        // The lanes' streams are created with the LOWEST priority, i.e. from a pool of hardware queues of their own: the
        // runtime maps the streams of one priority onto a few hardware queues (four by default), and a copy whose stream
        // shares a queue with a stream that holds a whole proof's kernels waits for all of them. Measured at 2^24, a witness
        // staged beside a running proof: normal priority (two of the four lanes share the compute streams' queues) 146 ms,
        // i.e. the whole proof; highest priority 10 ms, but the proof beside it takes 6 ms longer (its dispatches yield to
        // the copies' packets); lowest priority 38 ms, the proof 2.5 ms longer -- the best of the three for the pair. With
        // the device idle all three copy at the same 53 GB/s.
        int least = 0, greatest = 0;
        UG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        for (int l = 0; l < want; l++) {
            const char* pe = getenv("UG_UPLOAD_PRIORITY");      // tuning knob: l(ow, default) | n(ormal) | h(igh)
            const int prio = (pe && pe[0] == 'h') ? greatest : (pe && pe[0] == 'n') ? 0 : least;
            UG_HIP(hipStreamCreateWithPriority(&lanes[l].stream, hipStreamNonBlocking, prio));
            for (int d = 0; d < DEPTH; d++) {
                lanes[l].buf[d].alloc(CHUNK);
                lanes[l].done[d] = Event(false);
            }
            n_lanes = l + 1;
        }
    }
    void upload(int device, void* dst, const void* src, size_t bytes, const After& after = After()) {
        std::lock_guard<std::mutex> one(turn);
        init();
        const size_t n_chunks = (bytes + CHUNK - 1) / CHUNK;
        std::exception_ptr errs[MAX_LANES];
        auto work = [&](int l) {
            try {
                UG_HIP(hipSetDevice(device));
                Lane& ln = lanes[l];
                size_t turn = 0;
                for (size_t c = (size_t)l; c < n_chunks; c += (size_t)n_lanes, turn++) {
                    const int d = (int)(turn % DEPTH);
                    if (turn >= DEPTH) UG_HIP(hipEventSynchronize(ln.done[d].e));      // the DMA out of this buffer has finished
                    const size_t off = c * CHUNK, len = bytes - off < CHUNK ? bytes - off : CHUNK;
                    memcpy(ln.buf[d].get(), static_cast<const uint8_t*>(src) + off, len);
                    UG_HIP(hipMemcpyAsync(static_cast<uint8_t*>(dst) + off, ln.buf[d].get(), len, hipMemcpyHostToDevice, ln.stream));
                    UG_HIP(hipEventRecord(ln.done[d].e, ln.stream));
                    if (after) after(off, len, ln.stream);
                }
                UG_HIP(hipStreamSynchronize(ln.stream));
            } catch (...) { errs[l] = std::current_exception(); }
        };
        std::vector<std::thread> th;
        for (int l = 1; l < n_lanes && (size_t)l < n_chunks; l++) th.emplace_back(work, l);
        work(0);
        for (auto& t : th) t.join();
        for (int l = 0; l < n_lanes; l++) if (errs[l]) std::rethrow_exception(errs[l]);
    }
    void release() {
        for (int l = 0; l < n_lanes; l++) {
            if (lanes[l].stream) hipStreamDestroy(lanes[l].stream);
            lanes[l] = Lane();                  // (its pinned buffers and events go here)
        }
        n_lanes = 0;
    }
};

struct ug_ctx {
    int device = 0;
    StagedUploader uploader;
    hipStream_t stream = nullptr;
    MsmWorkspace ws_g1, ws_g2;
    // Stream-time accounting without host waits (stream_timer.hpp): the timed sections are resolved the next time the stream is
    // known to be idle -- ug_ctx_collect, ug_ctx_timings, ug_ctx_sync. msm | fft: the split of ug_ctx_timings; kernel: the launches
    // of one kernel class -- [0] G1, [1] G2 bucket accumulation, [2] NTT passes, [3] G1 group accumulation (ug_ctx_kernel_stats)
    StreamTimer timer;
    TimeSink msm, fft, kernel[4];
    // Per-kernel statistics are OFF until somebody asks for them (ug_ctx_kernel_stats with reset != 0 switches them on for the
    // context): an event pair around a launch costs 10-25 us of idle device on this runtime (rocprofv3 trace of a 2^20 proof,
    // profiles/r05_variants_ab.txt item 1) -- 0.2 ms per proof that only a measuring caller should pay.
    bool kernel_stats_on = false;
    LaunchTimer stat(int k) { return LaunchTimer{&timer, kernel_stats_on ? &kernel[k] : nullptr}; }
    // the product queue: MSMs queued by ug_msm_*_enqueue whose results are still on their way (pinned_results block k <-> pending_msm[k])
    struct QueuedMsm { MsmPending pend; void* out; bool g2; };
    std::vector<QueuedMsm> pending_msm;
    Event order_event{false};              // ug_ctx_wait
    hipStream_t side_stream = nullptr;     // ug_msm_witness_enqueue: the G2 tail runs here beside the G1 tail
    Event side_fork, side_join;            // (created with the side stream)
    bool defer_tables = false;             // ug_ctx_defer_tables: sets are created with room for their window tables, which are
                                           // then built piece by piece (ug_bases_tables_step)
    int check_level = 0;                   // ug_ctx_check_points: the sets created on this context check their records (check.hip)
    DevBuf<unsigned long long> check_word;      // ... the fault word of the check in flight (device memory) and the stream it is
    hipStream_t check_stream = nullptr;         //     armed and read on: the context's own may hold the previous set's table build
    ug_point_fault last_fault = {0, UG_POINT_OK};   // what the last creation on this context found (ug_ctx_last_point_fault) ...
    int last_fault_member = -1;                      // ... and in which member of a group (-1: a plain set)
    ug_graph* recording = nullptr;         // the stream is being captured into this graph (ug_graph_begin .. ug_graph_end)
    std::vector<ug_graph*> launched;       // graphs launched on this stream whose event pairs are not accounted yet (resolve_timer)
    NttPlan raw_ntt;                       // cache for ug_fr_ntt
    DevBuf<u32> lookup_last; u64 lookup_last_n = 0;      // zeroed scratch of ug_dvec_apply_lookup
    DevBuf<u32> lookup_stage; size_t lookup_stage_bytes = 0;      // staging of the lookup calls (kept: two allocations and
                                                                  // two frees -- each a device-wide wait -- per proof otherwise)
    u32* stage_for_lookup(size_t bytes) {
        if (bytes > lookup_stage_bytes) {
            lookup_stage_bytes = 0;
            lookup_stage.alloc((bytes + 3) / 4);
            lookup_stage_bytes = bytes;
        }
        return lookup_stage.get();
    }
    PinnedBuf<u32> pinned_results;         // MSM_QUEUE_DEPTH result blocks of MSM_PENDING_WORDS words: the queued products' (pending_msm)
    std::vector<DevBuf<u32>> deferred_free;      // staging memory of queued set-up work: hipFree waits for the whole device, so it is
                                           // freed the next time the stream is idle anyway (ug_ctx_sync, destroy)
    void use() const { UG_HIP(hipSetDevice(device)); }
};
struct ug_bases {
    ug_ctx* ctx; bool g2; u64 n; u64 global_first; DevBuf<u32> pts = {};
    int table_c = 0;          // window width of the precomputed tables (0: none, pts holds the n points only)
    int table_stride = 1;     // ... and their stride: table j = 2^(stride c j) P (MsmGeometry::stride)
    int members = 1;          // > 1: a group -- n = slots * members records, record slot * members + m is member m's point of
    u64 slots = 0;            //      scalar global_first + slot (ug_bases_create_group_g1)
    bool empty = false;       // every record is the point at infinity (e.g. the B2 section of a circuit without B-side wires): its
                              // products are the point at infinity and no kernel is launched for them
    u64 tables_built = ~(u64)0;   // deferred build (ug_ctx_defer_tables): points [0, tables_built) have their tables; >= n: all of them
    int deferred_c = 0;           // ... the width the set will get: until ug_bases_tables_adopt the set holds its n points only
    int deferred_stride = 1;      // ... and the stride
    bool tables_usable() const { return !table_c || tables_built >= n; }
};
struct ug_dvec {
    ug_ctx* ctx; u64 n; DevBuf<u32> data; bool owns = true;      // owns == false (ug_dvec_wrap): data is the caller's memory
    ug_dvec(ug_ctx* c, u64 n_) : ctx(c), n(n_) {}
    ~ug_dvec() { if (!owns) (void)data.take(); }
};
struct ug_index {
    ug_ctx* ctx; u64 n; DevBuf<u32> data = {};
};
struct ug_schedule {
    ug_ctx* ctx; MsmSchedule sched; u64 first = 0;
    BucketClasses cls;                    // ug_schedule_set_classes: applied by every later build
    u64 sp_first = 0, sp_end = 0;         // ... its special-bucket scalar range, in the scalar vector's (global) indices
    // the classes as the build of scalars [first, first + count) sees them (the scalar range clipped and made local)
    BucketClasses classes_for(u64 first_, u64 count) const {
        BucketClasses k = cls;
        if (!k.on()) return k;
        const u64 lo = sp_first > first_ ? sp_first - first_ : 0, hi = sp_end > first_ ? sp_end - first_ : 0;
        k.sp_lo = (u32)(lo < count ? lo : count); k.sp_hi = (u32)(hi < count ? hi : count);
        return k;
    }
};
struct ug_hpoly {
    ug_ctx* ctx; CoefMatrix mat; NttPlan ntt; u32 domain = 0, nvars = 0;
    DevBuf<u32> a, b, c, t, t2;                                                    // group * domain elements each: vector g of a launch
                                                                                   // group works on [g * domain, (g + 1) * domain)
    int group = 1;            // vectors side by side that the workspaces hold (ug_hpoly_reserve_vectors)
    int last_group = 0;       // largest launch group of the last ug_hpoly_run_vectors call (0: none yet)
};

// The three matrices of an .r1cs on the device (r1cs.hip) and the result words of the checks queued on it: slot k (one per witness
// of a batched pass, the last one ug_r1cs_check's own) has two device words -- failing constraints, ~(lowest failing index) --
// whose copy in pinned memory is complete once the slot's event has passed.
struct ug_r1cs {
    static constexpr int SLOTS = UG_BATCH_MAX + 1;
    ug_ctx* ctx = nullptr;
    ughost::R1csHeader hdr;
    u64 terms[3] = {0, 0, 0};
    DevBuf<u32> row_ptr[3], sig[3], val[3];
    DevBuf<unsigned long long> words;           // device: 2 per slot, then the word of the probe (ug_r1cs_match_hpoly)
    PinnedBuf<unsigned long long> words_host;   // pinned: the same
    DevBuf<u32> row_values;                     // device: A.w, B.w, C.w of one constraint (24 words) ...
    PinnedBuf<u32> row_values_host;             // ... and pinned
    Event done[SLOTS];
    Event t0, t1;
    struct Queued { const u32* wtns = nullptr; hipStream_t stream = nullptr; bool on = false; } queued[SLOTS];
    R1csDev dev() const {
        R1csDev d;
        d.rows = hdr.nConstraints;
        for (int t = 0; t < 3; t++) { d.row_ptr[t] = row_ptr[t].get(); d.sig[t] = sig[t].get(); d.val[t] = val[t].get(); }
        return d;
    }
};

// A fixed launch sequence of one or two contexts of a device, captured once and replayed (ug_graph_*). It owns the event pairs
// that were recorded inside it -- the timed spans of the contexts' MSM | FFT accumulators and the per-kernel statistics -- and a
// copy of the products that were queued while it was captured (their result blocks arrive in the same pinned memory every time).
struct ug_graph {
    ug_ctx* c[2] = {nullptr, nullptr};
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<ug_ctx::QueuedMsm> pend[2];
    std::vector<StreamTimer::Pair> pairs[2];   // recorded through context q's timer; each pair knows its sink
    uint64_t epoch = 0;                        // alloc_epoch() when the capture ended
    size_t nodes = 0;
    bool capturing = false;
};

namespace {
// blocking copy of a caller buffer into device memory; `after` as in StagedUploader::upload (called once for a small copy)
// fresh: dst was allocated just now, nothing queued on the device refers to it -- the copy then neither waits for the
// context's stream nor uses it (a window-table build of the previous section may be running there: the upload of the next
// section overlaps it)
void host_to_device(ug_ctx* c, void* dst, const void* src, size_t bytes, const StagedUploader::After& after = StagedUploader::After(),
                    bool fresh = false) {
    if (!bytes) return;
    if (fresh) { c->uploader.upload(c->device, dst, src, bytes, after); return; }
    UG_HIP(hipStreamSynchronize(c->stream));                   // nothing queued earlier may still read or write dst
    if (bytes >= StagedUploader::MIN_BYTES) { c->uploader.upload(c->device, dst, src, bytes, after); return; }
    UG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    if (after) after(0, bytes, c->stream);
    UG_HIP(hipStreamSynchronize(c->stream));
}
// ---- point validation (check.hip): the fault word of a context ----
// a creation found a bad point: remembered on the context (the outer layer asks for it instead of reading the message), then thrown
[[noreturn]] void throw_point_fault(ug_ctx* c, int member, const ug_point_fault& f) {
    c->last_fault = f; c->last_fault_member = member;
    throw std::runtime_error((member >= 0 ? "member " + std::to_string(member) + " point " : std::string("point ")) + std::to_string(f.index) + ": " +
                             ug_point_reason_text(f.reason));
}
// all ones = clean; returns when the word is set (the upload lanes' kernels that follow run on other streams)
void check_arm(ug_ctx* c) {
    if (!c->check_stream) UG_HIP(hipStreamCreateWithFlags(&c->check_stream, hipStreamNonBlocking));
    if (!c->check_word.get()) c->check_word.alloc(1);
    UG_HIP(hipMemsetAsync(c->check_word.get(), 0xff, 8, c->check_stream));
    UG_HIP(hipStreamSynchronize(c->check_stream));
}
// after every kernel that may have written the word has completed
ug_point_fault check_read(ug_ctx* c) {
    unsigned long long w = 0;
    UG_HIP(hipMemcpyAsync(&w, c->check_word.get(), 8, hipMemcpyDeviceToHost, c->check_stream));
    UG_HIP(hipStreamSynchronize(c->check_stream));
    ug_point_fault f;
    f.index = w == ~0ull ? 0 : (uint64_t)(w >> 2);
    f.reason = w == ~0ull ? UG_POINT_OK : (int)(w & 3);
    return f;
}
void check_release(ug_ctx* c) {
    c->check_word.release();
    if (c->check_stream) hipStreamDestroy(c->check_stream);
    c->check_stream = nullptr;
}
// Test hook (ug_test_inject_fault): the `after`-th next pass through fault point `site` throws. Only in processes started
// with ULTRAGROTH_TEST_HOOKS=1 (the same gate as the blinding hook); otherwise fault_point() is one relaxed load.
std::atomic<int> g_fault_site{0}, g_fault_after{0};
bool test_hooks_on() {
    static const bool on = [] { const char* e = getenv("ULTRAGROTH_TEST_HOOKS"); return e && e[0] == '1' && !e[1]; }();
    return on;
}
void fault_point(int site) {
    if (g_fault_site.load(std::memory_order_relaxed) != site) return;
    if (g_fault_after.fetch_sub(1) != 1) return;
    g_fault_site.store(0);
    throw std::runtime_error("injected fault (test hook) at site " + std::to_string(site));
}
// ULTRAGROTH_TRACE=1: where the host time of the set-up calls goes (stderr, ms of a process-wide clock)
void trace_step(const char* what) {
    static const bool on = getenv("ULTRAGROTH_TRACE") && atoi(getenv("ULTRAGROTH_TRACE")) != 0;
    if (!on) return;
    static const auto origin = std::chrono::steady_clock::now();
    fprintf(stderr, "[ug_api] %9.3f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - origin).count(), what);
}
// after the stream has been synchronised: account the finished sections
void resolve_timer(ug_ctx* c) {
    c->timer.resolve();
    // graphs launched on this stream have completed as well: one launch of each is accounted (their event pairs are re-recorded
    // by every launch, so a graph is resolved before it is launched again: ug_graph_launch sees to that)
    for (ug_graph* g : c->launched) for (int q = 0; q < 2; q++) StreamTimer::account(g->pairs[q]);
    c->launched.clear();
}
void sync_and_resolve(ug_ctx* c) {
    UG_HIP(hipStreamSynchronize(c->stream));
    resolve_timer(c);
    c->deferred_free.clear();
}
// The product queue of a context: ug_ctx::pending_msm, slot k of which owns block k of ug_ctx::pinned_results. An enqueue call
// takes its slots at the end of the queue through this object, which gives them back unless commit() is reached: nothing of a
// failed call stays queued.
struct QueueSlots {
    ug_ctx* c; const size_t first; bool committed = false;
    QueueSlots(ug_ctx* c_, int n) : c(c_), first(c_->pending_msm.size()) {            // (takes nothing yet: add)
        if (n < 0 || first + (size_t)n > (size_t)MSM_QUEUE_DEPTH)
            throw std::invalid_argument("at most " + std::to_string(MSM_QUEUE_DEPTH) + " products may be queued before ug_ctx_collect");
    }
    QueueSlots(const QueueSlots&) = delete;
    QueueSlots& operator=(const QueueSlots&) = delete;
    ~QueueSlots() { if (!committed) c->pending_msm.resize(first); }
    // the next slot, for a product whose records go to `out`: its pinned result block
    u32* add(void* out, bool g2) {
        c->pending_msm.push_back(ug_ctx::QueuedMsm{MsmPending(), out, g2});
        return c->pinned_results.get() + (c->pending_msm.size() - 1) * MSM_PENDING_WORDS;
    }
    // pend[k]: what msm_enqueue said about the k-th slot added
    void commit(const MsmPending* pend) {
        for (size_t k = first; k < c->pending_msm.size(); k++) c->pending_msm[k].pend = pend[k - first];
        committed = true;
    }
};
// MsmCall::Product::delta: the schedule's scalar i multiplies record i + delta of the set
int64_t schedule_delta(const ug_schedule* s, const ug_bases* b, int64_t index_shift = 0) { return (int64_t)s->first - index_shift - (int64_t)b->global_first; }
// the call of a base group's K products, results in the next K slots of the queue
MsmCall group_call(QueueSlots& slots, const ug_bases* group, const ug_schedule* s, void* const* outs) {
    MsmCall call;
    call.count = call.group = group->members;
    call.products[0] = {group->pts.get(), group->slots, schedule_delta(s, group), nullptr};
    for (int m = 0; m < call.count; m++) call.products[m].host = slots.add(outs[m], false);
    return call;
}
template <class F> void store_mont256(uint8_t* out, const F& v);
template <> void store_mont256<Fq>(uint8_t* out, const Fq& v) { u32 w[8]; to_mont256(w, v); memcpy(out, w, 32); }
}  // namespace

extern "C" {

const char* ug_last_error(void) { return g_last_error.c_str(); }

int ug_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int ug_ctx_create(ug_ctx** out, int device) { return ug_ctx_create_priority(out, device, 0); }
int ug_ctx_create_priority(ug_ctx** out, int device, int priority_class) {
    UG_TRY
    if (!out) throw std::invalid_argument("null ctx pointer");
    int n = 0;
    UG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::invalid_argument("no such HIP device: " + std::to_string(device));
    UG_HIP(hipSetDevice(device));               // (the context's events are created with it)
    std::unique_ptr<ug_ctx, void (*)(ug_ctx*)> hold(new ug_ctx(), ug_ctx_destroy);
    ug_ctx* c = hold.get();
    c->device = device;
    if (priority_class) {
        int least = 0, greatest = 0;                // (numerically: greatest priority = lowest number)
        UG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        UG_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, priority_class > 0 ? greatest : least));
    } else {
        UG_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    }
    c->pinned_results.alloc((size_t)MSM_QUEUE_DEPTH * MSM_PENDING_WORDS);
    *out = hold.release();
    UG_CATCH
}
void ug_ctx_destroy(ug_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->uploader.release();
    check_release(c);
    if (c->side_stream) { hipStreamSynchronize(c->side_stream); hipStreamDestroy(c->side_stream); }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                                   // (with its device and pinned memory -- the workspaces move the epoch -- and its events)
}
int ug_ctx_sync(ug_ctx* c) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->use();
    sync_and_resolve(c);
    UG_CATCH
}
// everything queued on `waiter` after this call starts only when everything queued on `signal` before it has finished
// (device-side ordering, no host wait)
int ug_ctx_wait(ug_ctx* waiter, ug_ctx* signal) {
    UG_TRY
    if (!waiter || !signal) throw std::invalid_argument("null argument");
    if (waiter->device != signal->device) throw std::invalid_argument("contexts on different devices");
    waiter->use();
    UG_HIP(hipEventRecord(signal->order_event.e, signal->stream));
    UG_HIP(hipStreamWaitEvent(waiter->stream, signal->order_event.e, 0));
    UG_CATCH
}

// table_c != 0: the set is created WITH its fixed-base window tables -- room for all of them is allocated at once, the points
// go straight into table 0, and the table kernel is queued on the context's stream without a host wait, so that the upload
// of the caller's next section (staged through the uploader's own streams) runs beside it. Everything queued on the
// context later is ordered behind the tables; ug_ctx_sync ends the build.
static bool host_all_zero(const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    size_t i = 0;
    for (; i < bytes && ((uintptr_t)(b + i) & 7); i++) if (b[i]) return false;
    for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); if (w) return false; }
    for (; i < bytes; i++) if (b[i]) return false;
    return true;
}
static int bases_create(ug_ctx* c, const void* host, u64 n, u64 global_first, bool g2, int table_c, int stride, ug_bases** out) {
    UG_TRY
    if (!c || !out || (!host && n)) throw std::invalid_argument("null argument");
    c->use();
    c->last_fault = {0, UG_POINT_OK}; c->last_fault_member = -1;
    int windows = 1;                                          // (the number of tables: ceil(W / stride))
    if (table_c) {
        windows = MsmGeometry::table_count(table_c, MsmGeometry::choose_tables(n, table_c, stride).stride);      // validates width and stride
        if (n > ((u64)1 << TABLE_INDEX_BITS)) throw std::invalid_argument("window tables need at most 2^27 points per set");
    }
    std::unique_ptr<ug_bases> hold(new ug_bases{c, g2, n, global_first});
    ug_bases* b = hold.get();
    const size_t rec = g2 ? 128 : 64, bytes = (size_t)n * rec;
    b->empty = n != 0 && host_all_zero(host, bytes);          // (stops at the first point that is not infinity: the first record, normally)
    const bool defer = table_c && c->defer_tables;            // the room for the tables comes later too (ug_bases_tables_alloc / _adopt):
    if (defer) windows = 1;                                   // a first allocation of tens of GiB can take a second by itself
    if (!b->pts.try_alloc(bytes / 4 * (size_t)windows))
        throw std::runtime_error(table_c ? "not enough device memory for the window tables" : "not enough device memory for the base points");
    if (n) {
        // each chunk's records are converted to the device form behind its own DMA (chunks are whole records: 8 MiB / 128)
        u32* pts = b->pts.get();
        const int level = c->check_level;                  // (0: exactly the path without the check)
        unsigned long long* word = nullptr;
        if (level) { check_arm(c); word = c->check_word.get(); }
        host_to_device(c, pts, host, bytes, [pts, rec, g2, level, word, global_first](size_t off, size_t len, hipStream_t st) {
            u32* p = pts + off / 4;
            if (level) check_points(g2, p, len / rec, global_first + off / rec, level, word, st);      // the raw records, before they are reduced
            if (g2) convert_points_g2(p, len / rec, st); else convert_points_g1(p, len / rec, st);
        }, /*fresh*/ true);
        if (level) {                                       // (the upload has waited for every chunk: one read, and no table build for a bad set)
            const ug_point_fault f = check_read(c);
            if (f.reason != UG_POINT_OK) throw_point_fault(c, -1, f);
        }
        if (table_c && !defer) build_window_tables(g2, pts, n, table_c * stride, windows, c->stream);
    }
    if (defer) { b->deferred_c = table_c; b->deferred_stride = stride; } else if (table_c) { b->table_c = table_c; b->table_stride = stride; }
    *out = hold.release();
    UG_CATCH
}
int ug_bases_create_g1(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, ug_bases** out) { return bases_create(c, host, n, gf, false, 0, 1, out); }
int ug_bases_create_g2(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, ug_bases** out) { return bases_create(c, host, n, gf, true, 0, 1, out); }
int ug_bases_create_tables_g1(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, int table_c, ug_bases** out) { return bases_create(c, host, n, gf, false, table_c, 1, out); }
int ug_bases_create_tables_g2(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, int table_c, ug_bases** out) { return bases_create(c, host, n, gf, true, table_c, 1, out); }
int ug_bases_create_tables_strided_g1(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, int table_c, int stride, ug_bases** out) {
    return bases_create(c, host, n, gf, false, table_c, stride, out);
}
int ug_bases_create_tables_strided_g2(ug_ctx* c, const void* host, uint64_t n, uint64_t gf, int table_c, int stride, ug_bases** out) {
    return bases_create(c, host, n, gf, true, table_c, stride, out);
}
// The n_records host records go up and are converted as one plain set; the records first, first + step, ... are then copied side
// by side on the device into the set that is returned, and the upload is freed.
int ug_bases_create_every_g1(ug_ctx* c, const void* host, uint64_t n_records, uint64_t first, uint64_t step, uint64_t gf, ug_bases** out) {
    if (!c || !out || !host || !step || first >= n_records) return fail("ug_bases_create_every_g1: null argument, step 0 or no record to take");
    ug_bases* all = nullptr;
    if (bases_create(c, host, n_records, 0, false, 0, 1, &all) != UG_OK) return UG_ERROR;
    std::unique_ptr<ug_bases, void (*)(ug_bases*)> hold(all, ug_bases_destroy);
    UG_TRY
    const u64 count = (n_records - first + step - 1) / step;
    std::unique_ptr<ug_bases> b(new ug_bases{c, false, count, gf});
    b->empty = true;
    for (u64 i = 0; i < count && b->empty; i++) b->empty = host_all_zero(static_cast<const unsigned char*>(host) + (first + i * step) * 64, 64);
    if (!b->pts.try_alloc((size_t)count * 16)) throw std::runtime_error("not enough device memory for the base points");
    points_take_every(b->pts.get(), all->pts.get(), first, step, count, c->stream);
    UG_HIP(hipStreamSynchronize(c->stream));
    *out = b.release();
    UG_CATCH
}

// A group of `members` (2 or 3) G1 sets that are always multiplied by the same scalars, as ONE array of members-point
// records (msm.hip: segment_accumulate_group_kernel). Member m brings n[m] points; its first point belongs to the scalar
// with global index first[m]. The group covers the scalars [group_first, group_first + slots); slots a member has no point
// for hold infinity. With table_c the window tables are built over the interleaved array (a plain G1 array of slots * members
// points as far as the table kernel is concerned), queued on the context's stream as for ug_bases_create_tables_g1.
int ug_bases_create_group_strided_g1(ug_ctx* c, int members, const void* const* host, const uint64_t* n, const uint64_t* first,
                                     uint64_t group_first, uint64_t slots, int table_c, int stride, ug_bases** out) {
    UG_TRY
    if (!c || !out || !host || !n || !first) throw std::invalid_argument("null argument");
    c->last_fault = {0, UG_POINT_OK}; c->last_fault_member = -1;
    if (members < 2 || members > 3) throw std::invalid_argument("a base group has 2 or 3 members");
    for (int m = 0; m < members; m++) {
        if (!host[m] && n[m]) throw std::invalid_argument("null argument");
        if (n[m] && (first[m] < group_first || first[m] + n[m] > group_first + slots)) throw std::invalid_argument("group member outside the group's scalar range");
    }
    c->use();
    int windows = 1;
    if (table_c) windows = MsmGeometry::table_count(table_c, MsmGeometry::choose_tables(slots, table_c, stride).stride);      // validates width and stride
    if (slots > ((u64)1 << TABLE_INDEX_BITS)) throw std::invalid_argument("a base group holds at most 2^27 scalars");
    std::unique_ptr<ug_bases> hold(new ug_bases{c, false, slots * (u64)members, group_first});
    ug_bases* b = hold.get();
    b->members = members; b->slots = slots;
    const bool defer = table_c && c->defer_tables;            // (as bases_create)
    if (defer) windows = 1;
    const size_t bytes = (size_t)b->n * 64;
    u64 most = 0;
    for (int m = 0; m < members; m++) most = n[m] > most ? n[m] : most;
    DevBuf<u32> stage_own;
    trace_step("group: allocating");
    if (!b->pts.try_alloc(bytes / 4 * (size_t)windows) || !stage_own.try_alloc((size_t)most * 16))
        throw std::runtime_error(table_c ? "not enough device memory for the window tables" : "not enough device memory for the base points");
    u32* const stage = stage_own.get();
    trace_step("group: allocated");
    if (bytes) {
        UG_HIP(hipMemsetAsync(b->pts.get(), 0, bytes, c->stream));            // slots without a point: infinity
        UG_HIP(hipStreamSynchronize(c->stream));
    }
    trace_step("group: table 0 cleared");
    u32* pts = b->pts.get();
    const int level = c->check_level;
    for (int m = 0; m < members; m++) {
        trace_step("group: member upload");
        // chunks of whole records: converted to the device form and moved to their slots behind their own DMA
        if (!n[m]) continue;
        const u64 slot0 = first[m] - group_first, first_m = first[m];
        unsigned long long* word = nullptr;
        if (level) { check_arm(c); word = c->check_word.get(); }
        host_to_device(c, stage, host[m], (size_t)n[m] * 64, [=](size_t off, size_t len, hipStream_t st) {
            if (level) check_points(false, stage + off / 4, len / 64, first_m + off / 64, level, word, st);
            convert_points_g1(stage + off / 4, len / 64, st);
            interleave_points_g1(pts, stage + off / 4, len / 64, members, m, slot0 + off / 64, st);
        }, /*fresh*/ true);
        if (level) {                                       // per member (its upload has waited for every chunk), so that the member can be named
            const ug_point_fault f = check_read(c);
            if (f.reason != UG_POINT_OK) throw_point_fault(c, m, f);
        }
    }
    if (table_c && b->n && !defer) build_window_tables(false, pts, b->n, table_c * stride, windows, c->stream);
    c->deferred_free.push_back(std::move(stage_own));      // (not freed here: that would wait for the table build just queued, and the
                                                           // caller's next section could no longer be uploaded beside it)
    if (defer) { b->deferred_c = table_c; b->deferred_stride = stride; } else if (table_c) { b->table_c = table_c; b->table_stride = stride; }
    *out = hold.release();
    UG_CATCH
}
int ug_bases_create_group_g1(ug_ctx* c, int members, const void* const* host, const uint64_t* n, const uint64_t* first,
                             uint64_t group_first, uint64_t slots, int table_c, ug_bases** out) {
    return ug_bases_create_group_strided_g1(c, members, host, n, first, group_first, slots, table_c, 1, out);
}
int ug_bases_members(const ug_bases* b) { return b ? b->members : 0; }

// POINT VALIDATION (check.hip). The records go through a bounded device buffer, piece by piece, each piece staged as an upload is
// (the check kernel of a chunk queued behind its DMA); the fault word is read once, after the last piece.
int ug_points_check(ug_ctx* c, int g2, const void* host_points, uint64_t n, int level, ug_point_fault* out) {
    UG_TRY
    if (!c || !out || (!host_points && n)) throw std::invalid_argument("null argument");
    if (level != 1 && level != 2) throw std::invalid_argument("check level must be 1 or 2");
    c->use();
    out->index = 0; out->reason = UG_POINT_OK;
    if (!n) return UG_OK;
    const size_t rec = g2 ? 128 : 64;
    const u64 piece = ((u64)64 << 20) / rec;                   // 64 MiB of records at a time
    // nothing stays resident: the fault word goes when the call ends, however it ends, unless it is the context's (check_level)
    struct WordScope { ug_ctx* c; ~WordScope() { if (!c->check_level) check_release(c); } } word_scope{c};
    DevBuf<u32> buf_own;
    if (!buf_own.try_alloc((size_t)(n < piece ? n : piece) * (rec / 4))) throw std::runtime_error("not enough device memory for the point check");
    u32* const buf = buf_own.get();
    check_arm(c);
    unsigned long long* word = c->check_word.get();
    const bool is_g2 = g2 != 0;
    for (u64 done = 0; done < n; done += piece) {
        const u64 m = n - done < piece ? n - done : piece;
        host_to_device(c, buf, static_cast<const uint8_t*>(host_points) + done * rec, (size_t)m * rec,
                       [=](size_t off, size_t len, hipStream_t st) { check_points(is_g2, buf + off / 4, len / rec, done + off / rec, level, word, st); },
                       /*fresh*/ true);      // (buf is this call's own, and every upload returns with its kernels done)
    }
    *out = check_read(c);
    UG_CATCH
}
// The mask form: the same pieces, the status bytes of each piece downloaded behind it.
int ug_points_check_mask(ug_ctx* c, int g2, const void* host_points, uint64_t n, int level, uint8_t* reasons) {
    UG_TRY
    if (!c || (n && (!host_points || !reasons))) throw std::invalid_argument("null argument");
    if (level != 1 && level != 2) throw std::invalid_argument("check level must be 1 or 2");
    c->use();
    if (!n) return UG_OK;
    const size_t rec = g2 ? 128 : 64;
    const u64 piece = ((u64)64 << 20) / rec;                   // 64 MiB of records at a time
    const u64 room = n < piece ? n : piece;
    DevBuf<u32> buf_own;
    DevBuf<uint8_t> status_own;
    if (!buf_own.try_alloc((size_t)room * (rec / 4)) || !status_own.try_alloc((size_t)room)) throw std::runtime_error("not enough device memory for the point check");
    u32* const buf = buf_own.get();
    uint8_t* const status = status_own.get();
    const bool is_g2 = g2 != 0;
    for (u64 done = 0; done < n; done += piece) {
        const u64 m = n - done < piece ? n - done : piece;
        host_to_device(c, buf, static_cast<const uint8_t*>(host_points) + done * rec, (size_t)m * rec,
                       [=](size_t off, size_t len, hipStream_t st) { check_points_mask(is_g2, buf + off / 4, len / rec, level, status + off / rec, st); },
                       /*fresh*/ true);      // (every upload returns with its kernels done)
        UG_HIP(hipMemcpy(reasons + done, status, (size_t)m, hipMemcpyDeviceToHost));
    }
    UG_CATCH
}
const char* ug_point_reason_text(int reason) {
    return reason == UG_POINT_UNREDUCED ? "coordinate not below the field modulus"
         : reason == UG_POINT_OFF_CURVE ? "not on the curve"
         : reason == UG_POINT_OFF_SUBGROUP ? "not in the subgroup of order r" : "";
}
int ug_ctx_last_point_fault(const ug_ctx* c, int* member, ug_point_fault* out) {
    if (!c || !out) return fail("null argument");
    *out = c->last_fault;
    if (member) *member = c->last_fault_member;
    return UG_OK;
}
int ug_ctx_check_points(ug_ctx* c, int level) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    if (level < 0 || level > 2) throw std::invalid_argument("check level must be 0, 1 or 2");
    c->use();
    c->check_level = level;
    if (level) check_arm(c); else check_release(c);            // (the word is the context's from here on: a failing creation leaves no trace)
    UG_CATCH
}
int ug_points_all_infinity(const void* host_points, uint64_t n, uint64_t record_bytes) {
    return (host_points && n) ? (host_all_zero(host_points, (size_t)n * (size_t)record_bytes) ? 1 : 0) : 0;
}
int ug_msm_table_window(uint64_t n) { return MsmGeometry::table_window(n); }
uint64_t ug_bases_tables_bytes(uint64_t n, int g2, int c) { return ug_bases_tables_bytes_strided(n, g2, c, 1); }
uint64_t ug_bases_tables_bytes_strided(uint64_t n, int g2, int c, int stride) {
    if (c < TABLE_MIN_C || c > TABLE_MAX_C || stride < 1 || stride > (255 + c - 1) / c) return 0;
    return (uint64_t)(MsmGeometry::table_count(c, stride) - 1) * n * (g2 ? 128 : 64);
}
// WINDOW-TABLE PLAN under a memory budget (host only). Everything fits: every qualifying group gets the cost-model width at stride
// 1 (what the provers chose before there was a plan). Otherwise each group gets none or one (c, stride), the choice that minimises
// the summed modelled cost within the budget: an exact multiple-choice knapsack over the groups' Pareto fronts (bytes against
// cost), deterministic for equal inputs.
namespace {
constexpr u64 PLAN_MIN_SCALARS = (u64)1 << 14, PLAN_MAX_SCALARS = (u64)1 << 26;
constexpr u64 PLAN_MAX_ENTRIES = (u64)1 << 30;          // scalars * windows of one schedule
constexpr u64 PLAN_MAX_BUCKETS = (u64)1 << 24;          // stride * 2^(c-1): a strided schedule's buckets per product stay within
                                                        // twice those of the widest full set (the caller reserves their memory)
constexpr double PLAN_G2_WEIGHT = 3.0;                  // a G2 addition against a G1 one: Fq2 products cost three Fq products
struct PlanOption { u64 bytes; double cost; int c, stride; };
bool plan_qualifies(const ug_table_group& g) { return g.scalars >= PLAN_MIN_SCALARS && g.scalars <= PLAN_MAX_SCALARS; }
u64 plan_bytes(const ug_table_group& g, int c, int stride) {
    return ug_bases_tables_bytes_strided(g.g1_points, 0, c, stride) + ug_bases_tables_bytes_strided(g.g2_points, 1, c, stride);
}
// modelled cost of a group's products: per product the MSM cost, G2 products weighted
double plan_cost(const ug_table_group& g, int c, int stride) {
    if (!g.scalars) return 0;
    const double products = ((double)g.g1_points + PLAN_G2_WEIGHT * (double)g.g2_points) / (double)g.scalars;
    return products * (c ? msm_model_cost(g.scalars, c, true, stride) : msm_model_cost(g.scalars, MsmGeometry::choose(g.scalars).c, false));
}
// options sorted by bytes, each strictly cheaper than every option before it
void pareto(std::vector<PlanOption>& v) {
    std::stable_sort(v.begin(), v.end(), [](const PlanOption& a, const PlanOption& b) { return a.bytes != b.bytes ? a.bytes < b.bytes : a.cost < b.cost; });
    std::vector<PlanOption> keep;
    for (const PlanOption& o : v) if (keep.empty() || o.cost < keep.back().cost) keep.push_back(o);
    v.swap(keep);
}
}  // namespace
int ug_plan_window_tables(const ug_table_group* groups, int n_groups, uint64_t budget, ug_table_choice* out) {
    UG_TRY
    if (n_groups < 0 || (n_groups && (!groups || !out))) throw std::invalid_argument("null argument");
    u64 full = 0;
    for (int k = 0; k < n_groups; k++) {
        out[k] = ug_table_choice{0, 0, 0};
        if (!plan_qualifies(groups[k])) continue;
        const int c = MsmGeometry::table_window(groups[k].scalars);
        out[k] = ug_table_choice{c, 1, plan_bytes(groups[k], c, 1)};
        full += out[k].bytes;
    }
    if (full <= budget) return UG_OK;
    // a state of the knapsack: bytes, cost and the option taken in every group so far
    struct State { u64 bytes; double cost; std::vector<int> pick; };
    std::vector<State> front{State{0, 0.0, {}}};
    std::vector<std::vector<PlanOption>> opts(n_groups);
    for (int k = 0; k < n_groups; k++) {
        const ug_table_group& g = groups[k];
        std::vector<PlanOption>& o = opts[k];
        o.push_back(PlanOption{0, plan_cost(g, 0, 0), 0, 0});
        if (plan_qualifies(g) && (g.g1_points || g.g2_points)) {
            for (int c = TABLE_MIN_C; c <= TABLE_MAX_C; c++) {
                const int windows = (255 + c - 1) / c;
                if (g.scalars * (u64)windows > PLAN_MAX_ENTRIES) continue;
                for (int st = 1; MsmGeometry::table_count(c, st) > 1; st++) {      // (one table would be the classic windows)
                    const u64 bytes = plan_bytes(g, c, st);
                    if (bytes > budget || (u64)st << (c - 1) > PLAN_MAX_BUCKETS) continue;
                    o.push_back(PlanOption{bytes, plan_cost(g, c, st), c, st});
                }
            }
        }
        pareto(o);
        std::vector<State> next;
        for (const State& st : front)
            for (size_t j = 0; j < o.size(); j++) {
                if (st.bytes + o[j].bytes > budget) break;               // (o is sorted by bytes)
                State n = st;
                n.bytes += o[j].bytes; n.cost += o[j].cost; n.pick.push_back((int)j);
                next.push_back(std::move(n));
            }
        std::stable_sort(next.begin(), next.end(), [](const State& a, const State& b) { return a.bytes != b.bytes ? a.bytes < b.bytes : a.cost < b.cost; });
        front.clear();
        for (State& st : next) if (front.empty() || st.cost < front.back().cost) front.push_back(std::move(st));
    }
    // the front is sorted by bytes with falling cost: its last state is the cheapest within the budget
    const State& best = front.back();
    for (int k = 0; k < n_groups; k++) {
        const PlanOption& o = opts[k][best.pick[k]];
        out[k] = ug_table_choice{o.c, o.stride, o.bytes};
    }
    UG_CATCH
}
// Witnesses per device pass of a batched proof (include/ultragroth_hip.h): the largest V <= min(requested, 16) for which every
// schedule group's V-vector schedule keeps its limits and the V-fold buffers fit the free bytes
namespace {
constexpr u64 BATCH_PAIR_BYTES = 64;      // per (scalar, window) pair: four sort arrays (16) + accumulation slots of 3 G1 and 1 G2 products
constexpr u64 BATCH_BUCKET_BYTES = 732;   // per bucket: start, count, list (12) + points of 3 G1 (3 x 144) and 1 G2 (288) products
u64 batch_bytes(const ug_batch_schedule* s, int n, uint64_t n_vars, uint64_t domain, int v) {
    u64 bytes = (u64)v * (n_vars + domain) * 32;                                  // witness and h vectors
    for (int k = 0; k < n; k++) {
        if (!s[k].scalars) continue;
        const MsmGeometry g = s[k].c ? MsmGeometry::choose_tables(s[k].scalars, s[k].c, s[k].stride) : MsmGeometry::choose(s[k].scalars);
        bytes += (u64)v * (g.n * (u64)g.windows * BATCH_PAIR_BYTES + (u64)g.window_sets() * g.buckets * BATCH_BUCKET_BYTES);
    }
    return bytes;
}
bool batch_fits(const ug_batch_schedule* s, int n, int v) {
    for (int k = 0; k < n; k++) {
        if (!s[k].scalars) continue;
        const MsmGeometry g = s[k].c ? MsmGeometry::choose_tables(s[k].scalars, s[k].c, s[k].stride) : MsmGeometry::choose(s[k].scalars);
        if (g.n > ((u64)1 << TABLE_INDEX_BITS)) return false;
        if ((u64)v * g.n * (u64)g.windows > PLAN_MAX_ENTRIES) return false;                 // pairs of one schedule (sort, u32 counts)
        if ((u64)v * g.window_sets() * g.buckets >= ((u64)1 << 31)) return false;          // bucket ids below the u32 sentinel
        if ((size_t)v * g.window_sets() * MSM_G2_PT_WORDS > MSM_PENDING_WORDS - 1) return false;      // one result block per product
    }
    return true;
}
}  // namespace
int ug_plan_proof_batch(const ug_batch_schedule* schedules, int n_schedules, uint64_t n_vars, uint64_t domain, uint64_t free_bytes,
                        int requested) {
    try {
        if (n_schedules < 0 || (n_schedules && !schedules)) return 0;
        for (int k = 0; k < n_schedules; k++) {
            const ug_batch_schedule& b = schedules[k];
            if (b.c && (b.c < TABLE_MIN_C || b.c > TABLE_MAX_C || b.stride < 1 || b.stride > (255 + b.c - 1) / b.c)) return 0;
        }
        int v = requested < 1 ? 1 : requested > UG_BATCH_MAX ? UG_BATCH_MAX : requested;
        while (v > 1 && (!batch_fits(schedules, n_schedules, v) || batch_bytes(schedules, n_schedules, n_vars, domain, v) > free_bytes)) v--;
        return v;
    } catch (...) { return 0; }
}
// ... for a prover whose pass holds more per witness than the witness and h vectors (UltraGroth: gathered aux scalars, lookup
// staging): the same limits, with V * aux_bytes_per_witness counted in the memory model. aux_bytes_per_witness = 0 is
// ug_plan_proof_batch.
int ug_plan_proof_batch_aux(const ug_batch_schedule* schedules, int n_schedules, uint64_t n_vars, uint64_t domain,
                            uint64_t aux_bytes_per_witness, uint64_t free_bytes, int requested) {
    try {
        int v = ug_plan_proof_batch(schedules, n_schedules, n_vars, domain, free_bytes, requested);
        while (v > 1 && ((u64)v * aux_bytes_per_witness > free_bytes ||
                         batch_bytes(schedules, n_schedules, n_vars, domain, v) > free_bytes - (u64)v * aux_bytes_per_witness)) v--;
        return v;
    } catch (...) { return 0; }
}
int ug_bases_precompute(ug_bases* b, int c) { return ug_bases_precompute_strided(b, c, 1); }
int ug_bases_precompute_strided(ug_bases* b, int c, int stride) {
    UG_TRY
    if (!b) throw std::invalid_argument("null argument");
    if (b->table_c) throw std::invalid_argument("bases already hold window tables");
    MsmGeometry g = MsmGeometry::choose_tables(b->n, c, stride);     // validates c and the stride
    const int tables = MsmGeometry::table_count(c, stride);
    if ((b->members > 1 ? b->slots : b->n) > ((u64)1 << TABLE_INDEX_BITS)) throw std::invalid_argument("window tables need at most 2^27 points per set");
    ug_ctx* ctx = b->ctx;
    ctx->use();
    if (b->n) {
        size_t rec = b->g2 ? 128 : 64;
        DevBuf<u32> all;                             // (the set's only after the last call that can throw)
        if (!all.try_alloc((size_t)tables * b->n * (rec / 4))) throw std::runtime_error("not enough device memory for the window tables");
        UG_HIP(hipMemcpyAsync(all.get(), b->pts.get(), (size_t)b->n * rec, hipMemcpyDeviceToDevice, ctx->stream));
        build_window_tables(b->g2, all.get(), b->n, c * g.stride, tables, ctx->stream);
        UG_HIP(hipStreamSynchronize(ctx->stream));
        alloc_epoch_bump();                          // (captured launch sequences that read the old array are stale now)
        b->pts.release();
        b->pts = std::move(all);
    }
    b->table_c = c;
    b->table_stride = stride;
    UG_CATCH
}
int ug_bases_drop_tables(ug_bases* b) {
    UG_TRY
    if (!b) throw std::invalid_argument("null argument");
    b->deferred_c = 0;                               // (a deferred build that has not got its room yet is simply called off)
    b->deferred_stride = 1;
    if (!b->table_c) return UG_OK;
    ug_ctx* ctx = b->ctx;
    ctx->use();
    UG_HIP(hipStreamSynchronize(ctx->stream));
    size_t bytes = (size_t)b->n * (b->g2 ? 128 : 64);
    DevBuf<u32> small(bytes / 4);
    if (bytes) UG_HIP(hipMemcpy(small.get(), b->pts.get(), bytes, hipMemcpyDeviceToDevice));
    alloc_epoch_bump();
    b->pts.release();
    b->pts = std::move(small);
    b->table_c = 0;
    b->table_stride = 1;
    UG_CATCH
}
int ug_bases_table_window(const ug_bases* b) { return b ? b->table_c : 0; }
int ug_bases_table_stride(const ug_bases* b) { return b && b->table_c ? b->table_stride : 0; }
// DEFERRED TABLE BUILDS (cold start of a created prover). After ug_ctx_defer_tables(ctx, 1) the sets made on the context with a
// table width get the room for their tables and table 0, nothing else: ug_bases_tables_step builds the tables of the next
// `max_points` points on the context's stream and WAITS for them (a bounded piece of device time: the caller interleaves the
// pieces with proofs, which use the classic windows on table 0 until *remaining reaches 0).
int ug_ctx_defer_tables(ug_ctx* c, int on) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->defer_tables = on != 0;
    UG_CATCH
}
// The room for a deferred set's tables, in two calls: ug_bases_tables_alloc is nothing but the allocation -- it touches no stream and
// may run beside proofs (a first allocation of 36 GiB was seen to take 1.1 s, which is why create no longer makes it) -- and
// ug_bases_tables_adopt, for a moment when nothing is queued on the set's context (the caller's turn), moves the points into table
// 0 of the new array, swaps it in and frees the old one. The pieces (ug_bases_tables_step) come after it.
int ug_bases_tables_alloc(ug_bases* b, void** mem) {
    UG_TRY
    if (!b || !mem) throw std::invalid_argument("null argument");
    *mem = nullptr;
    if (!b->deferred_c || !b->n) return UG_OK;                       // nothing deferred (or nothing to build)
    b->ctx->use();
    const int windows = MsmGeometry::table_count(b->deferred_c, b->deferred_stride);
    DevBuf<u32> room;
    if (!room.try_alloc((size_t)windows * b->n * (b->g2 ? 32 : 16))) throw std::runtime_error("not enough device memory for the window tables");
    *mem = room.take();                                              // the caller's until ug_bases_tables_adopt
    UG_CATCH
}
int ug_bases_tables_adopt(ug_bases* b, void* mem) {
    UG_TRY
    if (!b) throw std::invalid_argument("null argument");
    // (mem stays the caller's until it is swapped in: a failing call leaves it with them, as ug_bases_tables_alloc handed it over)
    if (!b->deferred_c) { DevBuf<u32> unused; unused.adopt(static_cast<u32*>(mem)); return UG_OK; }      // nothing deferred any more: freed here
    ug_ctx* c = b->ctx;
    c->use();
    if (b->n) {
        if (!mem) throw std::invalid_argument("null argument");
        UG_HIP(hipMemcpyAsync(mem, b->pts.get(), (size_t)b->n * (b->g2 ? 128 : 64), hipMemcpyDeviceToDevice, c->stream));
        UG_HIP(hipStreamSynchronize(c->stream));
        alloc_epoch_bump();                          // (captured launch sequences that read the old array are stale now)
        b->pts.adopt(static_cast<u32*>(mem));        // (frees the old array here, then owns the new one)
    }
    b->table_c = b->deferred_c;
    b->table_stride = b->deferred_stride;
    b->deferred_c = 0;
    b->deferred_stride = 1;
    b->tables_built = b->n ? 0 : ~(u64)0;
    UG_CATCH
}
int ug_bases_tables_step(ug_bases* b, uint64_t max_points, uint64_t* remaining) {
    UG_TRY
    if (!b) throw std::invalid_argument("null argument");
    if (b->deferred_c) throw std::logic_error("the set's tables have no room yet (ug_bases_tables_alloc / ug_bases_tables_adopt)");
    if (b->table_c && b->tables_built < b->n) {
        ug_ctx* c = b->ctx;
        c->use();
        const u64 first = b->tables_built, count = max_points < b->n - first ? max_points : b->n - first;
        const int windows = MsmGeometry::table_count(b->table_c, b->table_stride);
        // (a group is one array of n = slots * members records; a lane of the table kernel carries 4 (G1) / 2 (G2) consecutive
        // points, so pieces start at multiples of 4)
        const u64 take = count >= b->n - first ? b->n - first : (count + 3) / 4 * 4;
        build_window_tables(b->g2, b->pts.get(), b->n, b->table_c * b->table_stride, windows, c->stream, first, take);
        UG_HIP(hipStreamSynchronize(c->stream));
        b->tables_built = first + take >= b->n ? ~(u64)0 : first + take;
    }
    if (remaining) *remaining = (b->table_c && b->tables_built < b->n) ? b->n - b->tables_built : 0;
    UG_CATCH
}
// 1: a schedule with window tables may use this set (it has none to wait for, or they are complete); 0: a deferred build is not finished
int ug_bases_tables_ready(const ug_bases* b) { return b && b->tables_usable() ? 1 : 0; }
int ug_schedule_trim(ug_schedule* s) {
    UG_TRY
    if (!s) throw std::invalid_argument("null argument");
    s->ctx->use();
    UG_HIP(hipStreamSynchronize(s->ctx->stream));
    s->sched.release();
    UG_CATCH
}
int ug_ctx_trim(ug_ctx* c) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->use();
    UG_HIP(hipStreamSynchronize(c->stream));
    c->ws_g1.release(); c->ws_g2.release(); c->raw_ntt.release();
    c->lookup_last.release(); c->lookup_last_n = 0;
    c->lookup_stage.release(); c->lookup_stage_bytes = 0;
    UG_CATCH
}
int ug_ctx_mem_info(ug_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->use();
    size_t f = 0, t = 0;
    UG_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    UG_CATCH
}
void ug_bases_destroy(ug_bases* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    alloc_epoch_bump();
    delete b;
}

int ug_dvec_create(ug_ctx* c, uint64_t n, ug_dvec** out) {
    UG_TRY
    if (!c || !out) throw std::invalid_argument("null argument");
    c->use();
    std::unique_ptr<ug_dvec> v(new ug_dvec(c, n));
    v->data.alloc((size_t)n * 8);
    *out = v.release();
    UG_CATCH
}
int ug_dvec_upload(ug_dvec* v, const void* host, uint64_t n) {
    UG_TRY
    if (!v || (!host && n)) throw std::invalid_argument("null argument");
    if (n > v->n) throw std::invalid_argument("upload larger than the vector");
    v->ctx->use();
    host_to_device(v->ctx, v->data.get(), host, (size_t)n * 32);
    UG_CATCH
}
int ug_dvec_upload_range(ug_dvec* v, const void* host, uint64_t first, uint64_t n, ug_ctx* via) {
    UG_TRY
    if (!v || (!host && n)) throw std::invalid_argument("null argument");
    if (first + n > v->n) throw std::invalid_argument("upload outside the vector");
    ug_ctx* c = via ? via : v->ctx;
    if (c->device != v->ctx->device) throw std::invalid_argument("upload context on another device");
    c->use();
    host_to_device(c, v->data.get() + first * 8, host, (size_t)n * 32);
    UG_CATCH
}
int ug_dvec_upload_idle(ug_dvec* v, const void* host, uint64_t n) {
    UG_TRY
    if (!v || (!host && n)) throw std::invalid_argument("null argument");
    if (n > v->n) throw std::invalid_argument("upload larger than the vector");
    v->ctx->use();
    // the caller vouches that nothing queued on the device reads or writes v: the copy runs on the uploader's own streams and
    // neither waits for the context's stream nor touches it (a proof may be running there)
    host_to_device(v->ctx, v->data.get(), host, (size_t)n * 32, StagedUploader::After(), /*fresh*/ true);
    UG_CATCH
}
int ug_dvec_download(const ug_dvec* v, void* host, uint64_t first, uint64_t n) {
    UG_TRY
    if (!v || (!host && n)) throw std::invalid_argument("null argument");
    if (first + n > v->n) throw std::invalid_argument("download outside the vector");
    v->ctx->use();
    if (n) UG_HIP(hipMemcpyAsync(host, v->data.get() + first * 8, (size_t)n * 32, hipMemcpyDeviceToHost, v->ctx->stream));
    UG_HIP(hipStreamSynchronize(v->ctx->stream));
    UG_CATCH
}
int ug_dvec_gather(ug_dvec* out, const ug_dvec* src, const uint32_t* host_index, uint64_t n) {
    UG_TRY
    if (!out || !src || (!host_index && n)) throw std::invalid_argument("null argument");
    if (n > out->n) throw std::invalid_argument("gather larger than the output vector");
    ug_ctx* c = out->ctx;
    c->use();
    DevBuf<u32> idx(n);
    if (n) UG_HIP(hipMemcpyAsync(idx.get(), host_index, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    gather_elements(out->data.get(), src->data.get(), idx.get(), n, src->n, c->stream);
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}
// index lists that stay on the device (UltraGroth's round_indexes / final_round_indexes are part of the zkey)
int ug_index_create(ug_ctx* c, const uint32_t* host_index, uint64_t n, ug_index** out) {
    UG_TRY
    if (!c || !out || (!host_index && n)) throw std::invalid_argument("null argument");
    c->use();
    std::unique_ptr<ug_index> ix(new ug_index{c, n});
    ix->data.alloc(n);
    if (n) UG_HIP(hipMemcpyAsync(ix->data.get(), host_index, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    *out = ix.release();
    UG_CATCH
}
void ug_index_destroy(ug_index* ix) {
    if (!ix) return;
    hipSetDevice(ix->ctx->device);
    delete ix;
}
int ug_dvec_gather_index(ug_dvec* out, const ug_dvec* src, const ug_index* index) {
    UG_TRY
    if (!out || !src || !index) throw std::invalid_argument("null argument");
    if (index->n > out->n) throw std::invalid_argument("gather larger than the output vector");
    ug_ctx* c = out->ctx;
    c->use();
    gather_elements(out->data.get(), src->data.get(), index->data.get(), index->n, src->n, c->stream);      // queued; the stream orders its users
    UG_CATCH
}
int ug_dvec_gather_index_at(ug_dvec* out, uint64_t out_first, const ug_dvec* src, const ug_index* index) {
    UG_TRY
    if (!out || !src || !index) throw std::invalid_argument("null argument");
    if (out_first > out->n || index->n > out->n - out_first) throw std::invalid_argument("gather outside the output vector");
    ug_ctx* c = out->ctx;
    c->use();
    gather_elements(out->data.get() + out_first * 8, src->data.get(), index->data.get(), index->n, src->n, c->stream);
    UG_CATCH
}
int ug_dvec_scatter(ug_dvec* dst, const uint32_t* host_index, const void* host_values, uint64_t n) {
    UG_TRY
    if (!dst || ((!host_index || !host_values) && n)) throw std::invalid_argument("null argument");
    ug_ctx* c = dst->ctx;
    c->use();
    DevBuf<u32> idx(n), val((size_t)n * 8);
    if (n) {
        UG_HIP(hipMemcpyAsync(idx.get(), host_index, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        UG_HIP(hipMemcpyAsync(val.get(), host_values, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    }
    scatter_elements(dst->data.get(), idx.get(), val.get(), n, dst->n, c->stream);
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}
int ug_dvec_apply_lookup(ug_dvec* dst, const uint32_t* w_idx, const uint32_t* p_idx, uint64_t n, const uint32_t* chunks,
                         uint64_t n_chunks, const void* table, uint64_t lookup_size) {
    UG_TRY
    if (!dst || ((!w_idx || !p_idx) && n) || (!chunks && n_chunks) || !table) throw std::invalid_argument("null argument");
    if (n >= 0xffffffffull) throw std::invalid_argument("too many lookup writes");
    const uint64_t total = 1 + n_chunks + 2 * lookup_size;          // length of the reference's push_vector
    for (uint64_t j = 0; j < n_chunks; j++)
        if (chunks[j] >= lookup_size) throw std::range_error("uwtns: chunk index outside the lookup table");
    for (uint64_t i = 0; i < n; i++)
        if (w_idx[i] >= dst->n || p_idx[i] >= total) throw std::range_error("uwtns: lookup index out of range");
    if (!n) return UG_OK;
    ug_ctx* c = dst->ctx;
    c->use();
    if (c->lookup_last_n < dst->n) {
        c->lookup_last_n = 0;
        c->lookup_last.alloc((size_t)dst->n);
        UG_HIP(hipMemsetAsync(c->lookup_last.get(), 0, (size_t)dst->n * 4, c->stream));
        c->lookup_last_n = dst->n;
    }
    // one staging allocation: w_idx | p_idx | chunks | table
    const size_t tbytes = (size_t)(1 + 2 * lookup_size) * 32;
    u32* stage = c->stage_for_lookup((size_t)(2 * n + n_chunks) * 4 + tbytes);
    u32 *d_w = stage, *d_p = stage + n, *d_c = stage + 2 * n, *d_t = stage + 2 * n + n_chunks;
    UG_HIP(hipMemcpyAsync(d_w, w_idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    UG_HIP(hipMemcpyAsync(d_p, p_idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n_chunks) UG_HIP(hipMemcpyAsync(d_c, chunks, (size_t)n_chunks * 4, hipMemcpyHostToDevice, c->stream));
    UG_HIP(hipMemcpyAsync(d_t, table, tbytes, hipMemcpyHostToDevice, c->stream));
    apply_lookup(dst->data.get(), c->lookup_last.get(), d_w, d_p, n, d_c, n_chunks, d_t, c->stream);
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}
int ug_fr_lookup_table(ug_ctx* c, const void* rand_plain, const uint32_t* frequencies, uint64_t lookup_size, void* table_out) {
    UG_TRY
    if (!c || !rand_plain || (!frequencies && lookup_size) || !table_out) throw std::invalid_argument("null argument");
    c->use();
    const size_t tbytes = (size_t)(1 + 2 * lookup_size) * 32;
    u32* table = c->stage_for_lookup(tbytes + (lookup_size ? (size_t)lookup_size * 4 : 4));
    u32* freq = table + tbytes / 4;
    UG_HIP(hipMemcpyAsync(table, rand_plain, 32, hipMemcpyHostToDevice, c->stream));
    if (lookup_size) UG_HIP(hipMemcpyAsync(freq, frequencies, (size_t)lookup_size * 4, hipMemcpyHostToDevice, c->stream));
    lookup_table(table, freq, lookup_size, c->stream);
    UG_HIP(hipMemcpyAsync(table_out, table, tbytes, hipMemcpyDeviceToHost, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}
// ---- the vector forms: V witnesses of a batched proof (include/ultragroth_hip.h) ----
// One staging buffer per call: [LookupVec x V | challenges | tables given by the caller | frequencies, w_idx, p_idx, chunks of
// every witness] goes up in ONE copy; tables made on the device follow behind it. One table launch, one mark / write / clear
// sequence over all vectors, one copy back of the tables, one host wait.
namespace {
void lookup_vectors(ug_ctx* c, ug_dvec* dst, uint64_t stride, int V, const void* rands, const ug_lookup_lists* lists,
                    const void* const* tables_in, void* const* tables_out) {
    if (!c || !lists || V < 1 || V > UG_BATCH_MAX) throw std::invalid_argument(V < 1 || V > UG_BATCH_MAX ? "vectors outside 1 .. UG_BATCH_MAX" : "null argument");
    if (!rands && !tables_in) throw std::invalid_argument("null argument");
    if (dst && (stride > dst->n || (uint64_t)V * stride > dst->n)) throw std::invalid_argument("lookup vectors outside the vector");
    uint64_t max_n = 0, max_L = 0;
    for (int v = 0; v < V; v++) {
        const ug_lookup_lists& l = lists[v];
        if ((!l.frequencies && l.lookup_size && rands) || (tables_in && !tables_in[v]) || (tables_out && !tables_out[v]))
            throw std::invalid_argument("null argument");
        max_L = std::max<uint64_t>(max_L, l.lookup_size);
        if (!dst) continue;
        if (((!l.w_idx || !l.p_idx) && l.n) || (!l.chunks && l.n_chunks)) throw std::invalid_argument("null argument");
        if (l.n >= 0xffffffffull) throw std::invalid_argument("too many lookup writes");
        const uint64_t total = 1 + l.n_chunks + 2 * l.lookup_size;
        for (uint64_t j = 0; j < l.n_chunks; j++)
            if (l.chunks[j] >= l.lookup_size) throw std::range_error("uwtns: chunk index outside the lookup table");
        for (uint64_t i = 0; i < l.n; i++)
            if (l.w_idx[i] >= stride || l.p_idx[i] >= total) throw std::range_error("uwtns: lookup index out of range");
        max_n = std::max<uint64_t>(max_n, l.n);
    }
    c->use();
    // the layout, in u32 words (descriptors, challenges and tables are multiples of 8 words: 32-byte elements stay aligned)
    const uint64_t descWords = ((uint64_t)V * sizeof(LookupVec) / 4 + 7) / 8 * 8;
    std::vector<LookupVec> vec((size_t)V);
    uint64_t at = descWords;
    for (int v = 0; v < V; v++) { vec[(size_t)v].r_off = at; at += 8; }
    auto tablesAt = [&](uint64_t from) {
        for (int v = 0; v < V; v++) { vec[(size_t)v].t_off = from; from += (1 + 2 * lists[v].lookup_size) * 8; }
        return from;
    };
    if (tables_in) at = tablesAt(at);
    for (int v = 0; v < V; v++) {
        const ug_lookup_lists& l = lists[v];
        LookupVec& d = vec[(size_t)v];
        d.L = l.lookup_size; d.n = dst ? l.n : 0; d.n_chunks = dst ? l.n_chunks : 0;
        d.f_off = at; at += rands ? d.L : 0;
        d.w_off = at; at += d.n;
        d.p_off = at; at += d.n;
        d.c_off = at; at += d.n_chunks;
    }
    const uint64_t upWords = at;
    uint64_t tablesFirst = 0, tablesWords = 0;             // tables made here: behind what goes up
    if (!tables_in) { tablesFirst = (at + 7) / 8 * 8; at = tablesAt(tablesFirst); tablesWords = at - tablesFirst; }
    std::vector<u32> host((size_t)upWords, 0);
    memcpy(host.data(), vec.data(), (size_t)V * sizeof(LookupVec));
    for (int v = 0; v < V; v++) {
        const ug_lookup_lists& l = lists[v];
        const LookupVec& d = vec[(size_t)v];
        if (rands) memcpy(&host[d.r_off], (const uint8_t*)rands + (size_t)v * 32, 32);
        if (tables_in) memcpy(&host[d.t_off], tables_in[v], (size_t)(1 + 2 * d.L) * 32);
        if (rands && d.L) memcpy(&host[d.f_off], l.frequencies, (size_t)d.L * 4);
        if (d.n) { memcpy(&host[d.w_off], l.w_idx, (size_t)d.n * 4); memcpy(&host[d.p_off], l.p_idx, (size_t)d.n * 4); }
        if (d.n_chunks) memcpy(&host[d.c_off], l.chunks, (size_t)d.n_chunks * 4);
    }
    if (dst && max_n && c->lookup_last_n < (uint64_t)V * stride) {
        c->lookup_last_n = 0;
        c->lookup_last.alloc((size_t)V * stride);
        UG_HIP(hipMemsetAsync(c->lookup_last.get(), 0, (size_t)V * stride * 4, c->stream));
        c->lookup_last_n = (uint64_t)V * stride;
    }
    u32* stage = c->stage_for_lookup((size_t)std::max(at, upWords) * 4);
    const LookupVec* vecDev = reinterpret_cast<const LookupVec*>(stage);
    UG_HIP(hipMemcpyAsync(stage, host.data(), (size_t)upWords * 4, hipMemcpyHostToDevice, c->stream));
    if (rands) lookup_tables_vectors(stage, vecDev, V, max_L, c->stream);
    if (dst) apply_lookup_vectors(dst->data.get(), stride, c->lookup_last.get(), stage, vecDev, V, max_n, c->stream);
    std::vector<u32> back;
    if (tables_out && rands) {
        back.resize((size_t)tablesWords);
        UG_HIP(hipMemcpyAsync(back.data(), stage + tablesFirst, (size_t)tablesWords * 4, hipMemcpyDeviceToHost, c->stream));
    }
    UG_HIP(hipStreamSynchronize(c->stream));
    if (tables_out && rands)
        for (int v = 0; v < V; v++)
            memcpy(tables_out[v], &back[(size_t)(vec[(size_t)v].t_off - tablesFirst)], (size_t)(1 + 2 * vec[(size_t)v].L) * 32);
}
}  // namespace
int ug_fr_lookup_tables(ug_ctx* c, int vectors, const void* rands_plain, const ug_lookup_lists* lists, void* const* tables_out) {
    UG_TRY
    if (!rands_plain || !tables_out) throw std::invalid_argument("null argument");
    lookup_vectors(c, nullptr, 0, vectors, rands_plain, lists, nullptr, tables_out);
    UG_CATCH
}
int ug_dvec_apply_lookup_vectors(ug_dvec* dst, uint64_t vector_stride, int vectors, const ug_lookup_lists* lists, const void* const* tables) {
    UG_TRY
    if (!dst || !tables) throw std::invalid_argument("null argument");
    lookup_vectors(dst->ctx, dst, vector_stride, vectors, nullptr, lists, tables, nullptr);
    UG_CATCH
}
int ug_dvec_complete_lookup_vectors(ug_dvec* dst, uint64_t vector_stride, int vectors, const void* rands_plain, const ug_lookup_lists* lists,
                                    void* const* tables_out) {
    UG_TRY
    if (!dst || !rands_plain) throw std::invalid_argument("null argument");
    lookup_vectors(dst->ctx, dst, vector_stride, vectors, rands_plain, lists, nullptr, tables_out);
    UG_CATCH
}
uint64_t ug_lookup_vectors_bytes(uint64_t vector_stride, const ug_lookup_lists* lists, int vectors) {
    if (!lists || vectors < 1) return 0;
    uint64_t bytes = 0;
    for (int v = 0; v < vectors; v++)
        bytes += sizeof(LookupVec) + 64 + 4 * vector_stride + 4 * (lists[v].lookup_size + 2 * lists[v].n + lists[v].n_chunks) +
                 32 * (1 + 2 * lists[v].lookup_size);
    return bytes;
}
uint64_t ug_dvec_size(const ug_dvec* v) { return v ? v->n : 0; }
void* ug_dvec_device_ptr(const ug_dvec* v) { return v ? v->data.get() : nullptr; }
// dst[dst_first .. + count) = src[src_first .. + count); the vectors may live on different devices of the node (peer copy over
// xGMI, or through the host when peer access is not there: hipMemcpyPeer decides). Blocking; both vectors' earlier work must be
// complete (the phase calls that produce them are).
int ug_dvec_copy(ug_dvec* dst, uint64_t dst_first, const ug_dvec* src, uint64_t src_first, uint64_t count) {
    return ug_dvec_copy_via(dst, dst_first, src, src_first, count, nullptr);
}
// the same with the copy queued on `via`'s stream (a context of dst's device; NULL = dst's own): the witness of a chain rank is
// collected from its peers on the H branch's stream while its witness products are queued on the other
int ug_dvec_copy_via(ug_dvec* dst, uint64_t dst_first, const ug_dvec* src, uint64_t src_first, uint64_t count, ug_ctx* via) {
    UG_TRY
    if (!dst || !src) throw std::invalid_argument("null argument");
    if (dst_first + count > dst->n || src_first + count > src->n) throw std::invalid_argument("copy outside the vectors");
    if (!count) return UG_OK;
    ug_ctx* c = via ? via : dst->ctx;
    if (c->device != dst->ctx->device) throw std::invalid_argument("copy context on another device than the destination");
    c->use();
    const size_t bytes = (size_t)count * 32;
    if (src->ctx->device == c->device)
        UG_HIP(hipMemcpyAsync(dst->data.get() + dst_first * 8, src->data.get() + src_first * 8, bytes, hipMemcpyDeviceToDevice, c->stream));
    else {
        // two devices of the node: direct access over xGMI is switched on once per ordered pair (the copy works without it, staged
        // by the runtime; "already enabled" and "not supported" are not errors here)
        static std::atomic<bool> tried[64][64];
        const int a = c->device, b = src->ctx->device;
        if (a >= 0 && a < 64 && b >= 0 && b < 64 && !tried[a][b].exchange(true)) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(b, 0);      // (current device is a: c->use())
            (void)hipGetLastError();
        }
        UG_HIP(hipMemcpyPeerAsync(dst->data.get() + dst_first * 8, c->device, src->data.get() + src_first * 8, src->ctx->device, bytes, c->stream));
    }
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}
int ug_dvec_wrap(ug_ctx* c, void* device_ptr, uint64_t n, ug_dvec** out) {
    UG_TRY
    if (!c || !out || (!device_ptr && n)) throw std::invalid_argument("null argument");
    if ((uintptr_t)device_ptr & 15) throw std::invalid_argument("device pointer must be 16-byte aligned");
    std::unique_ptr<ug_dvec> v(new ug_dvec(c, n));
    v->owns = false;
    v->data.adopt(static_cast<u32*>(device_ptr));
    *out = v.release();
    UG_CATCH
}
void ug_dvec_destroy(ug_dvec* v) {
    if (!v) return;
    if (v->owns) { hipSetDevice(v->ctx->device); alloc_epoch_bump(); }
    delete v;
}

int ug_schedule_create(ug_ctx* c, ug_schedule** out) {
    UG_TRY
    if (!c || !out) throw std::invalid_argument("null argument");
    ug_schedule* s = new ug_schedule();
    s->ctx = c;
    *out = s;
    UG_CATCH
}
int ug_schedule_build(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count) {
    UG_TRY
    if (!s || !scalars) throw std::invalid_argument("null argument");
    if (first + count > scalars->n) throw std::invalid_argument("schedule range outside the scalar vector");
    ug_ctx* c = s->ctx;
    c->use();
    fault_point(UG_FAULT_SCHEDULE_BUILD);
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->msm);
    s->first = first;
    MsmGeometry g = MsmGeometry::choose(count);
    g.set_classes(s->classes_for(first, count));
    s->sched.build(scalars->data.get() + first * 8, g, c->stream);
    tm.stop();
    UG_CATCH
}
int ug_schedule_build_tables(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int c) {
    return ug_schedule_build_tables_strided(s, scalars, first, count, c, 1);
}
int ug_schedule_build_tables_strided(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int c, int stride) {
    UG_TRY
    if (!s || !scalars) throw std::invalid_argument("null argument");
    if (first + count > scalars->n) throw std::invalid_argument("schedule range outside the scalar vector");
    ug_ctx* ctx = s->ctx;
    ctx->use();
    fault_point(UG_FAULT_SCHEDULE_BUILD);
    MsmGeometry g = MsmGeometry::choose_tables(count, c, stride);
    g.set_classes(s->classes_for(first, count));
    StreamTimer::Scope tm = ctx->timer.time(ctx->stream, &ctx->msm);
    s->first = first;
    s->sched.build(scalars->data.get() + first * 8, g, ctx->stream);
    tm.stop();
    UG_CATCH
}
// V scalar vectors of `count` scalars, vector v at first + v * vector_stride, in ONE schedule (batched proofs): every product
// over it writes V records (internal.hpp: MsmGeometry::vectors)
int ug_schedule_build_vectors(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int vectors, uint64_t vector_stride,
                              int table_c, int stride) {
    UG_TRY
    if (!s || !scalars) throw std::invalid_argument("null argument");
    if (vectors < 1 || vectors > MSM_MAX_VECTORS) throw std::invalid_argument("vectors outside [1, " + std::to_string(MSM_MAX_VECTORS) + "]");
    if (vectors == 1) {
        ug_ctx* c = s->ctx;
        c->use();
        return table_c ? ug_schedule_build_tables_strided(s, scalars, first, count, table_c, stride) : ug_schedule_build(s, scalars, first, count);
    }
    if (vector_stride < count) throw std::invalid_argument("vector stride below the scalars per vector");
    if (first > scalars->n || (uint64_t)(vectors - 1) * vector_stride + count > scalars->n - first)
        throw std::invalid_argument("schedule range outside the scalar vector");
    if (s->cls.on()) throw std::invalid_argument("bucket classes cannot be combined with several scalar vectors");
    ug_ctx* ctx = s->ctx;
    ctx->use();
    fault_point(UG_FAULT_SCHEDULE_BUILD);
    MsmGeometry g = table_c ? MsmGeometry::choose_tables(count, table_c, stride) : MsmGeometry::choose(count);
    g.set_vectors(vectors, vector_stride);
    StreamTimer::Scope tm = ctx->timer.time(ctx->stream, &ctx->msm);
    s->first = first;
    s->sched.build(scalars->data.get() + first * 8, g, ctx->stream);
    tm.stop();
    UG_CATCH
}
// Bucket classes for every later build of this schedule (include/ultragroth_hip.h; csrc/internal.hpp: BucketClasses)
int ug_schedule_set_classes(ug_schedule* s, int q_log, uint32_t first_residue, uint32_t residues, uint32_t specials,
                            uint64_t special_first, uint64_t special_count) {
    UG_TRY
    if (!s) throw std::invalid_argument("null argument");
    if (q_log < 0 || q_log > 8) throw std::invalid_argument("bucket classes: q_log outside [0, 8]");
    BucketClasses k;
    if (q_log) {
        if (residues < 1 || (uint64_t)first_residue + residues > ((uint64_t)1 << q_log)) throw std::invalid_argument("bucket classes: residues outside [0, 2^q_log)");
        if (specials > MSM_MAX_SPECIALS) throw std::invalid_argument("bucket classes: more than 64 special buckets");
        k.q_log = q_log; k.r0 = first_residue; k.cnt = residues; k.specials = specials;
    }
    s->cls = k;
    s->sp_first = special_first; s->sp_end = special_first + special_count;
    UG_CATCH
}
void ug_schedule_destroy(ug_schedule* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    s->sched.release();
    delete s;
}

static void affine_out_g1(uint8_t* out, const G1XYZZ& p) {
    if (is_inf(p)) { memset(out, 0, 64); return; }
    Fq x, y;
    xyzz_to_affine(x, y, p);
    u32 w[16];
    to_mont256(w, x); to_mont256(w + 8, y);
    memcpy(out, w, 64);
}
static void affine_out_g2(uint8_t* out, const G2XYZZ& p) {
    if (is_inf(p)) { memset(out, 0, 128); return; }
    Fq2 x, y;
    xyzz_to_affine(x, y, p);
    u32 w[32];
    to_mont256(w, x.a); to_mont256(w + 8, x.b); to_mont256(w + 16, y.a); to_mont256(w + 24, y.b);
    memcpy(out, w, 128);
}

// a schedule built for window tables needs bases that hold tables of the same width (a classic schedule reads table 0 only)
static void check_tables(const ug_bases* b, const ug_schedule* s) {
    if (s->sched.geo.tables && !b->tables_usable())
        throw std::logic_error("the window tables of this base set are not complete yet (ug_bases_tables_step)");
    if (s->sched.geo.tables && s->sched.geo.c != b->table_c)
        throw std::invalid_argument("schedule built for window tables of width " + std::to_string(s->sched.geo.c) +
                                    " but the bases hold " + (b->table_c ? "tables of width " + std::to_string(b->table_c) : std::string("no tables")));
    if (s->sched.geo.tables && s->sched.geo.stride != b->table_stride)
        throw std::invalid_argument("schedule built for window tables of stride " + std::to_string(s->sched.geo.stride) +
                                    " but the bases hold tables of stride " + std::to_string(b->table_stride));
}
// One product, synchronously: ug_msm_batch of one set, after the curve check
static int msm_single(ug_ctx* c, const ug_bases* b, bool g2, const ug_schedule* s, int64_t index_shift, void* out) {
    UG_TRY
    if (!c || !b || !s || !out) throw std::invalid_argument("null argument");
    if (b->g2 != g2) throw std::invalid_argument(g2 ? "ug_msm_g2 called with G1 bases" : "ug_msm_g1 called with G2 bases");
    if (!c->pending_msm.empty()) throw std::logic_error("collect the queued MSMs first (ug_ctx_collect)");
    return ug_msm_batch(c, 1, &b, s, &index_shift, &out);
    UG_CATCH
}
int ug_msm_g1(ug_ctx* c, const ug_bases* b, const ug_schedule* s, int64_t index_shift, void* out) { return msm_single(c, b, false, s, index_shift, out); }
int ug_msm_g2(ug_ctx* c, const ug_bases* b, const ug_schedule* s, int64_t index_shift, void* out) { return msm_single(c, b, true, s, index_shift, out); }

// Several MSMs over one schedule, queued back to back on the stream with ONE host synchronisation at the end: the
// latency-bound tail of one product (bucket reduction, tree sums, result copy) no longer leaves the device idle while the
// host converts the previous result (A, B1, B2, C of src/groth16.cpp:55-64 share the witness schedule).
int ug_msm_batch_enqueue(ug_ctx* c, int count, const ug_bases* const* bases, const ug_schedule* s, const int64_t* index_shifts,
                         void* const* outs) {
    UG_TRY
    if (!c || !s || (count && (!bases || !outs))) throw std::invalid_argument("null argument");
    QueueSlots slots(c, count);
    for (int k = 0; k < count; k++) {
        if (!bases[k] || !outs[k]) throw std::invalid_argument("null argument");
        if (bases[k]->members > 1) throw std::invalid_argument("a base group is multiplied with ug_msm_group_enqueue");
        check_tables(bases[k], s);
    }
    c->use();
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->msm);
    // the G1 products of the call form one batch, the G2 products another (msm.hip: msm_enqueue_multi): one accumulation
    // launch per product, the tail kernels once per batch; within a curve the caller's order is kept
    u32* host[MSM_QUEUE_DEPTH]; MsmPending pend[MSM_QUEUE_DEPTH];
    for (int k = 0; k < count; k++) host[k] = slots.add(outs[k], bases[k]->g2);
    for (int g2 = 0; g2 < 2; g2++) {
        MsmCall call; int idx[MSM_BATCH_WIDTH];
        auto flush = [&] {
            if (!call.count) return;
            MsmPending part[MSM_BATCH_WIDTH];
            msm_enqueue(g2, s->sched, g2 ? c->ws_g2 : c->ws_g1, call, c->stream, c->stat(g2), part);
            for (int q = 0; q < call.count; q++) pend[idx[q]] = part[q];
            call.count = 0;
        };
        for (int k = 0; k < count; k++) {
            const ug_bases* b = bases[k];
            if ((b->g2 ? 1 : 0) != g2) continue;
            idx[call.count] = k;                  // (an all-infinity set takes no part: msm_enqueue_multi)
            call.products[call.count++] = {b->pts.get(), b->empty ? 0 : b->n, schedule_delta(s, b, index_shifts ? index_shifts[k] : 0), host[k]};
            if (call.count == MSM_BATCH_WIDTH) flush();
        }
        flush();
    }
    slots.commit(pend);
    tm.stop();
    UG_CATCH
}
// The K products of a base group over one schedule, queued like ug_msm_batch_enqueue (results after ug_ctx_collect): ONE
// accumulation launch gathers each K-point record once and keeps K accumulators; outs[m] receives member m's sum (64 bytes).
int ug_msm_group_enqueue(ug_ctx* c, const ug_bases* group, const ug_schedule* s, void* const* outs) {
    UG_TRY
    if (!c || !group || !s || !outs) throw std::invalid_argument("null argument");
    if (group->members < 2) throw std::invalid_argument("not a base group");
    const int K = group->members;
    QueueSlots slots(c, K);
    for (int m = 0; m < K; m++) if (!outs[m]) throw std::invalid_argument("null argument");
    check_tables(group, s);
    c->use();
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->msm);
    MsmPending pend[MSM_BATCH_WIDTH];
    msm_enqueue(false, s->sched, c->ws_g1, group_call(slots, group, s, outs), c->stream, c->stat(3), pend);
    slots.commit(pend);
    tm.stop();
    UG_CATCH
}
// The witness products of a proof -- the K products of a base group (A | B1 | C, or A | B1) and the G2 product B2 over ONE schedule
// (src/groth16.cpp:55-64) -- queued so that their latency-bound ends overlap: both accumulations back to back on the context's
// stream, then the G1 tail (fix-up of cut buckets, bucket reduction, tree sums, result copy) on that stream and the G2 tail on a
// side stream beside it. The two tails are chains of dependent EC additions in kernels of a few thousand waves: one after the other
// they leave most of the chip idle, most of all on a rank of a many-device prover (round 5: one rank of eight at 2^24 22.4 -> see
// profiles/r05_variants_ab.txt item 10). Results as after ug_msm_group_enqueue + ug_msm_batch_enqueue (ug_ctx_collect).
int ug_msm_witness_enqueue(ug_ctx* c, const ug_bases* group, const ug_bases* g2set, const ug_schedule* s, void* const* outs_group, void* out_g2) {
    UG_TRY
    if (!c || !group || !g2set || !s || !outs_group || !out_g2) throw std::invalid_argument("null argument");
    if (group->members < 2 || !g2set->g2 || g2set->members > 1) throw std::invalid_argument("a base group and a G2 set are expected");
    const int K = group->members;
    QueueSlots slots(c, K + 1);
    for (int m = 0; m < K; m++) if (!outs_group[m]) throw std::invalid_argument("null argument");
    check_tables(group, s); check_tables(g2set, s);
    c->use();
    if (!c->side_stream) {
        UG_HIP(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
        c->side_fork = Event(false); c->side_join = Event(false);
    }
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->msm);
    try {
        MsmPending pend[MSM_BATCH_WIDTH + 1];      // the group's, then the G2 product's
        const MsmCall g1 = group_call(slots, group, s, outs_group);
        MsmCall g2;
        g2.count = 1;
        g2.products[0] = {g2set->pts.get(), g2set->empty ? 0 : g2set->n, schedule_delta(s, g2set), slots.add(out_g2, true)};
        // both accumulations, back to back
        msm_enqueue(false, s->sched, c->ws_g1, g1, c->stream, c->stat(3), pend, MSM_PHASE_ACCUMULATE);
        msm_enqueue(true, s->sched, c->ws_g2, g2, c->stream, c->stat(1), pend + K, MSM_PHASE_ACCUMULATE);
        // the G2 tail on the side stream, the G1 tail on the context's, then the context's stream waits for the side
        UG_HIP(hipEventRecord(c->side_fork.e, c->stream));
        UG_HIP(hipStreamWaitEvent(c->side_stream, c->side_fork.e, 0));
        msm_enqueue(true, s->sched, c->ws_g2, g2, c->side_stream, LaunchTimer(), pend + K, MSM_PHASE_TAIL);
        msm_enqueue(false, s->sched, c->ws_g1, g1, c->stream, LaunchTimer(), pend, MSM_PHASE_TAIL);
        UG_HIP(hipEventRecord(c->side_join.e, c->side_stream));
        UG_HIP(hipStreamWaitEvent(c->stream, c->side_join.e, 0));
        slots.commit(pend);
    } catch (...) {
        (void)hipStreamSynchronize(c->side_stream);      // (whatever the side stream got reads the schedule and the workspace)
        throw;
    }
    tm.stop();
    UG_CATCH
}
// ONE host wait for everything queued on the context; then the queued MSM results are finished on the host
// (Horner over the window sums, affine conversion) and written to their `out` records
int ug_ctx_collect(ug_ctx* c) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->use();
    std::vector<ug_ctx::QueuedMsm> done;
    done.swap(c->pending_msm);                                  // whatever happens below, nothing stays queued
    sync_and_resolve(c);
    for (auto& q : done)
        for (int v = 0; v < q.pend.vectors; v++) {         // a schedule of V scalar vectors: V consecutive records
            if (q.g2) affine_out_g2((uint8_t*)q.out + (size_t)v * 128, msm_collect_g2(q.pend, v));
            else affine_out_g1((uint8_t*)q.out + (size_t)v * 64, msm_collect_g1(q.pend, v));
        }
    UG_CATCH
}
// A caller that queued work (ug_msm_batch_enqueue, schedules, ug_hpoly_run) and then failed before ug_ctx_collect: waits for
// whatever is still running on the context -- the kernels read the caller's witness buffer and write the pinned result
// blocks -- and forgets the queued products, whose `out` pointers may be gone with the caller's stack frame, and with them the
// timed sections that are still pending: the time of abandoned work is not reported. Never throws.
void ug_ctx_abandon(ug_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->recording) ug_graph_abort(c->recording->c[0]);      // a capture that failed half way: nothing of it was ever queued
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    c->pending_msm.clear();
    c->timer.drop_pending();
    c->launched.clear();
}
// the pass plan of the schedule sort for keys below 2^bits (sort.hip: radix_plan): host arithmetic only, for the CPU test-suite
int ug_sort_plan(int bits, int shift[4], int bins_log[4]) {
    if (bits < 1 || bits > 32 || !shift || !bins_log) return -1;
    return radix_plan(bits, shift, bins_log);
}
int ug_test_inject_fault(int site, int after) {
    if (!test_hooks_on()) return UG_ERROR;
    g_fault_after.store(after < 1 ? 1 : after);
    g_fault_site.store(site);
    return UG_OK;
}
int ug_msm_batch(ug_ctx* c, int count, const ug_bases* const* bases, const ug_schedule* s, const int64_t* index_shifts,
                 void* const* outs) {
    int rc = ug_msm_batch_enqueue(c, count, bases, s, index_shifts, outs);
    if (rc != UG_OK) { if (c) c->pending_msm.clear(); return rc; }
    return ug_ctx_collect(c);
}

int ug_hpoly_create(ug_ctx* c, const void* host_coefs, uint64_t n_coefs, uint32_t domain, uint32_t n_vars, ug_hpoly** out) {
    UG_TRY
    if (!c || !out || (!host_coefs && n_coefs)) throw std::invalid_argument("null argument");
    if (domain == 0 || (domain & (domain - 1))) throw std::invalid_argument("domain size is not a power of two");
    if (domain > (1u << 27)) throw std::invalid_argument("domain size above 2^27 (Fr has 2-adicity 28)");
    c->use();
    std::unique_ptr<ug_hpoly, void (*)(ug_hpoly*)> hp(new ug_hpoly(), ug_hpoly_destroy);   // frees everything on any throw below
    hp->ctx = c; hp->domain = domain; hp->nvars = n_vars;
    DevBuf<uint8_t> raw((size_t)n_coefs * 44);
    host_to_device(c, raw.get(), host_coefs, (size_t)n_coefs * 44);
    const bool ok = hp->mat.build(raw.get(), n_coefs, domain, n_vars, c->stream);
    raw.release();                               // (before the plan and the workspaces are allocated)
    if (!ok) throw std::invalid_argument("coefficient record out of range (m, row or signal index)");
    hp->ntt.init(hp->mat.logn, c->stream);
    for (DevBuf<u32>* w : {&hp->a, &hp->b, &hp->c, &hp->t, &hp->t2}) w->alloc((size_t)domain * 8);
    *out = hp.release();
    UG_CATCH
}

namespace {
// The H-polynomial block of g witnesses (1 <= g <= hp->group) queued on the context's stream: witness v at w + v * w_stride
// elements, its h vector at h + v * h_stride. Every launch covers the g vectors (the matvec in tiles of witnesses, the NTT passes
// with blockIdx.z); vector v works in slice v of the workspaces. g = 1 queues the launches of a single witness, no others.
void hpoly_queue(ug_hpoly* hp, const u32* w, u64 w_stride, u32* h, u64 h_stride, int g) {
    ug_ctx* c = hp->ctx;
    hipStream_t st = c->stream;
    const u64 n = hp->domain;
    // S5-S6: a = A.w, b = B.w   (rows stored bit-reversed)            src/groth16.cpp:66-99
    coef_matvec_vectors(hp->a.get(), hp->b.get(), n, hp->mat, w, w_stride, g, st);
    if (hp->mat.logn == 0) {
        // one-point domain: every transform is the identity (n^-1 = 1, omega_2^0 = 1), nothing to fold into
        fr_mul_pointwise(hp->c.get(), hp->a.get(), hp->b.get(), n * (u64)g, st);             // (the g slices of a, b and c are adjacent)
        if (g == 1) fr_h_final(h, hp->a.get(), hp->b.get(), hp->c.get(), n, st);
        else fr_h_final_vectors(h, h_stride, hp->a.get(), hp->b.get(), hp->c.get(), n, n, g, st);
        return;
    }
    static const bool batched = !(measure_env("UG_NTT_BATCH") && atoi(measure_env("UG_NTT_BATCH")) == 0);      // A/B switch (-DUG_MEASURE)
    NttPass pa[NTT_MAX_PASSES], pb[NTT_MAX_PASSES], pc[NTT_MAX_PASSES];
    NttFusion cinv; cinv.in2 = hp->b.get(); cinv.work = hp->c.get(); cinv.in2_stride = n; cinv.work_stride = n;
    NttFusion cfwd; cfwd.work = hp->c.get(); cfwd.fin_a = hp->a.get(); cfwd.fin_b = hp->b.get(); cfwd.work_stride = n; cfwd.fin_a_stride = n; cfwd.fin_b_stride = n;
    const int np = hp->ntt.passes(pc, hp->t2.get(), hp->a.get(), /*inverse*/ true, false, /*scatter_bitrev*/ true, hp->ntt.twist.get(), nullptr, &cinv, n, n);
    if (batched && np > 1) {
        // The three chains side by side, pass by pass: ONE launch per pass index holds the same pass of all three transforms
        // (blockIdx.y), 7 launches instead of 18 for a three-pass size, and the ends of the launches fill with the other
        // chains' workgroups. Buffers: every first pass only READS a and b (chain c's forms a o b from them, S7 :100-108), so
        // chains a and b take their intermediate passes to work buffers (hp->t and the h vector, which is written last of
        // all) and scatter their twisted coefficients back into a and b; chain c works on hp->c and leaves them in hp->t2.
        NttFusion wa; wa.work = hp->t.get(); wa.work_stride = n;
        NttFusion wb; wb.work = h; wb.work_stride = h_stride;
        hp->ntt.passes(pa, hp->a.get(), hp->a.get(), true, false, true, hp->ntt.twist.get(), nullptr, &wa, n, n);      // S8 ifft + twist :110-128
        hp->ntt.passes(pb, hp->b.get(), hp->b.get(), true, false, true, hp->ntt.twist.get(), nullptr, &wb, n, n);
        const NttPass* inv3[3] = {pa, pb, pc};
        for (int p = 0; p < np; p++) hp->ntt.launch(inv3, 3, p, st, c->stat(2), g);
        // S8 fft :130-140, in place on a and b; chain c's last pass also forms h = a o b - c (S9 :142-148) from the FINISHED
        // a and b, so it goes after theirs
        hp->ntt.passes(pa, hp->a.get(), hp->a.get(), false, false, false, nullptr, nullptr, nullptr, n, n);
        hp->ntt.passes(pb, hp->b.get(), hp->b.get(), false, false, false, nullptr, nullptr, nullptr, n, n);
        hp->ntt.passes(pc, h, hp->t2.get(), false, false, false, nullptr, nullptr, &cfwd, h_stride, n);
        const NttPass* fwd3[3] = {pa, pb, pc};
        for (int p = 0; p + 1 < np; p++) hp->ntt.launch(fwd3, 3, p, st, c->stat(2), g);
        hp->ntt.launch(fwd3, 2, np - 1, st, c->stat(2), g);
        const NttPass* last[1] = {pc};
        hp->ntt.launch(last, 1, np - 1, st, c->stat(2), g);
    } else {
        // S7 + the inverse half of the third chain: c = a o b is formed inside the first pass of its ifft (:100-108), whose
        // passes run on hp->c so that a and b stay intact; the twisted coefficients wait in hp->t2
        hp->ntt.transform(hp->t2.get(), hp->a.get(), /*inverse*/ true, false, /*scatter_bitrev*/ true, hp->ntt.twist.get(), nullptr, st, c->stat(2), &cinv, g, n, n);
        // S8: ifft, twist by omega_2n^i (with 1/n folded in), fft          :110-140
        u32* polys[2] = {hp->a.get(), hp->b.get()};
        for (int p = 0; p < 2; p++) {
            hp->ntt.transform(hp->t.get(), polys[p], /*inverse*/ true, false, /*scatter_bitrev*/ true, hp->ntt.twist.get(), nullptr, st, c->stat(2), nullptr, g, n, n);
            hp->ntt.transform(polys[p], hp->t.get(), /*inverse*/ false, false, false, nullptr, nullptr, st, c->stat(2), nullptr, g, n, n);
        }
        // the forward half of the third chain, with S9 (h = a o b - c, to plain integers, :142-148) inside its last pass
        hp->ntt.transform(h, hp->t2.get(), /*inverse*/ false, false, false, nullptr, nullptr, st, c->stat(2), &cfwd, g, h_stride, n);
    }
}
}  // namespace

int ug_hpoly_run(ug_hpoly* hp, const ug_dvec* w, ug_dvec* h_out) {
    UG_TRY
    if (!hp || !w || !h_out) throw std::invalid_argument("null argument");
    if (w->n < hp->nvars) throw std::invalid_argument("witness vector shorter than nVars");
    if (h_out->n < hp->domain) throw std::invalid_argument("h vector shorter than the domain");
    if (!hp->group) throw std::runtime_error("the H-polynomial handle has no workspaces (a reservation failed): reserve again");
    ug_ctx* c = hp->ctx;
    c->use();
    fault_point(UG_FAULT_HPOLY_RUN);
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->fft);
    hpoly_queue(hp, w->data.get(), 0, h_out->data.get(), 0, 1);
    tm.stop();
    UG_CATCH
}

// The block for `vectors` witnesses (include/ultragroth_hip.h): launch groups of up to hp->group vectors, the last one smaller.
int ug_hpoly_run_vectors(ug_hpoly* hp, const ug_dvec* w, uint64_t witness_stride, int vectors, ug_dvec* h_out, uint64_t h_stride) {
    UG_TRY
    if (!hp || !w || !h_out) throw std::invalid_argument("null argument");
    if (vectors < 1 || vectors > UG_BATCH_MAX) throw std::invalid_argument("vectors outside 1 .. UG_BATCH_MAX");
    if (witness_stride < hp->nvars) throw std::invalid_argument("witness stride below nVars");
    if (h_stride < hp->domain) throw std::invalid_argument("h stride below the domain");
    if (w->n < (u64)(vectors - 1) * witness_stride + hp->nvars) throw std::invalid_argument("witness vector shorter than its last slice");
    if (h_out->n < (u64)(vectors - 1) * h_stride + hp->domain) throw std::invalid_argument("h vector shorter than its last slice");
    if (!hp->group) throw std::runtime_error("the H-polynomial handle has no workspaces (a reservation failed): reserve again");
    ug_ctx* c = hp->ctx;
    c->use();
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->fft);
    hp->last_group = vectors < hp->group ? vectors : hp->group;
    for (int v0 = 0; v0 < vectors; v0 += hp->group) {
        const int g = vectors - v0 < hp->group ? vectors - v0 : hp->group;
        for (int v = 0; v < g; v++) fault_point(UG_FAULT_HPOLY_RUN);            // (once per witness, as a loop of ug_hpoly_run)
        hpoly_queue(hp, w->data.get() + (u64)v0 * witness_stride * 8, witness_stride, h_out->data.get() + (u64)v0 * h_stride * 8, h_stride, g);
    }
    tm.stop();
    UG_CATCH
}
uint64_t ug_hpoly_vectors_bytes(uint32_t domain_size, int group) {
    return group < 1 ? 0 : (uint64_t)group * 5 * 32 * domain_size;
}
int ug_hpoly_group(const ug_hpoly* hp) { return !hp ? 0 : hp->last_group ? hp->last_group : hp->group; }
// A larger group: new workspaces first, the old ones go only when all five exist, so a reservation that does not fit changes
// nothing. A smaller group gives memory back, so the old ones go first (shedding memory must not need memory); what was just
// freed is several times what the new ones take.
int ug_hpoly_reserve_vectors(ug_hpoly* hp, int group) {
    UG_TRY
    if (!hp) throw std::invalid_argument("null argument");
    if (group < 1 || group > UG_BATCH_MAX) throw std::invalid_argument("group outside 1 .. UG_BATCH_MAX");
    if (group == hp->group) return UG_OK;
    ug_ctx* c = hp->ctx;
    c->use();
    if (c->recording) throw std::invalid_argument("no reservation while a launch sequence is being recorded");
    const size_t words = (size_t)group * hp->domain * 8;
    DevBuf<u32>* held[5] = {&hp->a, &hp->b, &hp->c, &hp->t, &hp->t2};
    const bool shrink = group < hp->group;
    if (shrink) {
        UG_HIP(hipStreamSynchronize(c->stream));               // whatever was queued on the old workspaces has finished
        alloc_epoch_bump();                                    // (recorded launch sequences point into them)
        for (int k = 0; k < 5; k++) held[k]->release();
        hp->group = 0;                                         // (no workspaces until the five below exist: the run calls refuse)
    }
    DevBuf<u32> fresh[5];                                      // (a failure below frees what it got)
    for (int k = 0; k < 5; k++) {
        if (!fresh[k].try_alloc(words))
            throw std::runtime_error("H-polynomial workspaces for " + std::to_string(group) + " vectors (" +
                                     std::to_string(ug_hpoly_vectors_bytes(hp->domain, group)) + " bytes) do not fit the device memory");
        if (k == 2) fault_point(UG_FAULT_HPOLY_RESERVE);           // (test hook: a failure with part of the workspaces allocated)
    }
    if (!shrink) {
        UG_HIP(hipStreamSynchronize(c->stream));
        alloc_epoch_bump();
        for (int k = 0; k < 5; k++) held[k]->release();
    }
    for (int k = 0; k < 5; k++) *held[k] = std::move(fresh[k]);
    hp->group = group;
    UG_CATCH
}

// coset evaluations of one of the three polynomials (0 = A.w, 1 = B.w, 2 = (A.w) o (B.w)) into `out`
// (domain elements, device form): the unit of work a rank of a sharded prover takes
int ug_hpoly_chain(ug_hpoly* hp, const ug_dvec* w, int which, ug_dvec* out) {
    UG_TRY
    if (!hp || !w || !out) throw std::invalid_argument("null argument");
    if (which < 0 || which > 2) throw std::invalid_argument("polynomial index out of range");
    if (w->n < hp->nvars) throw std::invalid_argument("witness vector shorter than nVars");
    if (out->n < hp->domain) throw std::invalid_argument("output vector shorter than the domain");
    if (!hp->group) throw std::runtime_error("the H-polynomial handle has no workspaces (a reservation failed): reserve again");
    ug_ctx* c = hp->ctx;
    c->use();
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->fft);
    hipStream_t st = c->stream;
    u64 n = hp->domain;
    if (which == 2 && hp->mat.logn == 0) {
        coef_matvec(hp->a.get(), hp->b.get(), hp->mat, w->data.get(), 3, st);
        fr_mul_pointwise(out->data.get(), hp->a.get(), hp->b.get(), n, st);                // one-point domain: the chain is the identity
        tm.stop();
        return UG_OK;
    }
    if (which == 2) {
        coef_matvec(hp->a.get(), hp->b.get(), hp->mat, w->data.get(), 3, st);
        NttFusion cinv; cinv.in2 = hp->b.get(); cinv.work = hp->c.get();             // c = a o b inside the first pass
        hp->ntt.transform(hp->t.get(), hp->a.get(), /*inverse*/ true, false, /*scatter_bitrev*/ true, hp->ntt.twist.get(), nullptr, st, c->stat(2), &cinv);
    } else {
        coef_matvec(hp->a.get(), hp->b.get(), hp->mat, w->data.get(), 1 << which, st);
        u32* src = which ? hp->b.get() : hp->a.get();
        hp->ntt.transform(hp->t.get(), src, /*inverse*/ true, false, /*scatter_bitrev*/ true, hp->ntt.twist.get(), nullptr, st, c->stat(2));
    }
    hp->ntt.transform(out->data.get(), hp->t.get(), /*inverse*/ false, false, false, nullptr, nullptr, st, c->stat(2));
    tm.stop();
    sync_and_resolve(c);                         // the caller hands the buffer to other libraries (RCCL): complete on return
    UG_CATCH
}
// h[first .. first + count) = plain(a o b - c) from the matching slices of the three coset evaluation vectors
int ug_hpoly_combine(ug_hpoly* hp, const ug_dvec* a, const ug_dvec* b, const ug_dvec* cc, uint64_t first, uint64_t count,
                     ug_dvec* h_out) {
    UG_TRY
    if (!a || !b || !cc || !h_out) throw std::invalid_argument("null argument");
    if (a->n < count || b->n < count || cc->n < count) throw std::invalid_argument("slice vectors shorter than count");
    if (first + count > h_out->n) throw std::invalid_argument("h slice outside the h vector");
    ug_ctx* c = hp ? hp->ctx : h_out->ctx;      // (a rank that runs no chain keeps no ug_hpoly: the combine needs none)
    c->use();
    StreamTimer::Scope tm = c->timer.time(c->stream, &c->fft);
    fr_h_final(h_out->data.get() + first * 8, a->data.get(), b->data.get(), cc->data.get(), count, c->stream);
    tm.stop();
    UG_CATCH
}

int ug_hpoly_debug_abc(ug_hpoly* hp, void* ha, void* hb, void* hc) {
    UG_TRY
    if (!hp) throw std::invalid_argument("null argument");
    if (!hp->group) throw std::runtime_error("the H-polynomial handle has no workspaces (a reservation failed): reserve again");
    ug_ctx* c = hp->ctx;
    c->use();
    void* host[3] = {ha, hb, hc};
    u32* dev[3] = {hp->a.get(), hp->b.get(), hp->c.get()};
    // ug_hpoly_run folds the third chain's last pass into h; its coset evaluations are re-made from the twisted coefficients
    if (hc) hp->ntt.transform(hp->c.get(), hp->t2.get(), /*inverse*/ false, false, false, nullptr, nullptr, c->stream);
    for (int p = 0; p < 3; p++) {
        if (!host[p]) continue;
        fr_to_mont256(hp->t.get(), dev[p], hp->domain, c->stream);
        UG_HIP(hipMemcpyAsync(host[p], hp->t.get(), (size_t)hp->domain * 32, hipMemcpyDeviceToHost, c->stream));
        UG_HIP(hipStreamSynchronize(c->stream));
    }
    UG_CATCH
}

void ug_hpoly_destroy(ug_hpoly* hp) {
    if (!hp) return;
    hipSetDevice(hp->ctx->device);
    alloc_epoch_bump();
    delete hp;
}

// ---- .r1cs: witness check and circuit probe (r1cs.hip) ----------------------------------------------------------------------
namespace {
void r1cs_info_of(const ughost::R1csHeader& h, const u64 terms[3], ug_r1cs_info* out) {
    out->n_wires = h.nWires; out->n_pub_out = h.nPubOut; out->n_pub_in = h.nPubIn; out->n_prv_in = h.nPrvIn;
    out->n_constraints = h.nConstraints; out->n_labels = h.nLabels;
    for (int t = 0; t < 3; t++) out->terms[t] = terms[t];
}
const u32* r1cs_witness(const ug_r1cs* r, const ug_dvec* w, u64 first) {
    if (w->ctx->device != r->ctx->device) throw std::invalid_argument("r1cs: the witness lives on another device");
    if (first > w->n || w->n - first < r->hdr.nWires)
        throw std::invalid_argument("r1cs: the witness vector is shorter than first + n_wires (" + std::to_string(r->hdr.nWires) + " wires)");
    return w->data.get() + first * 8;
}
// the check of one witness queued on `stream`, its two result words on their way to pinned memory behind it
void r1cs_queue(ug_r1cs* r, const u32* wtns, int slot, hipStream_t stream, uint8_t* mask_dev, bool timed) {
    if (timed) UG_HIP(hipEventRecord(r->t0.e, stream));
    r1cs_check(r->dev(), wtns, r->words.get() + 2 * slot, mask_dev, stream);
    if (timed) UG_HIP(hipEventRecord(r->t1.e, stream));
    UG_HIP(hipMemcpyAsync(r->words_host.get() + 2 * slot, r->words.get() + 2 * slot, 16, hipMemcpyDeviceToHost, stream));
    UG_HIP(hipEventRecord(r->done[slot].e, stream));
    r->queued[slot].wtns = wtns; r->queued[slot].stream = stream; r->queued[slot].on = true;
}
// the checks of `count` witnesses (witness v at wtns + v * stride elements) queued on `stream` as ONE launch, slots slot0 .. slot0 + count - 1;
// mask_dev: count * rows status bytes or null
void r1cs_queue_vectors(ug_r1cs* r, const u32* wtns, u64 stride, int count, int slot0, hipStream_t stream, uint8_t* mask_dev, bool timed) {
    if (timed) UG_HIP(hipEventRecord(r->t0.e, stream));
    r1cs_check_vectors(r->dev(), wtns, stride * 8, count, r->words.get() + 2 * slot0, mask_dev, stream);
    if (timed) UG_HIP(hipEventRecord(r->t1.e, stream));
    UG_HIP(hipMemcpyAsync(r->words_host.get() + 2 * slot0, r->words.get() + 2 * slot0, (size_t)16 * count, hipMemcpyDeviceToHost, stream));
    for (int v = 0; v < count; v++) {
        UG_HIP(hipEventRecord(r->done[slot0 + v].e, stream));
        r->queued[slot0 + v].wtns = wtns + (size_t)v * stride * 8; r->queued[slot0 + v].stream = stream; r->queued[slot0 + v].on = true;
    }
}
// the first of `count` witnesses `stride` elements apart, the last one inside the vector
const u32* r1cs_witnesses(const ug_r1cs* r, const ug_dvec* w, u64 first, u64 stride, int count, int slot0) {
    if (count < 1 || count > UG_BATCH_MAX) throw std::invalid_argument("r1cs: count outside 1 .. UG_BATCH_MAX");
    if (slot0 < 0 || slot0 + count > UG_BATCH_MAX) throw std::invalid_argument("r1cs: slots outside 0 .. UG_BATCH_MAX - 1");
    const u32* p = r1cs_witness(r, w, first);
    if (count > 1 && (w->n - first - r->hdr.nWires) / (u64)(count - 1) < stride)
        throw std::invalid_argument("r1cs: the witness vector is shorter than first + (count - 1) * stride + n_wires (" + std::to_string(r->hdr.nWires) + " wires)");
    return p;
}
// the slot's result; a failing witness costs a one-lane launch for the three values of its first failing constraint
void r1cs_read(ug_r1cs* r, int slot, ug_r1cs_report* out) {
    ug_r1cs::Queued& q = r->queued[slot];
    if (!q.on) throw std::invalid_argument("r1cs: no check is queued in slot " + std::to_string(slot));
    q.on = false;
    UG_HIP(hipEventSynchronize(r->done[slot].e));
    memset(out, 0, sizeof *out);
    out->failed = r->words_host.get()[2 * slot];
    if (!out->failed) return;
    out->first = ~r->words_host.get()[2 * slot + 1];
    r1cs_row_values(r->dev(), q.wtns, (u32)out->first, r->row_values.get(), q.stream);
    UG_HIP(hipMemcpyAsync(r->row_values_host.get(), r->row_values.get(), 96, hipMemcpyDeviceToHost, q.stream));
    UG_HIP(hipStreamSynchronize(q.stream));
    memcpy(out->a, r->row_values_host.get(), 32); memcpy(out->b, r->row_values_host.get() + 8, 32); memcpy(out->c, r->row_values_host.get() + 16, 32);
}
}  // namespace

int ug_r1cs_parse_info(const void* r1cs, uint64_t size, ug_r1cs_info* out) {
    UG_TRY
    if (!r1cs || !out) throw std::invalid_argument("null argument");
    ughost::BinFile f(r1cs, size, "r1cs", 1);
    const ughost::R1csHeader h = ughost::loadR1csHeader(f);
    u64 terms[3];
    ughost::countR1csTerms(f, h, terms);
    r1cs_info_of(h, terms, out);
    UG_CATCH
}
int ug_r1cs_create(ug_ctx* c, const void* r1cs, uint64_t size, ug_r1cs** out) {
    UG_TRY
    if (!c || !r1cs || !out) throw std::invalid_argument("null argument");
    ughost::BinFile f(r1cs, size, "r1cs", 1);
    ughost::R1cs host;
    ughost::loadR1cs(f, host);                                  // every rule of the layout before the first device byte
    c->use();
    std::unique_ptr<ug_r1cs, void (*)(ug_r1cs*)> r(new ug_r1cs(), ug_r1cs_destroy);      // frees everything on any throw below
    r->ctx = c; r->hdr = host.hdr;
    const size_t rows = host.hdr.nConstraints;
    for (int t = 0; t < 3; t++) {
        const size_t n = (size_t)host.terms[t];
        r->terms[t] = host.terms[t];
        r->row_ptr[t].alloc(rows + 1);
        r->sig[t].alloc(n);
        r->val[t].alloc(n * 8);
        host_to_device(c, r->row_ptr[t].get(), host.m[t].rowPtr.data(), (rows + 1) * 4);
        host_to_device(c, r->sig[t].get(), host.m[t].sig.data(), n * 4);
        // (the conversion of a chunk's coefficients runs behind that chunk's copy, on the copy's stream)
        u32* val = r->val[t].get();
        host_to_device(c, val, host.m[t].val.data(), n * 32,
                       [val](size_t off, size_t bytes, hipStream_t st) { r1cs_convert_coefs(val + off / 4, bytes / 32, st); });
    }
    const size_t words = (size_t)ug_r1cs::SLOTS * 2 + 1;
    r->words.alloc(words);
    r->words_host.alloc(words);
    r->row_values.alloc(24);
    r->row_values_host.alloc(24);
    for (int k = 0; k < ug_r1cs::SLOTS; k++) r->done[k] = Event(false);
    r->t0 = Event(true); r->t1 = Event(true);
    UG_HIP(hipStreamSynchronize(c->stream));
    *out = r.release();
    UG_CATCH
}
int ug_r1cs_get_info(const ug_r1cs* r, ug_r1cs_info* out) {
    UG_TRY
    if (!r || !out) throw std::invalid_argument("null argument");
    r1cs_info_of(r->hdr, r->terms, out);
    UG_CATCH
}
int ug_r1cs_check(ug_r1cs* r, const ug_dvec* witness, uint64_t first, ug_r1cs_report* out, uint8_t* mask) {
    UG_TRY
    if (!r || !witness || !out) throw std::invalid_argument("null argument");
    ug_ctx* c = r->ctx;
    c->use();
    if (c->recording) throw std::invalid_argument("r1cs: no check while the context's stream is being recorded");
    const u32* w = r1cs_witness(r, witness, first);
    const size_t rows = r->hdr.nConstraints;
    DevBuf<uint8_t> md;
    if (mask && rows) md.alloc(rows);
    const int slot = ug_r1cs::SLOTS - 1;
    r1cs_queue(r, w, slot, c->stream, md.get(), /*timed*/ true);
    if (md.get()) UG_HIP(hipMemcpyAsync(mask, md.get(), rows, hipMemcpyDeviceToHost, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));                    // the one host wait of a witness that holds
    r1cs_read(r, slot, out);
    float ms = 0;
    UG_HIP(hipEventElapsedTime(&ms, r->t0.e, r->t1.e));
    out->device_ms = ms;
    UG_CATCH
}
int ug_r1cs_check_enqueue(ug_r1cs* r, const ug_dvec* witness, uint64_t first, int slot, ug_ctx* via) {
    UG_TRY
    if (!r || !witness) throw std::invalid_argument("null argument");
    if (slot < 0 || slot >= UG_BATCH_MAX) throw std::invalid_argument("r1cs: slot outside 0 .. UG_BATCH_MAX - 1");
    ug_ctx* c = via ? via : r->ctx;
    if (c->device != r->ctx->device) throw std::invalid_argument("r1cs: the queueing context is on another device");
    if (c->recording) throw std::invalid_argument("r1cs: no check while the context's stream is being recorded");
    c->use();
    r1cs_queue(r, r1cs_witness(r, witness, first), slot, c->stream, nullptr, /*timed*/ false);
    UG_CATCH
}
int ug_r1cs_check_vectors_enqueue(ug_r1cs* r, const ug_dvec* witness, uint64_t first, uint64_t stride, int count, int slot0, ug_ctx* via) {
    UG_TRY
    if (!r || !witness) throw std::invalid_argument("null argument");
    ug_ctx* c = via ? via : r->ctx;
    if (c->device != r->ctx->device) throw std::invalid_argument("r1cs: the queueing context is on another device");
    if (c->recording) throw std::invalid_argument("r1cs: no check while the context's stream is being recorded");
    const u32* w = r1cs_witnesses(r, witness, first, stride, count, slot0);
    c->use();
    r1cs_queue_vectors(r, w, stride, count, slot0, c->stream, nullptr, /*timed*/ false);
    UG_CATCH
}
int ug_r1cs_check_vectors(ug_r1cs* r, const ug_dvec* witness, uint64_t first, uint64_t stride, int count, ug_r1cs_report* reports, uint8_t* masks) {
    UG_TRY
    if (!r || !witness || !reports) throw std::invalid_argument("null argument");
    ug_ctx* c = r->ctx;
    if (c->recording) throw std::invalid_argument("r1cs: no check while the context's stream is being recorded");
    const u32* w = r1cs_witnesses(r, witness, first, stride, count, 0);
    for (int v = 0; v < count; v++)
        if (r->queued[v].on) throw std::invalid_argument("r1cs: a check is still queued in slot " + std::to_string(v));
    c->use();
    const size_t rows = r->hdr.nConstraints;
    DevBuf<uint8_t> md;
    if (masks && rows) md.alloc(rows * count);
    r1cs_queue_vectors(r, w, stride, count, 0, c->stream, md.get(), /*timed*/ true);
    if (md.get()) UG_HIP(hipMemcpyAsync(masks, md.get(), rows * count, hipMemcpyDeviceToHost, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    UG_HIP(hipEventElapsedTime(&ms, r->t0.e, r->t1.e));
    for (int v = 0; v < count; v++) { r1cs_read(r, v, &reports[v]); reports[v].device_ms = ms; }      // (the one launch's time in every report)
    UG_CATCH
}
int ug_r1cs_check_collect(ug_r1cs* r, int slot, ug_r1cs_report* out) {
    UG_TRY
    if (!r || !out) throw std::invalid_argument("null argument");
    if (slot < 0 || slot >= UG_BATCH_MAX) throw std::invalid_argument("r1cs: slot outside 0 .. UG_BATCH_MAX - 1");
    r->ctx->use();
    r1cs_read(r, slot, out);
    UG_CATCH
}
int ug_r1cs_match_hpoly(ug_r1cs* r, const ug_hpoly* hp, uint32_t n_public, int* matrix, uint64_t* row) {
    UG_TRY
    if (!r || !hp || !matrix || !row) throw std::invalid_argument("null argument");
    ug_ctx* c = r->ctx;
    if (hp->ctx->device != c->device) throw std::invalid_argument("r1cs: the coefficient matrix lives on another device");
    if (hp->nvars != r->hdr.nWires)
        throw std::invalid_argument("r1cs: not this circuit: " + std::to_string(r->hdr.nWires) + " wires, the zkey has " + std::to_string(hp->nvars));
    if ((u64)n_public + 1 > r->hdr.nWires)
        throw std::invalid_argument("r1cs: not this circuit: " + std::to_string(n_public) + " public signals, " + std::to_string(r->hdr.nWires) + " wires");
    if ((u64)r->hdr.nConstraints + n_public + 1 > hp->domain)
        throw std::invalid_argument("r1cs: not this circuit: " + std::to_string(r->hdr.nConstraints) + " constraints and " +
                                    std::to_string(n_public) + " public signals do not fit the zkey's domain of " + std::to_string(hp->domain));
    c->use();
    UG_HIP(hipStreamSynchronize(hp->ctx->stream));              // (the matrix may have been built on another context's stream)
    const size_t n = r->hdr.nWires;
    std::vector<uint8_t> z(n * 32);
    ughost::randomBytes(z.data(), z.size());
    for (size_t i = 0; i < n; i++) z[i * 32 + 31] &= 0x1f;      // below 2^253 < r
    DevBuf<u32> zd(n * 8);
    host_to_device(c, zd.get(), z.data(), n * 32);
    unsigned long long* word = r->words.get() + 2 * ug_r1cs::SLOTS;
    unsigned long long* word_host = r->words_host.get() + 2 * ug_r1cs::SLOTS;
    r1cs_match(r->dev(), hp->mat, n_public, zd.get(), word, c->stream);
    UG_HIP(hipMemcpyAsync(word_host, word, 8, hipMemcpyDeviceToHost, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    if (*word_host == ~0ull) { *matrix = -1; *row = 0; }
    else { *matrix = (int)(*word_host & 1); *row = *word_host >> 1; }
    UG_CATCH
}
// what the two folds share: the argument rules, the waits on the vectors' streams, the event pair around `launch` and its time.
// classes: the entry takes a class vector (cls); vectors: how many of 2^log_domain elements `out` takes
static int r1cs_fold_call(ug_r1cs* r, const ug_dvec* rho, bool classes, const ug_dvec* cls, uint32_t n_public, uint32_t log_domain,
                          int vectors, ug_dvec* out, double* kernel_ms, const std::function<void(u32 domain)>& launch) {
    UG_TRY
    if (!r || !rho || (classes && !cls) || !out) throw std::invalid_argument("null argument");
    ug_ctx* c = r->ctx;
    if (rho->ctx->device != c->device || (classes && cls->ctx->device != c->device) || out->ctx->device != c->device)
        throw std::invalid_argument("r1cs: a vector lives on another device");
    if (c->recording) throw std::invalid_argument("r1cs: no fold while the context's stream is being recorded");
    if (log_domain > 27) throw std::invalid_argument("r1cs: log_domain " + std::to_string(log_domain) + " is above 27");
    const u64 N = (u64)1 << log_domain;
    if (rho->n < r->hdr.nWires) throw std::invalid_argument("r1cs: the weight vector is shorter than n_wires (" + std::to_string(r->hdr.nWires) + " wires)");
    if (classes && cls->n * 32 < r->hdr.nWires) throw std::invalid_argument("r1cs: the class vector holds fewer than n_wires bytes");
    if ((u64)n_public + 1 > r->hdr.nWires) throw std::invalid_argument("r1cs: " + std::to_string(n_public) + " public signals, " + std::to_string(r->hdr.nWires) + " wires");
    if ((u64)r->hdr.nConstraints + n_public + 1 > N)
        throw std::invalid_argument("r1cs: " + std::to_string(r->hdr.nConstraints) + " constraints and " + std::to_string(n_public) +
                                    " public signals do not fit a domain of " + std::to_string(N));
    if (out->n < (u64)vectors * N) throw std::invalid_argument("r1cs: the output vector is shorter than " + std::to_string(vectors) + " * 2^log_domain");
    c->use();
    UG_HIP(hipStreamSynchronize(rho->ctx->stream));             // (the weights may have been queued on another context's stream)
    if (classes && cls->ctx != rho->ctx) UG_HIP(hipStreamSynchronize(cls->ctx->stream));
    if (out->ctx != rho->ctx) UG_HIP(hipStreamSynchronize(out->ctx->stream));
    UG_HIP(hipEventRecord(r->t0.e, c->stream));
    launch((u32)N);
    UG_HIP(hipEventRecord(r->t1.e, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    UG_HIP(hipEventElapsedTime(&ms, r->t0.e, r->t1.e));
    if (kernel_ms) *kernel_ms = ms;
    UG_CATCH
}
int ug_r1cs_fold_dvec(ug_r1cs* r, const ug_dvec* rho, uint32_t n_public, uint32_t log_domain, ug_dvec* out, double* kernel_ms) {
    return r1cs_fold_call(r, rho, false, nullptr, n_public, log_domain, 8, out, kernel_ms, [&](u32 domain) {
        r1cs_fold(r->dev(), rho->data.get(), n_public, domain, out->data.get(), r->ctx->stream);
    });
}
int ug_r1cs_fold_classes_dvec(ug_r1cs* r, const ug_dvec* rho, const ug_dvec* cls, uint32_t n_public, uint32_t log_domain, ug_dvec* out,
                              double* kernel_ms) {
    return r1cs_fold_call(r, rho, true, cls, n_public, log_domain, 11, out, kernel_ms, [&](u32 domain) {
        r1cs_fold_classes(r->dev(), rho->data.get(), reinterpret_cast<const uint8_t*>(cls->data.get()), n_public, domain, out->data.get(), r->ctx->stream);
    });
}
void ug_r1cs_destroy(ug_r1cs* r) {
    if (!r) return;
    hipSetDevice(r->ctx->device);
    for (int k = 0; k < ug_r1cs::SLOTS; k++)                    // a check that was queued and never collected may still be running
        if (r->queued[k].on) hipEventSynchronize(r->done[k].e);
    delete r;
}

int ug_fr_ntt(ug_ctx* c, void* host_data, int logn, int inverse) {
    UG_TRY
    if (!c || !host_data) throw std::invalid_argument("null argument");
    if (logn < 0 || logn > 27) throw std::invalid_argument("logn out of range");
    c->use();
    if (c->raw_ntt.logn != logn) c->raw_ntt.init(logn, c->stream);
    size_t bytes = ((size_t)1 << logn) * 32;
    DevBuf<u32> x_own(bytes / 4), y_own(bytes / 4);
    u32 *const x = x_own.get(), *const y = y_own.get();
    UG_HIP(hipMemcpyAsync(x, host_data, bytes, hipMemcpyHostToDevice, c->stream));
    fr_from_mont256(x, x, (u64)1 << logn, c->stream);
    if (logn == 0) UG_HIP(hipMemcpyAsync(y, x, bytes, hipMemcpyDeviceToDevice, c->stream));
    else c->raw_ntt.transform(y, x, inverse != 0, /*gather_bitrev*/ true, false, nullptr, inverse ? c->raw_ntt.ninv.get() : nullptr, c->stream);
    fr_to_mont256(y, y, (u64)1 << logn, c->stream);
    UG_HIP(hipMemcpyAsync(host_data, y, bytes, hipMemcpyDeviceToHost, c->stream));
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}

int ug_field_op(ug_ctx* c, int field, int op, void* out, const void* a, const void* b, uint64_t n) {
    UG_TRY
    if (!c || !out || !a || !b) throw std::invalid_argument("null argument");
    if (field != UG_FIELD_FR && field != UG_FIELD_FQ) throw std::invalid_argument("unknown field");
    if (op < 0 || op > 3) throw std::invalid_argument("unknown op");
    c->use();
    size_t bytes = (size_t)n * 32;
    DevBuf<u32> da_own(bytes / 4), db_own(bytes / 4), dout_own(bytes / 4);
    u32 *const da = da_own.get(), *const db = db_own.get(), *const dout = dout_own.get();
    if (n) {
        UG_HIP(hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, c->stream));
        UG_HIP(hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, c->stream));
        f_op_mont256(field, op, dout, da, db, n, c->stream);
        UG_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    UG_HIP(hipStreamSynchronize(c->stream));
    UG_CATCH
}

int ug_synth_points(ug_ctx* c, int g2, const void* generator_record, uint64_t seed, uint64_t n, void* host_out) {
    UG_TRY
    if (!c || !generator_record || (!host_out && n)) throw std::invalid_argument("null argument");
    c->use();
    size_t rec = g2 ? 128 : 64;
    u32 gen[32];
    memcpy(gen, generator_record, rec);
    const u64 CH = (u64)1 << 22;                       // stage through a bounded device buffer
    DevBuf<u32> dev_own((size_t)(n < CH ? (n ? n : 1) : CH) * (rec / 4));
    u32* const dev = dev_own.get();
    for (u64 done = 0; done < n; done += CH) {
        u64 m = n - done < CH ? n - done : CH;
        synth_points(g2 != 0, dev, gen, seed + done, m, c->stream);
        UG_HIP(hipMemcpy((uint8_t*)host_out + done * rec, dev, (size_t)m * rec, hipMemcpyDeviceToHost));
    }
    UG_CATCH
}

// ---- captured launch sequences ---------------------------------------------------------------------------------------------
// A created prover's proof is one fixed sequence of 60-75 launches on two streams, none of which depends on a host read-back:
// captured once per witness buffer, replayed with one hipGraphLaunch. ug_graph_begin puts the context's stream into capture
// (relaxed mode: other host threads -- the witness staging lanes -- go on using the runtime) and forks ctx2's stream off it;
// everything the library queues on either context until ug_graph_end becomes a node: kernels, memsets, the result copies into
// pinned memory, and the timing events as event-record nodes (dev_common.hpp: record_in_capture), so that the MSM | FFT split and the per-kernel statistics
// keep working under replay. Nothing runs during the capture. ug_graph_end joins the streams, instantiates, and takes the
// products that were queued (ug_msm_*_enqueue) out of the contexts; ug_graph_launch puts them back and launches: the caller
// then collects as after the eager calls -- ug_ctx_collect on the FIRST context first (the graph runs on its stream).
int ug_graph_begin(ug_ctx* c, ug_ctx* c2) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    if (c2 && c2->device != c->device) throw std::invalid_argument("contexts on different devices");
    if (c->recording || (c2 && c2->recording)) throw std::logic_error("a capture is already in progress on this context");
    if (!c->pending_msm.empty() || (c2 && !c2->pending_msm.empty())) throw std::logic_error("collect the queued MSMs first (ug_ctx_collect)");
    c->use();
    sync_and_resolve(c);                                   // pending spans and statistics of eager work: accounted before the switch
    if (c2) sync_and_resolve(c2);
    std::unique_ptr<ug_graph> g(new ug_graph());
    g->c[0] = c; g->c[1] = c2;
    UG_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    g->capturing = true;
    ug_graph* raw = g.release();
    c->recording = raw;
    c->timer.capture_into(&raw->pairs[0]);
    if (c2) {
        c2->recording = raw;
        c2->timer.capture_into(&raw->pairs[1]);
        hipError_t e = hipEventRecord(c->order_event.e, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c2->stream, c->order_event.e, 0);      // ctx2's stream joins the capture
        if (e != hipSuccess) { ug_graph_abort(c); UG_HIP(e); }
    }
    UG_CATCH
}
static void graph_unhook(ug_graph* g) {
    for (int q = 0; q < 2; q++) {
        if (!g->c[q]) continue;
        g->c[q]->recording = nullptr;
        g->c[q]->timer.capture_into(nullptr);
    }
}
void ug_graph_abort(ug_ctx* c) {
    if (!c || !c->recording) return;
    ug_graph* g = c->recording;
    (void)hipSetDevice(c->device);
    graph_unhook(g);
    for (int q = 0; q < 2; q++) if (g->c[q]) g->c[q]->pending_msm.clear();
    if (g->capturing) {
        hipGraph_t broken = nullptr;
        (void)hipStreamEndCapture(g->c[0]->stream, &broken);
        if (broken) (void)hipGraphDestroy(broken);
        (void)hipGetLastError();
        g->capturing = false;
    }
    ug_graph_destroy(g);
}
int ug_graph_end(ug_ctx* c, ug_graph** out) {
    UG_TRY
    if (!c || !out) throw std::invalid_argument("null argument");
    if (!c->recording || c->recording->c[0] != c) throw std::logic_error("no capture was begun on this context");
    ug_graph* g = c->recording;
    c->use();
    try {
        if (g->c[1]) {                                     // join: the first stream waits for everything queued on the second
            UG_HIP(hipEventRecord(g->c[1]->order_event.e, g->c[1]->stream));
            UG_HIP(hipStreamWaitEvent(c->stream, g->c[1]->order_event.e, 0));
        }
        hipError_t e = hipStreamEndCapture(c->stream, &g->graph);
        g->capturing = false;
        UG_HIP(e);
        if (!g->graph) throw std::runtime_error("stream capture produced no graph");
        UG_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0));
        (void)hipGraphGetNodes(g->graph, nullptr, &g->nodes);
    } catch (...) { ug_graph_abort(c); throw; }
    graph_unhook(g);
    for (int q = 0; q < 2; q++) if (g->c[q]) { g->pend[q].swap(g->c[q]->pending_msm); g->c[q]->pending_msm.clear(); }
    g->epoch = alloc_epoch();
    *out = g;
    UG_CATCH
}
// 1 while every buffer the captured launches refer to is still where it was (no per-proof device buffer of this process has been
// allocated or released since the capture ended)
int ug_graph_valid(const ug_graph* g) { return g && g->exec && g->epoch == alloc_epoch() ? 1 : 0; }
uint64_t ug_graph_nodes(const ug_graph* g) { return g ? g->nodes : 0; }
int ug_graph_launch(ug_graph* g) {
    UG_TRY
    if (!g || !g->exec) throw std::invalid_argument("null argument");
    if (!ug_graph_valid(g)) throw std::logic_error("the captured launch sequence is stale (device buffers were re-allocated since)");
    ug_ctx* c = g->c[0];
    c->use();
    for (int q = 0; q < 2; q++)
        if (g->c[q] && (!g->c[q]->pending_msm.empty() || g->c[q]->recording)) throw std::logic_error("collect the queued MSMs first (ug_ctx_collect)");
    // a launch whose event pairs have not been read yet would be overwritten: account it first (a caller that collects after
    // every launch never waits here)
    for (ug_graph* l : c->launched) if (l == g) { sync_and_resolve(c); break; }
    for (int q = 0; q < 2; q++) if (g->c[q]) g->c[q]->pending_msm = g->pend[q];
    hipError_t e = hipGraphLaunch(g->exec, c->stream);
    if (e != hipSuccess) { for (int q = 0; q < 2; q++) if (g->c[q]) g->c[q]->pending_msm.clear(); UG_HIP(e); }
    c->launched.push_back(g);
    UG_CATCH
}
void ug_graph_destroy(ug_graph* g) {
    if (!g) return;
    if (g->c[0]) {
        (void)hipSetDevice(g->c[0]->device);
        // a launch may still run, and the context may still want to read its event pairs
        if (!g->capturing) (void)hipStreamSynchronize(g->c[0]->stream);
        auto& l = g->c[0]->launched;
        for (size_t i = 0; i < l.size();) { if (l[i] == g) l.erase(l.begin() + (long)i); else i++; }
    }
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;                                   // (with its event pairs)
    (void)hipGetLastError();
}

int ug_ctx_timings(ug_ctx* c, double* msm_ms, double* fft_ms, int reset) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    c->use();
    sync_and_resolve(c);
    if (msm_ms) *msm_ms = c->msm.ms;
    if (fft_ms) *fft_ms = c->fft.ms;
    if (reset) { c->msm = TimeSink(); c->fft = TimeSink(); }
    UG_CATCH
}
int ug_ctx_kernel_stats(ug_ctx* c, int which, double* avg_ms, uint64_t* launches, uint64_t* entries, int reset) {
    UG_TRY
    if (!c) throw std::invalid_argument("null argument");
    if (which < 0 || which > 3) throw std::invalid_argument("kernel stats: 0 = G1 accumulation, 1 = G2 accumulation, 2 = NTT pass, 3 = G1 group accumulation");
    c->use();
    sync_and_resolve(c);
    TimeSink& st = c->kernel[which];
    if (avg_ms) *avg_ms = st.launches ? st.ms / (double)st.launches : 0.0;
    if (launches) *launches = st.launches;
    if (entries) *entries = st.units;
    if (reset) { st = TimeSink(); c->kernel_stats_on = true; }
    UG_CATCH
}

}  // extern "C"
