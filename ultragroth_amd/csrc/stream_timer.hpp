// stream_timer.hpp -- device time of launch sections on one stream, accounted without host waits.
#pragma once
#include <vector>
#include "dev_common.hpp"

namespace ug {

// where elapsed time is accounted: one per thing that is measured (a context's MSM | FFT split, one kernel class's launches)
struct TimeSink {
    double ms = 0; u64 launches = 0; u64 units = 0;
    void add(float ms_, u64 units_) { ms += ms_; launches++; units += units_; }
};

// Every timed section is an event pair recorded around it on the stream; the elapsed time goes to the section's sink the next
// time the stream is known to be idle (resolve), or -- for a caller that never waits -- once the pair is seen to have finished
// (drain_ready). The timer owns every event it creates and reuses them: a section costs no allocation in steady state.
// While the stream is being captured into a graph (capture_into) the pairs are made for the graph instead and belong to the
// vector given: event-record nodes (dev_common.hpp: record_in_capture) that every launch of the graph records again, one
// completed launch being accounted with account().
class StreamTimer {
public:
    struct Pair { Event e0, e1; TimeSink* sink = nullptr; u64 units = 0; };
    static constexpr size_t DRAIN_AT = 64;       // outstanding pairs at which time() looks for finished ones

    // A timed section: from time() to stop(). Destroyed without stop() -- the section threw -- its pair goes back unused.
    class Scope {
        StreamTimer* t = nullptr;                // null: inert, or stopped
        hipStream_t stream = nullptr;
        bool captured = false;
        Pair pair;
    public:
        Scope() = default;
        Scope(StreamTimer* timer, hipStream_t stream_, TimeSink* sink, u64 units) : stream(stream_) {
            if (!sink) return;
            if (timer->capture) {
                captured = true;
                pair.e0 = Event(true); pair.e1 = Event(true);
                record_in_capture(pair.e0.e, stream);
            } else {
                if (timer->pending.size() >= DRAIN_AT) timer->drain_ready();
                if (timer->idle.empty()) {       // nothing has finished either: the pool grows, no section goes untimed
                    Pair fresh;
                    fresh.e0 = Event(true); fresh.e1 = Event(true);
                    timer->idle.push_back(std::move(fresh));
                }
                UG_HIP(hipEventRecord(timer->idle.back().e0.e, stream));
                pair = std::move(timer->idle.back());
                timer->idle.pop_back();
            }
            pair.sink = sink; pair.units = units;
            t = timer;
        }
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
        ~Scope() { if (t && !captured) t->idle.push_back(std::move(pair)); }
        void stop() {
            if (!t) return;
            if (captured) record_in_capture(pair.e1.e, stream);
            else UG_HIP(hipEventRecord(pair.e1.e, stream));
            (captured ? *t->capture : t->pending).push_back(std::move(pair));
            t = nullptr;
        }
    };

    // sink == nullptr: an inert scope -- no event is taken, nothing is recorded
    Scope time(hipStream_t stream, TimeSink* sink, u64 units = 0) { return Scope(this, stream, sink, units); }
    // after the stream has been synchronised
    void resolve() {
        while (!pending.empty()) {
            Pair& p = pending.back();
            float ms = 0;
            UG_HIP(hipEventElapsedTime(&ms, p.e0.e, p.e1.e));
            p.sink->add(ms, p.units);
            idle.push_back(std::move(p));
            pending.pop_back();
        }
    }
    // the sections that have finished, without waiting
    void drain_ready() {
        size_t keep = 0;
        for (Pair& p : pending) {
            float ms = 0;
            if (hipEventQuery(p.e1.e) == hipSuccess && hipEventElapsedTime(&ms, p.e0.e, p.e1.e) == hipSuccess) {
                p.sink->add(ms, p.units);
                idle.push_back(std::move(p));
            } else {
                if (&pending[keep] != &p) pending[keep] = std::move(p);
                keep++;
            }
        }
        (void)hipGetLastError();                 // hipEventQuery reports hipErrorNotReady through the error state
        pending.resize(keep);
    }
    // the queued sections are given up: nothing is accounted, the events are kept
    void drop_pending() {
        for (Pair& p : pending) idle.push_back(std::move(p));
        pending.clear();
    }
    void capture_into(std::vector<Pair>* pairs) { capture = pairs; }
    // one completed launch of the graph that owns these pairs
    static void account(const std::vector<Pair>& pairs) {
        for (const Pair& p : pairs) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.e0.e, p.e1.e) == hipSuccess) p.sink->add(ms, p.units);
            else (void)hipGetLastError();
        }
    }

private:
    std::vector<Pair> idle, pending;
    std::vector<Pair>* capture = nullptr;
};

// the timing argument of the launch functions (msm_enqueue, NttPlan::launch): every launch of one kernel class is a section
// of `timer` that goes to `sink` with its work units; the default times nothing
struct LaunchTimer {
    StreamTimer* timer = nullptr; TimeSink* sink = nullptr;
    StreamTimer::Scope time(hipStream_t stream, u64 units) const { return StreamTimer::Scope(timer, stream, sink, units); }
};

}  // namespace ug
