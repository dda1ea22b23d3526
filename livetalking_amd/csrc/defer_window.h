// Knob DEFER: the host-side bookkeeping of deferred Wav2Lip calls, and the choice of the prefetch slot a call fills.  No HIP in here:
// the event type and what is done with an event come from the user (the engine: hipEvent_t; tests/native/defer_window_main.cpp: fake
// events), so the CPU suite drives the same code the engine runs.
//
// Rule (include/ltk.h, ltk_wav2lip_infer_deferred): a deferred call returns when its own pass is enqueued and every pass issued before
// it is complete.  A pass that is enqueued and not yet KNOWN to be complete has a record in the window: its event (recorded on the
// compute stream behind the pass), what must outlive the pass instead of the call (the avatar banks), the frame ranges it writes and the
// prefetch slot it works in.  The call that follows waits for the records it found, then retires them; with one caller thread the
// window holds one record whenever a call returns.
#pragma once
#include <stddef.h>

#include <memory>
#include <mutex>
#include <vector>

namespace ltk {

struct PredRange {
    const unsigned char* p = nullptr;
    size_t bytes = 0;
    bool overlaps(const void* q, size_t n) const {
        const unsigned char* b = (const unsigned char*)q;
        return n && bytes && b < p + bytes && p < b + n;
    }
};

template <class Event>
struct PendingPass {
    Event ev{};                                   // recorded on the compute stream behind the pass; owned by the record for its life
    std::vector<std::shared_ptr<void>> hold;      // the avatar banks the pass (and the prefetch it launched) reads
    std::vector<PredRange> ranges;                // the d_pred blocks the pass writes
    int slot = 0;                                 // the prefetch slot (concat-buffer set) the pass works in; 0: the arena's own
    unsigned long seq = 0;                        // issue number, 1-based
};

struct DeferStats {
    unsigned long long deferred = 0;              // calls that returned with their own pass outstanding
    unsigned long long max_outstanding = 0;       // most records in the window when such a call returned
    unsigned long long outstanding = 0;           // records in the window now
};

// The window.  Its lock is a leaf (taken under the engine's enqueue lock by push, alone by everything else, never held across a wait).
// Records are shared_ptr: a waiter keeps the record - and so its event - while it waits, whoever retires it meanwhile.  Retired records
// go to a small pool and are taken from it again once nobody else refers to them, so a steady session creates no event per call.
template <class Event>
class DeferWindow {
   public:
    using Rec = std::shared_ptr<PendingPass<Event>>;

    // a record with a usable event: from the pool, or a new one whose event `create(Event*)` (returns true on success) makes; null
    // when that fails
    template <class Create>
    Rec acquire(Create create) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < pool_.size(); ++i)
                if (pool_[i].use_count() == 1) {
                    Rec r = std::move(pool_[i]);
                    pool_.erase(pool_.begin() + i);
                    return r;
                }
        }
        Rec r = std::make_shared<PendingPass<Event>>();
        if (!create(&r->ev)) return nullptr;
        return r;
    }
    // an acquired record that was not pushed after all (the call failed, or ran synchronously)
    void give_back(Rec r) {
        if (!r) return;
        clear_record(*r);
        std::lock_guard<std::mutex> g(mu_);
        pool_.push_back(std::move(r));
    }
    // `r`'s pass has been enqueued and its event recorded (under the enqueue lock, so window order = stream order).  Returns the
    // records that were in the window: the passes in front of it, oldest first.
    std::vector<Rec> push(const Rec& r) {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<Rec> before = live_;
        r->seq = ++issued_;
        live_.push_back(r);
        return before;
    }
    // every record of the window, oldest first (drains, and synchronous calls: what their own completion implies is complete)
    std::vector<Rec> snapshot() {
        std::lock_guard<std::mutex> g(mu_);
        return live_;
    }
    // `r`'s pass is complete (its event, or a later one of the same stream, has been waited for): what it held goes
    void retire(const Rec& r) {
        std::vector<std::shared_ptr<void>> drop;     // released outside the lock: the last reference to a bank frees device memory
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < live_.size(); ++i)
                if (live_[i] == r) {
                    live_.erase(live_.begin() + i);
                    drop.swap(r->hold);
                    r->ranges.clear();
                    r->slot = 0;
                    pool_.push_back(r);
                    break;
                }
        }
    }
    // a deferred call is about to return
    void returned() {
        std::lock_guard<std::mutex> g(mu_);
        ++stats_.deferred;
        if (live_.size() > stats_.max_outstanding) stats_.max_outstanding = live_.size();
    }
    // the records whose pass writes into [p, p + bytes): a reader of those frames on another stream waits for their events first
    std::vector<Rec> writers_of(const void* p, size_t bytes) {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<Rec> out;
        for (const Rec& r : live_)
            for (const PredRange& q : r->ranges)
                if (q.overlaps(p, bytes)) { out.push_back(r); break; }
        return out;
    }
    // a pass that may still be running works in prefetch slot `slot`
    bool slot_in_use(int slot) {
        if (slot <= 0) return false;
        std::lock_guard<std::mutex> g(mu_);
        for (const Rec& r : live_)
            if (r->slot == slot) return true;
        return false;
    }
    // bit k set: a pass that may still be running works in prefetch slot k (1 <= k < 64); one lock for a whole slot scan
    unsigned long long slots_in_use() {
        std::lock_guard<std::mutex> g(mu_);
        unsigned long long m = 0;
        for (const Rec& r : live_)
            if (r->slot > 0 && r->slot < 64) m |= 1ull << r->slot;
        return m;
    }
    // the newest record (null: none): the pass the next one runs behind
    Rec newest() {
        std::lock_guard<std::mutex> g(mu_);
        return live_.empty() ? nullptr : live_.back();
    }
    DeferStats stats() {
        std::lock_guard<std::mutex> g(mu_);
        DeferStats s = stats_;
        s.outstanding = live_.size();
        return s;
    }
    // engine teardown, after the device has been drained: every event is handed to `destroy(Event&)`
    template <class Destroy>
    void clear(Destroy destroy) {
        std::vector<Rec> all;
        {
            std::lock_guard<std::mutex> g(mu_);
            all.swap(live_);
            for (Rec& r : pool_) all.push_back(std::move(r));
            pool_.clear();
        }
        for (Rec& r : all) { clear_record(*r); destroy(r->ev); }
    }

   private:
    static void clear_record(PendingPass<Event>& r) { r.hold.clear(); r.ranges.clear(); r.slot = 0; }
    std::mutex mu_;
    std::vector<Rec> live_;      // issue order
    std::vector<Rec> pool_;
    unsigned long issued_ = 0;
    DeferStats stats_;
};

// ---------------------------------------------------------------- which prefetch slot the next call's face encoder goes into
// What the choice looks at, per slot (index 0 unused, as in the engine's table).
struct PfSlotView {
    bool valid = false;          // holds data a call has not come for yet
    double age = 0;              // seconds since it was filled
    bool reader_running = false; // the last pass that worked in it may still be running (its event is not complete, or a deferred
                                 // pass of the window works in it)
    unsigned long stamp = 0;     // LRU clock of the last fill / use
};

// Victim: a slot nobody is waiting for - consumed, never used, or filled for a call that did not come within `stale` seconds - other
// than `cur` (the slot the calling pass works in); among those the MOST recently used whose last reader is done, so that a lone
// session walks as few slots (and captured graphs) as it can: two when its calls are synchronous, three when they are deferred (the
// slot of the pass still running is skipped).  When every candidate's reader is still running, the most recently used of those (the
// prefetch then waits for that pass).  0: no slot (every other slot is waited for).
inline int choose_prefetch_slot(const PfSlotView* s, int nslots, int cur, double stale) {
    int victim = 0, busy = 0;
    for (int k = 1; k <= nslots; ++k) {
        if (k == cur) continue;
        if (s[k].valid && s[k].age < stale) continue;
        if (s[k].reader_running) { if (!busy || s[k].stamp > s[busy].stamp) busy = k; continue; }
        if (!victim || s[k].stamp > s[victim].stamp) victim = k;
    }
    return victim ? victim : busy;
}

// The lone session's walk under `choose_prefetch_slot`, host side only: which slot call `n` (0-based) works in (0 = whole pass) and
// which it prefetches into, given how many earlier passes may still be running when a call enqueues (0: synchronous calls, 1:
// deferred).  Used by the tests to derive the call at which every graph variant has been captured; mirrors ltk_wav2lip_infer's
// bookkeeping with every prefetch succeeding.
struct SoloWalk {
    static constexpr int kSlots = 16;
    PfSlotView s[kSlots + 1];
    unsigned long clock = 0;
    int filled_for_next = 0;     // slot holding the next call's encoder outputs
    int calls = 0;
    int prev_slot = 0;           // slot of the pass issued by the previous call
    struct Step { int slot, prefetch_into; };
    Step call(int depth) {
        Step st{filled_for_next, 0};
        const bool hit = st.slot > 0;
        if (hit) { s[st.slot].valid = false; s[st.slot].stamp = ++clock; }
        const bool prefetch = hit || calls > 0;              // a continuing sequence: the second call of a session prefetches first
        if (prefetch) {
            for (int k = 1; k <= kSlots; ++k) s[k].reader_running = depth > 0 && k == prev_slot && k != 0;
            const int v = choose_prefetch_slot(s, kSlots, st.slot, 1.5);
            if (v) { s[v].valid = true; s[v].age = 0; s[v].stamp = ++clock; }
            st.prefetch_into = v;
        }
        filled_for_next = st.prefetch_into;
        prev_slot = st.slot;
        ++calls;
        return st;
    }
    void jump() { filled_for_next = 0; calls = 0; }            // the index jumped: the next call misses and does not prefetch
};

// The last call (0-based) of a lone session's first `calls` calls that runs a launch variant - the pass in a slot, the prefetch into a
// slot - for the first or second time (eager run, then capture: knob GRAPH); from the call after it everything replays.  `jump_at`:
// the index jumps in front of that call (-1: never).  *slots_used: prefetch slots the walk touched.
inline int solo_walk_last_capture(int depth, int calls, int jump_at, int* slots_used) {
    SoloWalk walk;
    int seen_pass[SoloWalk::kSlots + 1] = {0}, seen_pf[SoloWalk::kSlots + 1] = {0};
    int last = 0, used = 0;
    for (int n = 0; n < calls; ++n) {
        if (n == jump_at) walk.jump();
        const SoloWalk::Step st = walk.call(depth);
        if (++seen_pass[st.slot] <= 2) last = n;
        if (st.prefetch_into && ++seen_pf[st.prefetch_into] <= 2) last = n;
    }
    for (int k = 1; k <= SoloWalk::kSlots; ++k) used += seen_pf[k] ? 1 : 0;
    if (slots_used) *slots_used = used;
    return last;
}

}  // namespace ltk
