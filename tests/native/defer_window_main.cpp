// Drives csrc/defer_window.h (the window of deferred Wav2Lip passes and the prefetch-slot choice) with fake events, the way
// engine_internal.h infer_call and w2l_infer.hip drive it with HIP events.  Built with -fsanitize=address,undefined and run by
// tests/test_defer_host.py; prints one line per sequence and exits non-zero on the first failed check.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../livetalking_amd/csrc/defer_window.h"

using namespace ltk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

// A fake device: one in-order stream.  An event is the number of the pass it was recorded behind; waiting for it completes every pass
// up to that number (what hipEventSynchronize on an in-order stream implies).
struct FakeEvent { int id = 0; long recorded = 0; };
struct Bank { int* alive; explicit Bank(int* a) : alive(a) { ++*alive; } ~Bank() { --*alive; } };

struct FakeEngine {
    DeferWindow<FakeEvent> win;
    long enqueued = 0, completed = 0;
    int events_made = 0, events_destroyed = 0, banks_alive = 0;
    long fail_pass = 0;                       // this pass fails on the device: whoever waits for it (or a later one) sees it
    bool seen_failure = false;

    bool wait(const FakeEvent& ev) {          // false: a pass up to ev.recorded failed asynchronously
        const bool bad = fail_pass && !seen_failure && fail_pass > completed && fail_pass <= ev.recorded;
        if (ev.recorded > completed) completed = ev.recorded;
        if (bad) seen_failure = true;
        return !bad;
    }
    // infer_call.  deferred: as ltk_wav2lip_infer_deferred for a solo call; bad_request: the enqueue lambda refuses.  Returns 0, -1
    // (refused) or -2 (device failure).
    int call(bool deferred, bool bad_request, std::shared_ptr<Bank> bank, const unsigned char* pred, size_t bytes, int slot) {
        auto rec = win.acquire([&](FakeEvent* ev) { ev->id = ++events_made; return true; });
        CHECK(rec);
        CHECK(rec->hold.empty() && rec->ranges.empty() && rec->slot == 0);
        if (bad_request) { drain(); win.give_back(rec); return -1; }
        rec->ev.recorded = ++enqueued;
        std::vector<DeferWindow<FakeEvent>::Rec> before;
        if (deferred) {
            rec->hold.push_back(bank);
            rec->ranges.push_back({pred, bytes});
            rec->slot = slot;
            before = win.push(rec);
            int rc = 0;
            if (!before.empty() && !wait(before.back()->ev)) rc = -2;
            for (auto& r : before) win.retire(r);
            if (rc) { completed = enqueued; win.retire(rec); return rc; }
            win.returned();
            return 0;
        }
        before = win.snapshot();
        const bool ok = wait(rec->ev);
        for (auto& r : before) win.retire(r);
        win.give_back(rec);
        return ok ? 0 : -2;
    }
    int drain() {
        auto recs = win.snapshot();
        if (recs.empty()) return 0;
        const bool ok = wait(recs.back()->ev);
        for (auto& r : recs) win.retire(r);
        return ok ? 0 : -2;
    }
    void destroy() {
        completed = enqueued;                 // hipDeviceSynchronize
        drain();
        win.clear([&](FakeEvent& ev) { CHECK(ev.id > 0); ev.id = 0; ++events_destroyed; });
    }
};

static unsigned char g_frames[16][64];

static void steady_walk() {
    FakeEngine e;
    auto bank = std::make_shared<Bank>(&e.banks_alive);
    SoloWalk walk;
    for (int n = 0; n < 14; ++n) {
        const SoloWalk::Step st = walk.call(1);
        CHECK(e.call(true, false, bank, g_frames[n], 64, st.slot) == 0);
        // at most one pass is outstanding when a call returns, and it is this call's
        CHECK(e.win.stats().outstanding == 1);
        CHECK(e.completed == n);                               // every earlier pass is complete
        CHECK(e.win.writers_of(g_frames[n], 64).size() == 1);
        CHECK(e.win.writers_of(g_frames[n] + 63, 1).size() == 1);
        if (n) CHECK(e.win.writers_of(g_frames[n - 1], 64).empty());   // older frames: complete by the depth-1 rule
        CHECK(e.win.slot_in_use(st.slot) == (st.slot > 0));
    }
    const DeferStats s = e.win.stats();
    CHECK(s.deferred == 14 && s.max_outstanding == 1);
    CHECK(e.events_made == 2);                                  // the pool: a steady session creates no event per call
    CHECK(e.drain() == 0 && e.win.stats().outstanding == 0 && e.completed == 14);
    bank.reset();
    CHECK(e.banks_alive == 0);
    e.destroy();
    CHECK(e.events_destroyed == e.events_made);
    printf("steady walk: ok\n");
}

// the lone session's slot rotation: two slots when calls are synchronous, three when deferred
static int captured_by(int depth, int calls, int jump_at, int* slots_used) {
    SoloWalk walk;
    for (int n = 0; n < calls; ++n) {
        if (n == jump_at) walk.jump();
        const SoloWalk::Step st = walk.call(depth);
        CHECK(!st.prefetch_into || st.prefetch_into != st.slot);
        CHECK(n < 2 || n == jump_at || n == jump_at + 1 || st.slot > 0);       // every continuing call starts at the decoder
    }
    return solo_walk_last_capture(depth, calls, jump_at, slots_used);
}

static void slot_rotation() {
    int used = 0;
    int last = captured_by(0, 40, -1, &used);
    CHECK(used == 2);
    printf("synchronous walk: %d slots, last capture at call %d\n", used, last);
    last = captured_by(1, 40, -1, &used);
    CHECK(used == 3);
    CHECK(last == 7);                  // 0-based: the eighth call; a benchmark's 8 priming + 5 warm-up calls cover it
    CHECK(last + 1 <= 13);
    printf("deferred walk: %d slots, last capture at call %d\n", used, last);
    // the slot the running pass reads is never the victim, whatever the stamps say
    PfSlotView v[5];
    v[1].stamp = 9; v[1].reader_running = true; v[2].stamp = 3; v[3].stamp = 1; v[4].valid = true; v[4].age = 0.1; v[4].stamp = 20;
    CHECK(choose_prefetch_slot(v, 4, 2, 1.5) == 3);
    v[3].reader_running = true;
    CHECK(choose_prefetch_slot(v, 4, 2, 1.5) == 1);             // every candidate busy: the most recently used of them
    v[4].age = 2.0;
    CHECK(choose_prefetch_slot(v, 4, 2, 1.5) == 4);             // a stale slot is free again
    PfSlotView w[3];
    w[1].valid = true; w[1].age = 0.0;
    CHECK(choose_prefetch_slot(w, 2, 2, 1.5) == 0);             // everything else is waited for: no prefetch
    printf("slot rotation: ok\n");
}

static void jump() {
    int used = 0;
    const int last = captured_by(1, 40, 9, &used);
    // the slot filled for the call that never came stays reserved until it is stale: the walk moves to a fourth slot
    CHECK(used == 4);
    printf("deferred walk with a jump at call 9: %d slots, last capture at call %d\n", used, last);
    FakeEngine e;
    auto bank = std::make_shared<Bank>(&e.banks_alive);
    for (int n = 0; n < 6; ++n) CHECK(e.call(true, false, bank, g_frames[n % 2], 64, n % 3) == 0);
    // frames of call 5 live where call 3's did: only the pass in flight counts
    CHECK(e.win.writers_of(g_frames[1], 64).size() == 1 && e.win.writers_of(g_frames[0], 64).empty());
    e.destroy();
    printf("jump: ok\n");
}

static void release_while_pending() {
    FakeEngine e;
    auto bank = std::make_shared<Bank>(&e.banks_alive);
    CHECK(e.call(true, false, bank, g_frames[0], 64, 0) == 0);
    bank.reset();                                   // the table's reference goes (ltk_avatar_release, without its drain)
    CHECK(e.banks_alive == 1);                      // the pass holds the bank, not the call
    CHECK(e.drain() == 0);                          // ltk_avatar_release drains
    CHECK(e.banks_alive == 0 && e.completed == 1);
    e.destroy();
    printf("release while pending: ok\n");
}

static void error_while_pending() {
    FakeEngine e;
    auto bank = std::make_shared<Bank>(&e.banks_alive);
    CHECK(e.call(true, false, bank, g_frames[0], 64, 0) == 0);
    CHECK(e.call(true, true, bank, g_frames[1], 64, 0) == -1);       // refused: the earlier pass is drained, its frames are complete
    CHECK(e.completed == 1 && e.win.stats().outstanding == 0);
    CHECK(e.call(true, false, bank, g_frames[2], 64, 0) == 0);       // the engine stays usable
    e.fail_pass = e.enqueued;                                        // ... and that pass fails on the device
    CHECK(e.call(true, false, bank, g_frames[3], 64, 0) == -2);      // reported by the call that waited for it
    CHECK(e.win.stats().outstanding == 0 && e.completed == e.enqueued);    // nothing of either call is in flight
    CHECK(e.call(false, false, bank, g_frames[4], 64, 0) == 0);
    CHECK(e.call(true, false, bank, g_frames[5], 64, 1) == 0);
    CHECK(e.call(false, false, bank, g_frames[6], 64, 0) == 0);      // a synchronous call runs behind the pass in flight and retires it
    CHECK(e.win.stats().outstanding == 0 && e.completed == e.enqueued);
    bank.reset();
    CHECK(e.banks_alive == 0);
    e.destroy();
    printf("error while pending: ok\n");
}

static void destroy_with_pending() {
    FakeEngine e;
    auto bank = std::make_shared<Bank>(&e.banks_alive);
    CHECK(e.call(true, false, bank, g_frames[0], 64, 2) == 0);
    CHECK(e.call(true, false, bank, g_frames[1], 64, 3) == 0);
    bank.reset();
    CHECK(e.banks_alive == 1 && e.win.stats().outstanding == 1);
    e.destroy();
    CHECK(e.banks_alive == 0 && e.events_destroyed == e.events_made && e.win.stats().outstanding == 0);
    // a waiter that still holds a record keeps its event out of the pool's hands
    FakeEngine f;
    auto b2 = std::make_shared<Bank>(&f.banks_alive);
    CHECK(f.call(true, false, b2, g_frames[0], 64, 0) == 0);
    auto held = f.win.newest();
    CHECK(f.drain() == 0);
    CHECK(f.call(true, false, b2, g_frames[1], 64, 0) == 0);
    CHECK(f.win.newest() != held);                  // not reused while `held` refers to it
    held.reset();
    f.destroy();
    printf("destroy with a pass pending: ok\n");
}

int main() {
    steady_walk();
    slot_rotation();
    jump();
    release_while_pending();
    error_while_pending();
    destroy_with_pending();
    printf("all ok\n");
    return 0;
}
