// Knob table: environment read once, then plain array reads (tune.h).
#include "tune.h"

#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <map>
#include <set>
#include <vector>
#include <utility>

namespace ltk {
namespace {

struct KnobDef { const char* name; int dflt; };
const KnobDef kDefs[K_COUNT] = {
#define LTK_KNOB_DEF(name, dflt) {"LTK_" #name, dflt},
    LTK_KNOBS(LTK_KNOB_DEF)
#undef LTK_KNOB_DEF
};

std::atomic<int> g_val[K_COUNT];     // knob_set (tests, tuners) may run beside launch threads reading the table
std::atomic<unsigned> g_epoch{0};
std::once_flag g_once;

void init() {
    for (int i = 0; i < K_COUNT; ++i) {
        const char* e = getenv(kDefs[i].name);
        // presence-style switches: any value means 1 - the empty string, "true", "yes" - unless the WHOLE value parses as a
        // number (LTK_FACE_CACHE=0 switches it off again)
        int v = kDefs[i].dflt;
        if (e) {
            char* end = nullptr;
            const long n = strtol(e, &end, 10);
            v = (*e != 0 && end && *end == 0) ? (int)n : 1;
        }
        g_val[i].store(v, std::memory_order_relaxed);
    }
}

}  // namespace

int knob(Knob k) {
    std::call_once(g_once, init);
    return g_val[k].load(std::memory_order_relaxed);
}

int ensure_dyn_lds(const void* func, int bytes) {
    // Runs in front of every conv launch (~70 per eager pass, from any engine / session thread): the common case is answered from
    // a per-thread cache without a lock; the process-wide table behind it records the byte count configured per (device,
    // function), so a later, larger request re-sets the attribute instead of being skipped.
    struct Seen { int dev; const void* func; int bytes; };
    thread_local std::vector<Seen> mine;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (const Seen& s : mine)
        if (s.func == func && s.dev == dev && s.bytes >= bytes) return 0;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> done;
    int have = 0;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = done.find({dev, func});
        if (it != done.end()) have = it->second;
        if (have < bytes) {
            const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (e != hipSuccess) return (int)e;
            done[{dev, func}] = have = bytes;
        }
    }
    for (Seen& s : mine)
        if (s.func == func && s.dev == dev) { s.bytes = have; return 0; }
    mine.push_back({dev, func, have});
    return 0;
}

unsigned knob_epoch() { return g_epoch.load(std::memory_order_relaxed); }

int knob_set(const char* name, int value) {
    std::call_once(g_once, init);
    if (!name) return -1;
    for (int i = 0; i < K_COUNT; ++i)
        if (!strcmp(name, kDefs[i].name) || !strcmp(name, kDefs[i].name + 4)) {
            g_val[i].store(value, std::memory_order_relaxed);
            g_epoch.fetch_add(1, std::memory_order_relaxed);
            return 0;
        }
    return -1;
}

}  // namespace ltk
