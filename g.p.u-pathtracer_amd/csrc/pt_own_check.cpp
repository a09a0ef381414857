// pt_own_check.cpp — the owners of pt_own.h over host stubs of the runtime's calls: a CPU program with its own main, linked
// against no HIP library (make own_check; SAN=1 adds the address and undefined-behaviour sanitizers).  The stubs count the live
// objects, log the order of the calls and can make the next allocation fail.  Every case ends with nothing alive.  Exit status 0: all
// checks hold; else the failed ones are printed.
#include "pt_own.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {
int live_blocks = 0, live_events = 0, live_streams = 0;
int n_malloc = 0, n_free = 0, n_event_create = 0, n_event_destroy = 0, n_stream_create = 0, n_stream_destroy = 0;
bool fail_next_malloc = false;
unsigned last_event_flags = ~0u, last_stream_flags = ~0u;
int last_stream_priority = 0;
std::string call_log;   // 'm' malloc, 'f' free, 'e' / 'E' event create / destroy, 's' / 'S' stream create / destroy
int failures = 0;

void reset_stubs() {
    n_malloc = n_free = n_event_create = n_event_destroy = n_stream_create = n_stream_destroy = 0;
    fail_next_malloc = false;
    last_event_flags = last_stream_flags = ~0u;
    last_stream_priority = 0;
    call_log.clear();
}
bool nothing_alive() { return live_blocks == 0 && live_events == 0 && live_streams == 0; }
}  // namespace

// ---- the runtime, over malloc ------------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    call_log += 'm';
    if (fail_next_malloc) {
        fail_next_malloc = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    n_malloc++;
    live_blocks++;
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    call_log += 'f';
    if (!p) return hipSuccess;
    n_free++;
    live_blocks--;
    std::free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    call_log += 'e';
    n_event_create++;
    live_events++;
    last_event_flags = flags;
    *e = (hipEvent_t)std::malloc(1);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDefault); }
hipError_t hipEventDestroy(hipEvent_t e) {
    call_log += 'E';
    n_event_destroy++;
    live_events--;
    std::free((void*)e);
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) {
    call_log += 's';
    n_stream_create++;
    live_streams++;
    last_stream_flags = flags;
    last_stream_priority = priority;
    *s = (hipStream_t)std::malloc(1);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return hipStreamCreateWithPriority(s, flags, 0); }
hipError_t hipStreamDestroy(hipStream_t s) {
    call_log += 'S';
    n_stream_destroy++;
    live_streams--;
    std::free((void*)s);
    return hipSuccess;
}
}

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                         \
        }                                                                       \
    } while (0)

using namespace ptmi;

static void check_devbuf() {
    reset_stubs();
    {
        DevBuf<float> b;
        CHECK(b.get() == nullptr && b.count() == 0 && b.bytes() == 0 && !b);
        CHECK(b.alloc(3) == hipSuccess);
        CHECK(b.get() != nullptr && b.count() == 3 && b.bytes() == 12 && b);
        b.get()[2] = 1.0f;   // (the block is as large as it says: the sanitizer build watches)
        CHECK(b.alloc(5) == hipSuccess);
        CHECK(live_blocks == 1 && n_malloc == 2 && n_free == 1 && b.count() == 5);
        b.get()[4] = 1.0f;

        DevBuf<float> m(std::move(b));   // move-construction
        CHECK(b.get() == nullptr && b.count() == 0 && m.count() == 5 && live_blocks == 1);
        DevBuf<float> a;
        CHECK(a.alloc(2) == hipSuccess && live_blocks == 2);
        float* const was = m.get();
        a = std::move(m);   // move-assignment: a's own block goes, m's comes
        CHECK(a.get() == was && a.count() == 5 && m.get() == nullptr && m.count() == 0 && live_blocks == 1);
        DevBuf<float>& self = a;
        a = std::move(self);   // self-move-assignment keeps the block
        CHECK(a.get() == was && a.count() == 5 && live_blocks == 1);

        a.reset();
        a.reset();   // twice
        CHECK(a.get() == nullptr && a.count() == 0 && live_blocks == 0 && n_free == n_malloc);

        CHECK(a.alloc(0) == hipSuccess && a.get() == nullptr && a.count() == 0);   // nothing asked for: empty, no call
        CHECK(a.alloc(4) == hipSuccess);
        fail_next_malloc = true;
        CHECK(a.alloc(8) == hipErrorOutOfMemory);
        CHECK(a.get() == nullptr && a.count() == 0 && live_blocks == 0);
        CHECK(a.alloc(1) == hipSuccess);   // left to the destructor
    }
    CHECK(nothing_alive());
}

static void check_grow_only() {
    reset_stubs();
    {
        DevBuf<int> b;
        CHECK(b.reserve(4) == hipSuccess && b.count() == 4);
        int* const p4 = b.get();
        CHECK(b.reserve(2) == hipSuccess);
        CHECK(b.get() == p4 && b.count() == 4 && n_malloc == 1 && n_free == 0);
        CHECK(b.reserve(4) == hipSuccess && b.get() == p4 && n_malloc == 1);
        call_log.clear();
        CHECK(b.reserve(8) == hipSuccess && b.count() == 8);
        CHECK(call_log == "fm");   // the old block is released BEFORE the new one is asked for
        CHECK(live_blocks == 1);
        fail_next_malloc = true;
        CHECK(b.reserve(16) == hipErrorOutOfMemory);
        CHECK(b.get() == nullptr && b.count() == 0 && live_blocks == 0);   // empty, not dangling
        CHECK(b.reserve(1) == hipSuccess && b.count() == 1);               // and usable again
    }
    CHECK(nothing_alive());
}

static void check_event_stream() {
    reset_stubs();
    {
        Event e;
        CHECK((hipEvent_t)e == nullptr);
        CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e != nullptr);
        CHECK(last_event_flags == hipEventDisableTiming);
        const hipEvent_t was = e;
        CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e == was && n_event_create == 1);   // twice: once
        Event d;
        CHECK(d.ensure() == hipSuccess && last_event_flags == hipEventDefault && live_events == 2);
        Event m(std::move(e));
        CHECK((hipEvent_t)e == nullptr && (hipEvent_t)m == was && live_events == 2);
        d = std::move(m);   // d's own event goes
        CHECK((hipEvent_t)d == was && (hipEvent_t)m == nullptr && live_events == 1 && n_event_destroy == 1);
        Event& self = d;
        d = std::move(self);
        CHECK((hipEvent_t)d == was && live_events == 1);
        CHECK(e.ensure() == hipSuccess && live_events == 2);   // a moved-from event is an empty one: usable again

        Stream s;
        CHECK((hipStream_t)s == nullptr);
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && (hipStream_t)s != nullptr && last_stream_flags == hipStreamNonBlocking);
        Stream p;
        CHECK(p.create(hipStreamNonBlocking, -1) == hipSuccess && last_stream_priority == -1 && last_stream_flags == hipStreamNonBlocking);
        CHECK(live_streams == 2);
        const hipStream_t sp = p;
        Stream q(std::move(p));
        CHECK((hipStream_t)p == nullptr && (hipStream_t)q == sp && live_streams == 2);
        s = std::move(q);
        CHECK((hipStream_t)s == sp && (hipStream_t)q == nullptr && live_streams == 1 && n_stream_destroy == 1);
    }
    // moved-from objects destroyed nothing: every creation met exactly one destruction
    CHECK(n_event_destroy == n_event_create && n_stream_destroy == n_stream_create);
    CHECK(nothing_alive());
}

static void check_devtemp() {
    reset_stubs();
    {
        DevTemp t;
        float* a = nullptr;
        int* b = nullptr;
        char* c = nullptr;
        double* d = nullptr;
        short* z = nullptr;
        CHECK(t.get(&a, 4) == hipSuccess && a);
        CHECK(t.get(&b, 1) == hipSuccess && b);
        fail_next_malloc = true;
        CHECK(t.get(&c, 9) == hipErrorOutOfMemory && c == nullptr);
        CHECK(t.get(&d, 2) == hipSuccess && d);
        CHECK(t.get(&z, 0) == hipSuccess && z);   // an empty request still gets a block of its own
        CHECK(live_blocks == 4 && n_free == 0);
    }
    CHECK(n_free == 4);
    CHECK(nothing_alive());
}

// one member of each owner, as the context holds them: built, half filled, destroyed (members go in reverse order of declaration)
struct Holder {
    Stream stream;
    Event ready, never_made;
    DevBuf<float> filled, empty;
    DevTemp temp;
};

static void check_struct() {
    reset_stubs();
    {
        Holder h;
        CHECK(h.stream.create(hipStreamNonBlocking) == hipSuccess);
        CHECK(h.ready.ensure() == hipSuccess);
        CHECK(h.filled.alloc(7) == hipSuccess);
        int* t = nullptr;
        CHECK(h.temp.get(&t, 3) == hipSuccess);
        call_log.clear();
    }
    CHECK(call_log == "ffES");   // the buffers first, the stream last
    {
        struct Value { DevBuf<float> filled, empty; Event ready; } a, b;   // as the scene's values are adopted: built in a local, moved over the old one
        CHECK(a.filled.alloc(1) == hipSuccess && a.ready.ensure() == hipSuccess && b.filled.alloc(2) == hipSuccess);
        b = std::move(a);   // b's own block is released, a is left empty
        CHECK(live_blocks == 1 && live_events == 1 && a.filled.get() == nullptr && (hipEvent_t)a.ready == nullptr && b.filled.count() == 1);
    }
    CHECK(nothing_alive());
}

int main() {
    check_devbuf();
    check_grow_only();
    check_event_stream();
    check_devtemp();
    check_struct();
    if (failures == 0) std::printf("pt_own_check: DevBuf, grow-only, Event, Stream, DevTemp, struct of owners: all checks hold, nothing left alive\n");
    else std::printf("pt_own_check: %d check(s) FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
