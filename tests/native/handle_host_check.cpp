// handle_host_check.cpp -- csrc/handle_host.h on the host, by itself (tests/test_handle_host_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and links it to the HIP runtime).  A toy handle goes through what a module's create and
// destroy do when the device cannot be had: the ordinal 2^20 exists on no machine, so handle_open fails at hipSetDevice with or
// without a GPU and nothing here ever launches.
//   open fails, then the created-tail: the handle is destroyed, the text of the FIRST failing call survives, *out stays null
//   close of a handle whose every member is null; close of what a failed open left; close twice
//   a failing check before the open (a create's own RT_CHECK) through the same tail
//   elapsed before anything was recorded: RTMODT_E_INVALID in the module's own words
//   a timer that was never created: destroy is harmless
// The leak checker of the sanitized build sees the toy's own allocation: a tail that forgot the destroy would be reported.
#include <cstdarg>
#include <cstdio>
#include <string>

#include "handle_host.h"

namespace rtmodt {
std::string &last_error() {
    static thread_local std::string e;
    return e;
}
int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}
void note_bad_option(const char *) {}
}  // namespace rtmodt

using namespace rtmodt;

static int failures = 0;
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            ++failures; printf("FAIL " __VA_ARGS__); printf("\n"); \
        }                                                        \
    } while (0)

struct Toy : HandleBase {
    EventTimer<3> timer;
    int *own = nullptr;                 // what the module holds: freed by its destroy, seen by the leak checker
};

static int destroyed = 0;
static void toy_destroy(Toy *t) {
    if (!t) return;
    handle_close(t, [&] {
        delete[] t->own;
        t->timer.destroy();
        last_error() = "overwritten by the destroy";       // a destroy may fail inside and leave its own text: the tail must put the first one back
    });
    ++destroyed;
    delete t;
}

static const int NO_DEVICE = 1 << 20;

static int toy_create(int device, bool bad_argument, Toy **out) {
    Toy *t = new Toy();
    t->device = device;
    t->own = new int[16]();
    auto body = [&]() -> int {
        RT_CHECK(!bad_argument, RTMODT_E_CAPACITY, "toy: capacity %d", 7);
        RT_TRY(handle_open(t));
        RT_TRY(t->timer.create());
        return RTMODT_OK;
    };
    return handle_created(body(), t, toy_destroy, out);
}

int main() {
    {   // open failing at hipSetDevice, followed by the created-tail
        Toy *out = nullptr;
        destroyed = 0;
        const int rc = toy_create(NO_DEVICE, false, &out);
        EXPECT(rc == RTMODT_E_HIP, "create on device 2^20: rc %d", rc);
        EXPECT(out == nullptr, "*out was written on failure");
        EXPECT(destroyed == 1, "the handle was destroyed %d times", destroyed);
        EXPECT(last_error().find("hipSetDevice") != std::string::npos, "error text: %s", last_error().c_str());
        EXPECT(last_error().find("handle_host.h") != std::string::npos, "the location names the shared header: %s", last_error().c_str());
        printf("ok open fails: %s\n", last_error().c_str());
    }
    {   // a check of the create itself, before the device is touched
        Toy *out = nullptr;
        destroyed = 0;
        const int rc = toy_create(NO_DEVICE, true, &out);
        EXPECT(rc == RTMODT_E_CAPACITY && out == nullptr && destroyed == 1, "failing check: rc %d, out %p, destroyed %d", rc, (void *)out, destroyed);
        EXPECT(last_error() == "toy: capacity 7", "error text: %s", last_error().c_str());
        printf("ok check fails\n");
    }
    {   // close of a handle with every member null, and once more
        HandleBase b;
        b.device = NO_DEVICE;
        int freed = 0;
        handle_close(&b, [&] { ++freed; });
        handle_close(&b, [&] { ++freed; });
        EXPECT(freed == 2 && b.stream == nullptr, "close of an empty handle: freed %d", freed);
        hipStream_t same = nullptr;
        handle_close(&b, [&] { ++freed; }, same);          // a last foreign stream that is not set
        EXPECT(freed == 3, "close with a null last stream");
        printf("ok close of an empty handle\n");
    }
    {   // close called on what a failed open left
        Toy t;
        t.device = NO_DEVICE;
        last_error().clear();
        const int rc = handle_open(&t);
        const std::string first = last_error();
        EXPECT(rc == RTMODT_E_HIP && t.stream == nullptr, "open: rc %d, stream %p", rc, (void *)t.stream);
        int freed = 0;
        handle_close(&t, [&] { t.timer.destroy(); ++freed; });
        EXPECT(freed == 1 && t.stream == nullptr, "close after a failed open");
        EXPECT(last_error() == first, "close touched the error text: %s", last_error().c_str());
        printf("ok close after a failed open\n");
    }
    {   // elapsed before anything was recorded; destroy of a timer that was never created
        EventTimer<2> timer;
        float ms = -1.f;
        const int rc = timer.elapsed(NO_DEVICE, 0, 1, &ms, "no process call has launched yet");
        EXPECT(rc == RTMODT_E_INVALID, "elapsed on a fresh timer: rc %d", rc);
        EXPECT(last_error() == "no process call has launched yet", "error text: %s", last_error().c_str());
        EXPECT(ms == -1.f, "elapsed wrote its output");
        const int rc2 = timer.elapsed(NO_DEVICE, 0, 1, &ms, "100% of no embed has run yet");       // the words are data, not a format
        EXPECT(rc2 == RTMODT_E_INVALID && last_error() == "100% of no embed has run yet", "error text: %s", last_error().c_str());
        timer.destroy();
        timer.destroy();
        for (hipEvent_t e : timer.ev) EXPECT(e == nullptr, "an event appeared");
        printf("ok timer\n");
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("all ok\n");
    return 0;
}
