// order_host_check.cpp -- csrc/lmpc_order.h under the host compiler's sanitizers: the cross-stream ordering of a context's
// buffers and the grown buffer, instantiated with an Api that logs every call in place of HIP's.  Each case asserts the
// exact sequence of calls.  S is the context's own stream, A, B, C callers' streams.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lmpc_order.h"

namespace {

std::vector<std::string> calls;
int fail_records = 0;  // the next so many record() calls fail
bool fail_alloc = false;
int live_blocks = 0;

struct FakeApi {
    using Error = int;
    using Stream = char;
    using Event = int;
    static constexpr Error success = 0;
    static Error record(Event, Stream s) {
        calls.push_back(std::string("record ") + s);
        if (fail_records > 0) return --fail_records, 7;
        return success;
    }
    static Error stream_wait(Stream s, Event) { return calls.push_back(std::string("wait ") + s), success; }
    static Error event_sync(Event) { return calls.push_back("event_sync"), success; }
    static Error device_sync() { return calls.push_back("device_sync"), success; }
    static Error event_create(Event* ev) { return *ev = 1, success; }
    static Error event_destroy(Event) { return success; }
    static Error alloc(void** p, size_t bytes) {
        calls.push_back("alloc " + std::to_string(bytes));
        if (fail_alloc) return 2;
        *p = std::malloc(bytes);
        ++live_blocks;
        return success;
    }
    static Error free(void* p) {
        if (p) calls.push_back("free"), --live_blocks;
        std::free(p);
        return success;
    }
};
using Order = lmpc_order::Order<FakeApi>;
const char S = 'S', A = 'A', B = 'B', C = 'C';

int failures = 0;
// the calls since the last expect()
void expect(const char* what, std::vector<std::string> want) {
    if (calls != want) {
        ++failures;
        std::printf("FAIL %s: got [", what);
        for (const auto& c : calls) std::printf(" %s;", c.c_str());
        std::printf(" ] want [");
        for (const auto& c : want) std::printf(" %s;", c.c_str());
        std::printf(" ]\n");
    }
    calls.clear();
}
void check(const char* what, bool ok) {
    if (!ok) ++failures, std::printf("FAIL %s\n", what);
}
Order fresh() {
    Order o;
    check("create", o.create() == 0 && o.ev == 1);
    return o;
}

}  // namespace

int main() {
    {  // back-to-back launches on one stream: no call at all (the 1.7 us of round 6)
        Order o = fresh();
        for (int i = 0; i < 300; ++i) {
            check("enter A", o.enter(A) == 0);
            o.leave(A);
        }
        expect("one stream", {});
    }
    {  // the stream changes: one record on the old stream, one wait of the new one
        Order o = fresh();
        o.leave(A);
        check("enter B", o.enter(B) == 0);
        expect("A then B", {"record A", "wait B"});
        o.leave(B);
        check("enter B again", o.enter(B) == 0);
        expect("B then B", {});
        o.leave(B);
        check("enter A", o.enter(A) == 0);
        expect("B then A", {"record B", "wait A"});
    }
    {  // two enters without a leave between: the second waits for the event already recorded and records nothing
        Order o = fresh();
        o.leave(A);
        check("enter B", o.enter(B) == 0);
        expect("A then B", {"record A", "wait B"});
        check("enter C", o.enter(C) == 0);
        expect("then C", {"wait C"});
        check("enter A", o.enter(A) == 0);  // the event's own stream
        expect("then A", {});
    }
    {  // the host waits for a launch noted on a caller's stream: the device, once, and no event call
        Order o = fresh();
        o.leave(A);
        check("wait_host", o.wait_host(S) == 0);
        expect("leave A, wait_host S", {"device_sync"});
        check("wait_host again", o.wait_host(S) == 0);
        expect("second wait_host", {});
    }
    {  // an event recorded on A, the last launch on S: the host waits for the event
        Order o = fresh();
        o.leave(A);
        check("enter S", o.enter(S) == 0);
        expect("A then S", {"record A", "wait S"});
        o.leave(S);
        check("wait_host", o.wait_host(S) == 0);
        expect("record on A, leave S, wait_host S", {"event_sync"});
    }
    {  // without that record: nothing
        Order o = fresh();
        o.leave(S);
        check("wait_host", o.wait_host(S) == 0);
        expect("leave S, wait_host S", {});
    }
    {  // the device synchronise leaves nothing outstanding: the event is no longer waited for
        Order o = fresh();
        o.leave(A);
        check("enter B", o.enter(B) == 0);
        o.leave(B);
        expect("A then B", {"record A", "wait B"});
        check("wait_host", o.wait_host(S) == 0);
        expect("wait_host S", {"device_sync"});
        check("enter C", o.enter(C) == 0);
        check("wait_host", o.wait_host(S) == 0);
        expect("after the device synchronise", {});
    }
    {  // a failing record is the call's error and leaves the event off; the next noted launch is recorded again
        Order o = fresh();
        o.leave(A);
        fail_records = 1;
        check("enter B fails", o.enter(B) == 7 && !o.ev_live);
        expect("failing record", {"record A"});
        check("enter C", o.enter(C) == 0 && !o.ev_live);
        expect("no event to wait for", {});
        o.leave(A);
        check("enter B", o.enter(B) == 0 && o.ev_live);
        expect("recorded again", {"record A", "wait B"});
        o.destroy();
        check("destroy", o.ev == 0);
    }
    {  // the grown buffer
        lmpc_order::Grown<FakeApi, double> g;
        check("grow 0", g.grow(0) == LMPC_OK && !g.p && g.cap == 0);
        expect("nothing to allocate", {});
        check("grow 10", g.grow(10) == LMPC_OK && g.p && g.cap == 10);
        expect("first block: nobody to wait for", {"alloc 80"});
        g.p[9] = 1.0;
        check("grow 4", g.grow(4) == LMPC_OK && g.cap == 10);
        expect("never shrunk", {});
        check("grow 12", g.grow(12) == LMPC_OK && g.cap == 12);
        expect("old block freed after the device", {"device_sync", "free", "alloc 96"});
        g.p[11] = 1.0;
        fail_alloc = true;
        check("failed allocation", g.grow(13) == LMPC_ERR_ALLOC && !g.p && g.cap == 0);
        expect("failed allocation", {"device_sync", "free", "alloc 104"});
        fail_alloc = false;
        check("grow after a failure", g.grow(3) == LMPC_OK && g.cap == 3);
        expect("empty: nobody to wait for", {"alloc 24"});
        g.release();
        check("release", !g.p && g.cap == 0 && live_blocks == 0);
        g.release();
        expect("release", {"free"});
    }
    if (failures) return std::printf("order_host_check: %d failures\n", failures), 1;
    std::printf("order_host_check ok\n");
    return 0;
}
