// lmpc_order.h -- what a context (lmpc_capi.cpp, hoqp_capi.cpp) needs around its own device buffers: the order of the
// launches that use them across streams, and a buffer that grows on demand.  No HIP header: both are templates on an
// Api type, lmpc_launch.h instantiates them with HIP's calls and tests/cpp/order_host_check.cpp with a fake that logs.
//
// Api supplies: the types Error, Stream, Event and the value `success`; record(Event, Stream),
// stream_wait(Stream, Event), event_sync(Event), device_sync(); event_create(Event*), event_destroy(Event);
// alloc(void**, bytes), free(void*).
#pragma once
#include <cstddef>

#include "lmpc/lmpc.h"

namespace lmpc_order {

// Launches that use a context's buffers are ordered as issued, whatever stream each comes on.  leave(s) notes the
// launch's stream; enter(s), before a launch on stream s, records the event on a noted launch's stream when s differs
// (everything issued there so far precedes it) and makes s wait for it.  A launch on the noted stream needs nothing:
// stream order already holds, and recording an event after every launch cost config 2 ~3 us per step (1.8 %, round 6,
// profiles/r06/overhead/).  The host waits for the device instead (wait_host): the noted stream may be gone by then.
template <class Api>
struct Order {
    using Error = typename Api::Error;
    using Stream = typename Api::Stream;
    typename Api::Event ev{};
    Stream ev_stream{};    // where ev was last recorded
    bool ev_live = false;  // ev holds a record that nothing on the host has waited for
    Stream last{};         // stream of the last launch that used the buffers, not yet fenced
    bool pend = false;

    Error create() { return Api::event_create(&ev); }
    void destroy() {
        if (ev) (void)Api::event_destroy(ev);
        ev = {};
    }
    Error enter(Stream s) {
        if (pend) {
            if (last == s) return Api::success;
            const Error e = Api::record(ev, last);
            pend = false;
            ev_stream = last;
            ev_live = e == Api::success;
            if (!ev_live) return e;
        }
        if (ev_live && ev_stream != s) return Api::stream_wait(s, ev);
        return Api::success;
    }
    void leave(Stream s) {
        last = s;
        pend = true;
    }
    // Wait on the host for the last launch that used the buffers; s: a stream the caller has synchronised or is about
    // to use itself.  A launch noted on another stream: the device as a whole, after which nothing is outstanding
    // (rare -- a host-pointer call after device-path calls on a caller's stream, a sync, a destroy).
    Error wait_host(Stream s) {
        if (pend && last != s) {
            const Error e = Api::device_sync();
            pend = false;
            if (e == Api::success) ev_live = false;
            return e;
        }
        if (ev_live && ev_stream != s) return Api::event_sync(ev);
        return Api::success;
    }
};

// A device buffer of `cap` elements, grown on demand and never shrunk; contents are not kept.  An old block may still
// be read by queued launches on any stream, so the device is waited for before it is freed.
template <class Api, class T>
struct Grown {
    T* p = nullptr;
    size_t cap = 0;

    int grow(size_t n) {
        if (n <= cap) return LMPC_OK;
        if (p) (void)Api::device_sync();
        release();
        if (Api::alloc((void**)&p, n * sizeof(T)) != Api::success) {
            p = nullptr;
            return LMPC_ERR_ALLOC;
        }
        cap = n;
        return LMPC_OK;
    }
    void release() {
        (void)Api::free(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace lmpc_order
