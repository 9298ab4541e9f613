// lmpc_launch.h -- the host side of every launch: which device a call runs on, whether a caller's stream belongs to it,
// a launch error as a status, and lmpc_order.h's cross-stream ordering and grown buffers over HIP.  Used by the two
// context files (lmpc_capi.cpp, hoqp_capi.cpp) and by the entry points that take no context (lmpc_lowlevel.hip,
// lmpc_lowsim.hip, lmpc_stack.hip, lmpc_est.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lmpc/lmpc.h"
#include "lmpc_order.h"

namespace lmpc_launch {

// An entry point runs on device `dev` and leaves the caller's current device as it found it.
struct DeviceScope {
    int prev = -1, dev;
    bool ok = false;
    explicit DeviceScope(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) {
            prev = -1;
            return;
        }
        ok = dev == prev || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// A caller's stream must belong to the device the call runs on (the null stream is the current device's).
inline bool stream_ok(hipStream_t s, int dev) {
    if (!s) return true;
    hipDevice_t d = -1;
    return hipStreamGetDevice(s, &d) == hipSuccess && d == dev;
}

// The device a device pointer lives on, or -1.
inline int pointer_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return a.device;
}

// Launch context: the device of `anchor` (a device buffer of the call), the caller's current device restored on
// return; a non-NULL stream must belong to that device.
struct PtrScope {
    int prev = -1, dev = -1;
    bool ok = false;
    PtrScope(const void* anchor, hipStream_t s) {
        if (hipGetDevice(&prev) != hipSuccess) {
            prev = -1;
            return;
        }
        dev = pointer_device(anchor);
        if (dev < 0) dev = prev;
        if (!stream_ok(s, dev)) return;
        ok = dev == prev || hipSetDevice(dev) == hipSuccess;
    }
    ~PtrScope() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

inline int launch_rc(hipError_t e) {
    if (e == hipErrorInvalidDeviceFunction || e == hipErrorNoBinaryForGpu) return LMPC_ERR_NOT_BUILT;
    return e == hipSuccess ? LMPC_OK : LMPC_ERR_LAUNCH;
}

struct HipApi {
    using Error = hipError_t;
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    static constexpr Error success = hipSuccess;
    static Error record(Event ev, Stream s) { return hipEventRecord(ev, s); }
    static Error stream_wait(Stream s, Event ev) { return hipStreamWaitEvent(s, ev, 0); }
    static Error event_sync(Event ev) { return hipEventSynchronize(ev); }
    static Error device_sync() { return hipDeviceSynchronize(); }
    static Error event_create(Event* ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming); }
    static Error event_destroy(Event ev) { return hipEventDestroy(ev); }
    static Error alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static Error free(void* p) { return hipFree(p); }
};
using Order = lmpc_order::Order<HipApi>;
template <class T>
using DeviceBuffer = lmpc_order::Grown<HipApi, T>;

}  // namespace lmpc_launch
