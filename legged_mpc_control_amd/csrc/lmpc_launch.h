// lmpc_launch.h -- the launch bookkeeping of the robot kernels' entry points that take no MPC context (lmpc_lowlevel.hip,
// lmpc_lowsim.hip, lmpc_stack.hip, lmpc_est.hip): which device a call runs on, and a launch error as a status.  Host
// side of the .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "lmpc/lmpc.h"

namespace lmpc_launch {

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
        if (s) {
            hipDevice_t d = -1;
            if (hipStreamGetDevice(s, &d) != hipSuccess || d != dev) return;
        }
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

}  // namespace lmpc_launch
