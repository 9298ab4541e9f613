// lmpc_quad_device.h -- the device helpers of the kernels that give a robot one quad of lanes, lane l owning leg l
// (lmpc_rbd.hip, lmpc_sim.hip, lmpc_contact.hip, lmpc_lowsim.hip): the launch layout they share, and the device
// helpers -- values travel between the four lanes by __shfl with width 4, what all four hold identically is stored a
// quarter per lane, and each lane works on its own leg of the model in slot 0.  The arithmetic is lmpc_rbd_common.h's
// and lmpc_sim_common.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "lmpc_sim_common.h"

namespace lmpc_sim {
// One wavefront per block: 4096 robots are 256 wavefronts, which 64-thread blocks spread over 256 CUs and 256-thread
// blocks over 64 (measured on lmpc_rbd_kernel, alternating runs: 16.9 us at 64 threads, 18.8 at 128, 22.9 at 256;
// DESIGN.md 4e).  Lane 4 r + l of a block owns leg l of the block's r-th robot.
constexpr int BLOCK = 64;
constexpr int BLOCK_ROBOTS = BLOCK / 4;  // one quad of lanes per robot
inline dim3 quad_grid(int batch) { return dim3((unsigned)((batch + BLOCK_ROBOTS - 1) / BLOCK_ROBOTS)); }

#if defined(__HIPCC__)
__device__ inline double quad_get(double v, int l) { return __shfl(v, l, 4); }
__device__ inline V3 quad_get(const V3& v, int l) { return V3{quad_get(v.x, l), quad_get(v.y, l), quad_get(v.z, l)}; }
__device__ inline Part quad_get(const Part& p, int l) {
    return Part{quad_get(p.m, l), quad_get(p.mc, l),
                Sym3{quad_get(p.Io.xx, l), quad_get(p.Io.xy, l), quad_get(p.Io.xz, l), quad_get(p.Io.yy, l),
                     quad_get(p.Io.yz, l), quad_get(p.Io.zz, l)},
                quad_get(p.F, l), quad_get(p.N, l)};
}
__device__ inline bool quad_get_flag(bool b, int l) { return __shfl(b ? 1 : 0, l, 4) != 0; }
// b <- src where take
__device__ inline void blk_pick(Blk& b, bool take, const Blk& src) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) b.a[i][j] = take ? src.a[i][j] : b.a[i][j];
}
__device__ inline bool quad_any(bool b) {
    const int v = b ? 1 : 0;
    return (__shfl(v, 0, 4) | __shfl(v, 1, 4) | __shfl(v, 2, 4) | __shfl(v, 3, 4)) != 0;
}
__device__ inline double pick4(const double* v, int i, int n, int l) {
    const double a = v[i], b = v[i + 1 < n ? i + 1 : i], c = v[i + 2 < n ? i + 2 : i], d = v[i + 3 < n ? i + 3 : i];
    return l == 0 ? a : l == 1 ? b : l == 2 ? c : d;
}
// v[0..N) is held identically by the four lanes of a quad: lane l stores the entries l, l + 4, ...
template <int N>
__device__ inline void quad_store(double* dst, const double* v, int l, bool active) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const double pick = pick4(v, i, N, l);
        if (active && i + l < N) dst[i + l] = pick;
    }
}

// The lane's leg of the model in slot 0 (trunk and gravity as they are).
__device__ inline void lane_model(const lmpc_rbd_model& md, int L, lmpc_rbd_model& lm) {
    lm.gravity = md.gravity;
    lm.mass[0] = md.mass[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) lm.com[0][i] = md.com[0][i];
#pragma unroll
    for (int i = 0; i < 6; ++i) lm.inertia[0][i] = md.inertia[0][i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = 3 * L + k;
        lm.mass[1 + k] = md.mass[1 + j];
#pragma unroll
        for (int i = 0; i < 3; ++i) lm.com[1 + k][i] = md.com[1 + j][i], lm.joint_origin[k][i] = md.joint_origin[j][i];
#pragma unroll
        for (int i = 0; i < 6; ++i) lm.inertia[1 + k][i] = md.inertia[1 + j][i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) lm.foot[0][i] = md.foot[L][i];
}
#endif
}  // namespace lmpc_sim
