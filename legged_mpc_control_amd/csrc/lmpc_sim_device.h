// lmpc_sim_device.h -- one substep of the rigid-body plant for the lane that owns one leg of a quad's robot, as device
// functions.  The step is written once for both plants: lane_terms() (everything up to K, which no contact set enters),
// lane_back() (the back-substitution) and lane_advance() (the state after the step and what the step reports) are the
// halves around the contact solve.  substep() puts the default plant's unilateral rule between them (lmpc_sim.hip's
// kernel and the fused controller + plant kernel of lmpc_lowsim.hip run it through step_lane()); lmpc_contact.hip's
// step kernel puts the friction-pyramid problem there.  The lane's loads and stores that all three kernels share are
// here too: load_lane_state(), store_state(), store_out().  Device code only; the arithmetic is lmpc_rbd_common.h's and
// lmpc_sim_common.h's, the quad exchanges are lmpc_quad_device.h's.  Every lane of the wavefront must call these
// together: they shuffle within quads, and substep()'s unilateral loop leaves on a wavefront vote.
#pragma once
#include <hip/hip_runtime.h>

#include "lmpc/lmpc_sim.h"
#include "lmpc_sim_common.h"
#include "lmpc_quad_device.h"

namespace lmpc_sim {
#if defined(__HIPCC__)
// by components: a ?: on the structs themselves selects between their addresses, which puts them into scratch
__device__ inline V3 pick(bool take, const V3& a, const V3& b) { return V3{take ? a.x : b.x, take ? a.y : b.y, take ? a.z : b.z}; }

// The lane's private state: the base's state, and the lane's own joints in slot 0.
__device__ __forceinline__ void load_lane_state(const lmpc_rbd_state& st, int L, lmpc_rbd_state& ls) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ls.euler[i] = st.euler[i], ls.pos[i] = st.pos[i], ls.omega[i] = st.omega[i], ls.lin_vel[i] = st.lin_vel[i];
        ls.joint_pos[i] = st.joint_pos[3 * L + i], ls.joint_vel[i] = st.joint_vel[3 * L + i];
    }
}
// the same fields from one private state to another
__device__ __forceinline__ void copy_lane_state(lmpc_rbd_state& dst, const lmpc_rbd_state& src) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dst.euler[i] = src.euler[i], dst.pos[i] = src.pos[i], dst.omega[i] = src.omega[i], dst.lin_vel[i] = src.lin_vel[i];
        dst.joint_pos[i] = src.joint_pos[i], dst.joint_vel[i] = src.joint_vel[i];
    }
}

// What lane_terms() leaves of lane L's leg for the contact solve and for lane_back() / lane_advance().
struct LaneTerms {
    BaseKin bk;
    LegOut g;
    V3 rl;
    LegRed rd;
    Chol6 Ls;
    double yb[6];
    LegRows w;
    Blk K[4];  // K[k] = K_Lk, the whole block row (the default plant uses k <= L)
    bool bad;  // a non-positive pivot so far
};

// Steps 1-3 of lmpc_sim_common.h for lane L's leg: nothing here depends on the contact set.  `md` is the kernel's
// argument; `ls` is the lane's private state and is only read.  s = dt (STEP) or 1.
template <bool STEP>
__device__ __forceinline__ void lane_terms(const lmpc_rbd_model& md, int L, const lmpc_rbd_state& ls, const double (&tau3)[3],
                                           double s, LaneTerms& t) {
    // The leg's 42 doubles of the model are loaded anew in every substep: the empty asm makes the index opaque, so
    // the loads cannot be hoisted out of the caller's loop, where they held 84 registers through the solve and spilled.
    int Ll = L;
    asm volatile("" : "+v"(Ll));
    lmpc_rbd_model lm;
    lane_model(md, Ll, lm);
    t.bk = base_kin(ls);
    leg_pass(lm, ls, t.bk, 0, t.g);
    BaseOut base;
    base_pass(t.bk, total_part(trunk_part(lm, t.bk), quad_get(t.g.sum, 0), quad_get(t.g.sum, 1), quad_get(t.g.sum, 2),
                               quad_get(t.g.sum, 3)), base);
    V3 c;
    leg_rhs(t.g, tau3, s, STEP, t.rl, c);
    leg_reduce(t.g, t.rl, c, t.rd);
    t.bad = !t.rd.okm;
    double e[NC + 6];
    base_entries(base, s, e);
#pragma unroll
    for (int n = 0; n < NC + 6; ++n)
        e[n] = minus4(e[n], quad_get(t.rd.Cs[n], 0), quad_get(t.rd.Cs[n], 1), quad_get(t.rd.Cs[n], 2), quad_get(t.rd.Cs[n], 3));
    t.bad = !base_factor(e, t.Ls, t.yb) || t.bad;
    leg_rows(t.rd, t.Ls, t.yb, t.w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double Zk[3][6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) Zk[i][j] = quad_get(t.w.Z[i][j], k);
        blk_of(t.w.Z, Zk, t.rd.A, L == k, t.K[k]);
    }
}

// Step 5 for the lane's multiplier P of either plant's contact solve: xb (the same bits in the four lanes) and the
// leg's xl.  Returns `bad`, or that one of xb, xl, P is not finite.  The flag goes through the function, the checks
// or-ed onto it one by one, and is not or-ed with the function's result by the caller: that other order of the same
// chain cost the fused contact kernel 9 more spilled VGPRs and the back-substituting one 12 more registers.
__device__ __forceinline__ bool lane_back(const LaneTerms& t, const V3& P, bool bad, double (&xb)[6], V3& xl) {
    double zp[6], t6[6];
    leg_zp(t.w, P, zp);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        t6[i] = plus4(t.yb[i], quad_get(zp[i], 0), quad_get(zp[i], 1), quad_get(zp[i], 2), quad_get(zp[i], 3));
    base_back(t.Ls, t6, xb);
    xl = leg_back(t.g, t.rd, t.rl, xb, P);
#pragma unroll
    for (int i = 0; i < 6; ++i) bad = bad || !finite(xb[i]);
    return bad || !finite(xl) || !finite(P);
}

// What a substep reports, nothing of which is carried to the next substep: the base's and the leg's accelerations, the
// foot's force, position and velocity.  A failed robot reports zeros.
struct LaneOut {
    double q[6];
    V3 qdd, force, foot_pos, foot_vel;
};
__device__ __forceinline__ void zero_lane_out(LaneOut& o) {
#pragma unroll
    for (int i = 0; i < 6; ++i) o.q[i] = 0.0;
    o.qdd = v3(0.0, 0.0, 0.0), o.force = o.qdd, o.foot_pos = o.qdd, o.foot_vel = o.qdd;
}

// The step taken (a robot that has not failed): the state after it into `next`, of which only the fields of
// load_lane_state() are written, and its report into `o`.  `next` may be `ls` itself: `ls` is read before `next` is
// written.
__device__ __forceinline__ void lane_advance(const LaneTerms& t, const lmpc_rbd_state& ls, const double (&xb)[6], const V3& xl,
                                             const V3& P, double dt, lmpc_rbd_state& next, LaneOut& o) {
    const V3 pos = v3(ls.pos[0], ls.pos[1], ls.pos[2]);
    BaseNext bn;
    base_advance(t.bk, v3(ls.euler[0], ls.euler[1], ls.euler[2]), pos, xb, dt, bn);
    LegNext ln;
    leg_advance(t.g, v3(ls.joint_pos[0], ls.joint_pos[1], ls.joint_pos[2]),
                v3(ls.joint_vel[0], ls.joint_vel[1], ls.joint_vel[2]), xl, P, dt, bn, pos, ln);
    next.euler[0] = bn.euler.x, next.euler[1] = bn.euler.y, next.euler[2] = bn.euler.z;
    next.pos[0] = bn.pos.x, next.pos[1] = bn.pos.y, next.pos[2] = bn.pos.z;
    next.omega[0] = bn.omega.x, next.omega[1] = bn.omega.y, next.omega[2] = bn.omega.z;
    next.lin_vel[0] = bn.vlin.x, next.lin_vel[1] = bn.vlin.y, next.lin_vel[2] = bn.vlin.z;
    next.joint_pos[0] = ln.jp.x, next.joint_pos[1] = ln.jp.y, next.joint_pos[2] = ln.jp.z;
    next.joint_vel[0] = ln.jv.x, next.joint_vel[1] = ln.jv.y, next.joint_vel[2] = ln.jv.z;
#pragma unroll
    for (int i = 0; i < 6; ++i) o.q[i] = bn.qdd[i];
    o.qdd = ln.qdd, o.force = ln.force, o.foot_pos = ln.foot_pos, o.foot_vel = ln.foot_vel;
}

// One substep of lane L's leg under the default plant's unilateral rule.  `ls` is only read.  `next` must hold a copy
// of `ls` on entry and holds the state after the substep on return: advanced when STEP and the robot has not failed,
// else left as it was (STEP = false, the forward dynamics, never touches it; dt and ground_z are unused there).  The
// caller then copies `next` back over `ls` unconditionally (step_lane() below).  This shape is deliberate: advancing
// `ls` in place under `!failed` through the reference made the compiler carry the state twice around the caller's
// substep loop (36 more registers, 20 VGPRs spilled).  `failed` is quad-uniform and, once set, freezes the state.
// Returned: the substep's report, whether the foot was held, its touch flag.
template <bool STEP>
__device__ __forceinline__ void substep(const lmpc_rbd_model& md, int L, const lmpc_rbd_state& ls, lmpc_rbd_state& next, const double (&tau3)[3],
                                        bool candidate, double dt, double ground_z, int unilateral, LaneOut& o, bool& held,
                                        int& otouch, bool& failed) {
    LaneTerms t;
    lane_terms<STEP>(md, L, ls, tau3, STEP ? dt : 1.0, t);
    bool bad = t.bad;

    // 4: the block Cholesky of lmpc_sim_common.h's solve_contacts(), lane L owning block row L.  Every lane runs
    // every phase; what a lane computes for blocks it does not own is never read.
    held = candidate;
    V3 P = v3(0.0, 0.0, 0.0);
    for (int pass = 0; pass < 4; ++pass) {
        Blk B[4], Dg;  // B[k] = K_Lk for k < L, Dg = K_LL
        blk_mask(t.K[0], false, true, Dg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hk = quad_get_flag(held, k);
            blk_mask(t.K[k], held && hk, false, B[k]);
            Blk d;
            blk_mask(t.K[k], held, true, d);
            blk_pick(Dg, L == k, d);
        }
        const V3 floor = blk_floor(Dg);
        Chol3 Ld;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = chol3(Dg.a, floor, Ld);
            bad = bad || !quad_get_flag(ok, k);
            const Chol3 Lkk{quad_get(Ld.l00, k), quad_get(Ld.l10, k), quad_get(Ld.l11, k),
                            quad_get(Ld.l20, k), quad_get(Ld.l21, k), quad_get(Ld.l22, k)};
            blk_trsm(B[k], Lkk);
#pragma unroll
            for (int j = k + 1; j < 4; ++j) {
                Blk Ljk, X = B[j];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int q = 0; q < 3; ++q) Ljk.a[i][q] = quad_get(B[k].a[i][q], j);
                blk_pick(X, L == j, Dg);
                blk_update(X, B[k], Ljk);
                blk_pick(Dg, L == j, X);
                blk_pick(B[j], L != j, X);
            }
        }
        V3 y = pick(held, t.w.rhs, v3(0.0, 0.0, 0.0));
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // L y = rhs
            const V3 yl = chol3_fwd(Ld, y);
            const V3 yk = quad_get(yl, k);
            const V3 lower = sub(y, mul3(B[k].a, yk));
            y = pick(L == k, yl, pick(L > k, lower, y));
        }
#pragma unroll
        for (int k = 3; k >= 0; --k) {  // L' P = y
            const V3 u = mul3t(B[k].a, P);
            V3 a = y;
#pragma unroll
            for (int m = k + 1; m < 4; ++m) a = sub(a, quad_get(u, m));
            const V3 Pk = chol3_bwd(Ld, a);
            P = pick(L == k, Pk, P);
        }
        P = pick(held, P, v3(0.0, 0.0, 0.0));
        // a quad whose set did not change solves the same system again, to the same bits: the loop's exit can
        // be wavefront-uniform without touching any robot's result
        const bool release = unilateral != 0 && held && P.z < 0.0;
        held = held && !release;
        if (!__any(release)) break;
    }
    // a fourth pass that still released a foot has emptied the quad's set: every P is 0, no further solve
    P = pick(held, P, v3(0.0, 0.0, 0.0));
    // 5
    double xb[6];
    V3 xl;
    bad = lane_back(t, P, bad, xb, xl);
    failed = failed || quad_any(bad);
    zero_lane_out(o);
    otouch = 0;
    if (!STEP) {
        if (!failed) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o.q[i] = xb[i];
            o.qdd = xl, o.force = P, o.foot_vel = t.g.foot_vel;
            o.foot_pos = add(v3(ls.pos[0], ls.pos[1], ls.pos[2]), t.g.foot);
        }
    } else if (!failed) {
        lane_advance(t, ls, xb, xl, P, dt, next, o);
        otouch = o.foot_pos.z <= ground_z ? 1 : 0;
    }
}

// substep() on the state the lane carries through its loop: a copy in and, unconditionally, a copy out (the comment
// above substep() has the reason).  The forward dynamics has no state after it.
template <bool STEP>
__device__ __forceinline__ void step_lane(const lmpc_rbd_model& md, int L, lmpc_rbd_state& ls, const double (&tau3)[3], bool candidate,
                                          double dt, double ground_z, int unilateral, LaneOut& o, bool& held, int& otouch,
                                          bool& failed) {
    lmpc_rbd_state nx;
    if (STEP) copy_lane_state(nx, ls);
    substep<STEP>(md, L, ls, nx, tau3, candidate, dt, ground_z, unilateral, o, held, otouch, failed);
    if (STEP) copy_lane_state(ls, nx);
}

// The lane's private state into robot state `n`: the base, which the four lanes hold identically, a quarter per lane,
// and the lane's own joints (slot 0 of `ls`).
__device__ __forceinline__ void store_state(lmpc_rbd_state& n, const lmpc_rbd_state& ls, int L, bool active) {
    const double q6[6] = {ls.euler[0], ls.euler[1], ls.euler[2], ls.pos[0], ls.pos[1], ls.pos[2]};
    const double v6[6] = {ls.omega[0], ls.omega[1], ls.omega[2], ls.lin_vel[0], ls.lin_vel[1], ls.lin_vel[2]};
    double* nd = reinterpret_cast<double*>(&n);  // 36 doubles: euler, pos, joint_pos, omega, lin_vel, joint_vel
    quad_store<6>(nd, q6, L, active);
    quad_store<6>(nd + 18, v6, L, active);
    if (active) {
#pragma unroll
        for (int i = 0; i < 3; ++i) n.joint_pos[3 * L + i] = ls.joint_pos[i], n.joint_vel[3 * L + i] = ls.joint_vel[i];
    }
}

// Lane L's part of lmpc_sim_out from what its last substep reported (`held` already cleared for a failed robot);
// `status` is the robot's, quad-uniform.
__device__ __forceinline__ void store_out(lmpc_sim_out& o, const LaneOut& s, int held, int touch, int status, int L, bool active) {
    quad_store<6>(o.qdd, s.q, L, active);
    if (active) {
        o.qdd[6 + 3 * L] = s.qdd.x, o.qdd[7 + 3 * L] = s.qdd.y, o.qdd[8 + 3 * L] = s.qdd.z;
        o.force[3 * L] = s.force.x, o.force[3 * L + 1] = s.force.y, o.force[3 * L + 2] = s.force.z;
        o.foot_pos[3 * L] = s.foot_pos.x, o.foot_pos[3 * L + 1] = s.foot_pos.y, o.foot_pos[3 * L + 2] = s.foot_pos.z;
        o.foot_vel[3 * L] = s.foot_vel.x, o.foot_vel[3 * L + 1] = s.foot_vel.y, o.foot_vel[3 * L + 2] = s.foot_vel.z;
        o.held[L] = held;
        o.touch[L] = touch;
        if (L == 0) o.status = status;
        if (L == 1) o.reserved = 0;
    }
}
#endif
}  // namespace lmpc_sim
