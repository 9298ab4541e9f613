// lmpc_sim_device.h -- one substep of the rigid-body plant for the lane that owns one leg of a quad's robot, as a
// device function: the body of lmpc_sim.hip's substep loop, shared with the fused controller + plant kernel
// (lmpc_lowsim.hip).  Device code only; the arithmetic is lmpc_rbd_common.h's and lmpc_sim_common.h's, the quad
// exchanges are lmpc_quad_device.h's.  Every lane of the wavefront must call it together: it shuffles within quads
// and its unilateral loop leaves on a wavefront vote.
#pragma once
#include <hip/hip_runtime.h>

#include "lmpc/lmpc_sim.h"
#include "lmpc_sim_common.h"
#include "lmpc_quad_device.h"

namespace lmpc_sim {
#if defined(__HIPCC__)
// by components: a ?: on the structs themselves selects between their addresses, which puts them into scratch
__device__ inline V3 pick(bool take, const V3& a, const V3& b) { return V3{take ? a.x : b.x, take ? a.y : b.y, take ? a.z : b.z}; }

// One substep of lane L's leg.  `md` is the kernel's argument; `ls` is the lane's private state (the base, and the lane's
// own joints in slot 0) and is only read.  `next` must hold a copy of `ls` on entry and holds the state after the
// substep on return: advanced when STEP and the robot has not failed, else left as it was (STEP = false, the forward
// dynamics, never touches it; dt and ground_z are unused there).  The caller then copies `next` back over `ls`
// unconditionally.  This shape is deliberate: advancing `ls` in place under `!failed` through the reference made the
// compiler carry the state twice around the caller's substep loop (36 more registers, 20 VGPRs spilled).  `failed` is
// quad-uniform and, once set, freezes the state.
// Returned: what the substep reports (a failed robot: zeros), nothing of which is carried to the next substep -- the
// base's and the leg's accelerations, the foot's force, position and velocity, whether the foot was held, its touch
// flag.
template <bool STEP>
__device__ __forceinline__ void substep(const lmpc_rbd_model& md, int L, const lmpc_rbd_state& ls, lmpc_rbd_state& next, const double (&tau3)[3],
                                        bool candidate, double dt, double ground_z, int unilateral, double (&oq)[6],
                                        V3& oqdd, V3& oforce, V3& ofp, V3& ofv, bool& held, int& otouch, bool& failed) {
    const double s = STEP ? dt : 1.0;
    // The leg's 42 doubles of the model are loaded anew in every substep: the empty asm makes the index opaque, so
    // the loads cannot be hoisted out of the caller's loop, where they held 84 registers through the solve and spilled.
    int Ll = L;
    asm volatile("" : "+v"(Ll));
    lmpc_rbd_model lm;
    lane_model(md, Ll, lm);
    const BaseKin bk = base_kin(ls);
    LegOut g;
    leg_pass(lm, ls, bk, 0, g);
    BaseOut base;
    base_pass(bk, total_part(trunk_part(lm, bk), quad_get(g.sum, 0), quad_get(g.sum, 1), quad_get(g.sum, 2),
                             quad_get(g.sum, 3)), base);
    V3 rl, c;
    leg_rhs(g, tau3, s, STEP, rl, c);
    // 1-3: nothing here depends on the contact set
    LegRed rd;
    leg_reduce(g, rl, c, rd);
    bool bad = !rd.okm;
    double e[NC + 6], yb[6];
    base_entries(base, s, e);
#pragma unroll
    for (int n = 0; n < NC + 6; ++n)
        e[n] = minus4(e[n], quad_get(rd.Cs[n], 0), quad_get(rd.Cs[n], 1), quad_get(rd.Cs[n], 2), quad_get(rd.Cs[n], 3));
    Chol6 Ls;
    bad = !base_factor(e, Ls, yb) || bad;
    LegRows w;
    leg_rows(rd, Ls, yb, w);
    Blk K[4];  // K[k] = K_Lk; only k <= L is used
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double Zk[3][6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) Zk[i][j] = quad_get(w.Z[i][j], k);
        blk_of(w.Z, Zk, rd.A, L == k, K[k]);
    }

    // 4: the block Cholesky of lmpc_sim_common.h's solve_contacts(), lane L owning block row L.  Every lane runs
    // every phase; what a lane computes for blocks it does not own is never read.
    held = candidate;
    V3 P = v3(0.0, 0.0, 0.0);
    for (int pass = 0; pass < 4; ++pass) {
        Blk B[4], Dg;  // B[k] = K_Lk for k < L, Dg = K_LL
        blk_mask(K[0], false, true, Dg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hk = quad_get_flag(held, k);
            blk_mask(K[k], held && hk, false, B[k]);
            Blk d;
            blk_mask(K[k], held, true, d);
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
        V3 t = pick(held, w.rhs, v3(0.0, 0.0, 0.0));
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // L y = t
            const V3 y = chol3_fwd(Ld, t);
            const V3 yk = quad_get(y, k);
            const V3 lower = sub(t, mul3(B[k].a, yk));
            t = pick(L == k, y, pick(L > k, lower, t));
        }
#pragma unroll
        for (int k = 3; k >= 0; --k) {  // L' P = y
            const V3 u = mul3t(B[k].a, P);
            V3 a = t;
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
    double zp[6], t6[6], xb[6];
    leg_zp(w, P, zp);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        t6[i] = plus4(yb[i], quad_get(zp[i], 0), quad_get(zp[i], 1), quad_get(zp[i], 2), quad_get(zp[i], 3));
    base_back(Ls, t6, xb);
    const V3 xl = leg_back(g, rd, rl, xb, P);
#pragma unroll
    for (int i = 0; i < 6; ++i) bad = bad || !finite(xb[i]);
    bad = bad || !finite(xl) || !finite(P);
    failed = failed || quad_any(bad);
    // what this substep reports (a failed robot: zeros)
#pragma unroll
    for (int i = 0; i < 6; ++i) oq[i] = 0.0;
    oqdd = v3(0.0, 0.0, 0.0), oforce = oqdd, ofp = oqdd, ofv = oqdd;
    otouch = 0;
    if (!STEP) {
        if (!failed) {
#pragma unroll
            for (int i = 0; i < 6; ++i) oq[i] = xb[i];
            oqdd = xl, oforce = P, ofv = g.foot_vel;
            ofp = add(v3(ls.pos[0], ls.pos[1], ls.pos[2]), g.foot);
        }
    } else if (!failed) {
        const V3 pos = v3(ls.pos[0], ls.pos[1], ls.pos[2]);
        BaseNext bn;
        base_advance(bk, v3(ls.euler[0], ls.euler[1], ls.euler[2]), pos, xb, dt, bn);
        LegNext ln;
        leg_advance(g, v3(ls.joint_pos[0], ls.joint_pos[1], ls.joint_pos[2]),
                    v3(ls.joint_vel[0], ls.joint_vel[1], ls.joint_vel[2]), xl, P, dt, bn, pos, ln);
        next.euler[0] = bn.euler.x, next.euler[1] = bn.euler.y, next.euler[2] = bn.euler.z;
        next.pos[0] = bn.pos.x, next.pos[1] = bn.pos.y, next.pos[2] = bn.pos.z;
        next.omega[0] = bn.omega.x, next.omega[1] = bn.omega.y, next.omega[2] = bn.omega.z;
        next.lin_vel[0] = bn.vlin.x, next.lin_vel[1] = bn.vlin.y, next.lin_vel[2] = bn.vlin.z;
        next.joint_pos[0] = ln.jp.x, next.joint_pos[1] = ln.jp.y, next.joint_pos[2] = ln.jp.z;
        next.joint_vel[0] = ln.jv.x, next.joint_vel[1] = ln.jv.y, next.joint_vel[2] = ln.jv.z;
#pragma unroll
        for (int i = 0; i < 6; ++i) oq[i] = bn.qdd[i];
        oqdd = ln.qdd, oforce = ln.force, ofp = ln.foot_pos, ofv = ln.foot_vel;
        otouch = ln.foot_pos.z <= ground_z ? 1 : 0;
    }
}

// The lane's private state into robot state `n`: the base, which the four lanes hold identically, a quarter per lane,
// and the lane's own joints (slot 0 of `ls`).  Shared by lmpc_sim_kernel and lmpc_lowsim_kernel.
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

// Lane L's part of lmpc_sim_out from what its last substep reported (`held` already cleared for a failed robot).
__device__ __forceinline__ void store_out(lmpc_sim_out& o, const double (&oq)[6], const V3& oqdd, const V3& oforce,
                                          const V3& ofp, const V3& ofv, int held, int touch, bool failed, int L,
                                          bool active) {
    quad_store<6>(o.qdd, oq, L, active);
    if (active) {
        o.qdd[6 + 3 * L] = oqdd.x, o.qdd[7 + 3 * L] = oqdd.y, o.qdd[8 + 3 * L] = oqdd.z;
        o.force[3 * L] = oforce.x, o.force[3 * L + 1] = oforce.y, o.force[3 * L + 2] = oforce.z;
        o.foot_pos[3 * L] = ofp.x, o.foot_pos[3 * L + 1] = ofp.y, o.foot_pos[3 * L + 2] = ofp.z;
        o.foot_vel[3 * L] = ofv.x, o.foot_vel[3 * L + 1] = ofv.y, o.foot_vel[3 * L + 2] = ofv.z;
        o.held[L] = held;
        o.touch[L] = touch;
        if (L == 0) o.status = failed ? 1 : 0;
        if (L == 1) o.reserved = 0;
    }
}
#endif
}  // namespace lmpc_sim
