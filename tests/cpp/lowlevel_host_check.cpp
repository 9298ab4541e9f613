// lowlevel_host_check.cpp -- a stand-alone program over csrc/lmpc_lowlevel_common.h (no HIP, no liblmpc): it runs the
// low-level controller's host path on a few hundred seeded robots and on the hand cases, so that the shared arithmetic
// can run under the host compiler's sanitizers (-fsanitize=address,undefined; tests/test_lowlevel_host.py builds and
// runs it).  It checks what needs no reference: reachable targets come back without a flag and inv_kin(fk(q), q) = q,
// the velocity solve satisfies J w = v, mode 0 sends the feed-forward torque alone, and the NaN / clamp flags.  The
// robots run twice: on mirror-image legs with one pair of gains, and on a cfg with no two numbers alike (gains, limits,
// rho_opt, lengths), where tau must be built from the leg's own gains and clamped by the joint's own limit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lmpc_lowlevel_common.h"

namespace {

lmpc_lowlevel_cfg toy_cfg(double kp, double kd) {
    lmpc_lowlevel_cfg c{};
    for (int l = 0; l < 4; ++l) {
        const double sx = (l & 2) ? -1.0 : 1.0, sy = (l & 1) ? -1.0 : 1.0;
        const double rf[5] = {0.19 * sx, 0.05 * sy, 0.08 * sy, 0.213, 0.21};
        std::memcpy(c.kin.rho_fix[l], rf, sizeof rf);
        for (int k = 0; k < 3; ++k) c.kp[l][k] = kp, c.kd[l][k] = kd;
    }
    return c;
}

// no two numbers alike: 12 gains of each kind, three limits, a rho_opt and 20 lengths (tests/model_sets.py's "skew_limited"
// in spirit; rho_opt[l][1] has the sign of the leg's d, so that targets made by fk stay inside inv_kin's reach)
lmpc_lowlevel_cfg skew_cfg() {
    lmpc_lowlevel_cfg c{};
    const double rf[4][5] = {{0.168, 0.042, 0.075, 0.187, 0.193},
                             {0.185, -0.048, -0.080, 0.207, 0.213},
                             {-0.202, 0.049, 0.085, 0.231, 0.223},
                             {-0.232, -0.058, -0.091, 0.256, 0.254}};
    const double ro[4][3] = {{0.007, 0.014, -0.011}, {0.010, -0.015, -0.020}, {-0.019, 0.016, 0.017}, {-0.012, -0.009, -0.013}};
    const double kp[4][3] = {{5.8, 9.7, 0.5}, {12.4, 8.4, 13.7}, {1.8, 3.1, 7.1}, {15.0, 4.5, 11.0}};
    const double kd[4][3] = {{0.45, 0.27, 0.49}, {0.56, 0.53, 0.24}, {0.60, 0.35, 0.31}, {0.38, 0.20, 0.42}};
    std::memcpy(c.kin.rho_fix, rf, sizeof rf);
    std::memcpy(c.kin.rho_opt, ro, sizeof ro);
    std::memcpy(c.kp, kp, sizeof kp);
    std::memcpy(c.kd, kd, sizeof kd);
    c.tau_limit[0] = 9.0, c.tau_limit[1] = 14.0, c.tau_limit[2] = 21.0;
    return c;
}

unsigned long long rng_state = 88172645463325252ull;
double uniform(double lo, double hi) {  // xorshift64
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return lo + (hi - lo) * (double)(rng_state >> 11) / 9007199254740992.0;
}

int fail(const char* what, int robot) {
    std::printf("FAIL: %s (robot %d)\n", what, robot);
    return 1;
}

// a robot in a random pose whose foot targets are fk(q + delta) in the world frame
void draw(const lmpc_lowlevel_cfg& cfg, lmpc_rbd_state& st, lmpc_wbc_target& tg) {
    st = lmpc_rbd_state{};
    tg = lmpc_wbc_target{};
    st.euler[0] = uniform(-3.0, 3.0), st.euler[1] = uniform(-0.3, 0.3), st.euler[2] = uniform(-0.3, 0.3);
    st.pos[0] = uniform(-1.0, 1.0), st.pos[1] = uniform(-1.0, 1.0), st.pos[2] = uniform(0.25, 0.35);
    for (int i = 0; i < 3; ++i) st.omega[i] = uniform(-0.5, 0.5), st.lin_vel[i] = uniform(-0.5, 0.5);
    double R[9];
    lmpc_common::euler_zyx_to_rot(st.euler[2], st.euler[1], st.euler[0], R);
    for (int l = 0; l < 4; ++l) {
        double* q = st.joint_pos + 3 * l;
        q[0] = uniform(-0.8, 0.8), q[1] = uniform(-0.6, 2.0), q[2] = uniform(-2.6, -0.9);
        const double qt[3] = {q[0] + uniform(-0.1, 0.1), q[1] + uniform(-0.1, 0.1), q[2] + uniform(-0.1, 0.1)};
        double p[3];
        lmpc_ll::fk(cfg.kin.rho_fix[l], cfg.kin.rho_opt[l], qt, p);
        for (int r = 0; r < 3; ++r) {
            tg.foot_pos_des[3 * l + r] = R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2] + st.pos[r];
            tg.foot_vel_des[3 * l + r] = uniform(-1.0, 1.0);
            tg.forces_des[3 * l + r] = uniform(-150.0, 150.0);
            st.joint_vel[3 * l + r] = uniform(-2.0, 2.0);
        }
    }
}

// `robots` seeded robots on `cfg`: no flag but the clamp's, J w = v, tau = clamp(kp da + kd dw + feed-forward) with the
// leg's own gains and the joint's own limit, mode 0; with rho_opt = 0 also inv_kin(fk(q), q) = q
int run_pool(const lmpc_lowlevel_cfg& cfg, int robots, bool round_trip, double& worst_rt, double& worst_lu, int& clamped,
             int& free) {
    std::vector<lmpc_lowlevel_out> outs(robots);  // on the heap: the sanitizer watches its bounds
    for (int r = 0; r < robots; ++r) {
        lmpc_rbd_state st;
        lmpc_wbc_target tg;
        draw(cfg, st, tg);
        lmpc_lowlevel_out& o = outs[r];
        std::memset(&o, 0xA5, sizeof o);
        lmpc_ll::robot(cfg, st, tg, 1, o);
        double R[9];
        lmpc_common::euler_zyx_to_rot(st.euler[2], st.euler[1], st.euler[0], R);
        for (int l = 0; l < 4; ++l) {
            if ((o.flags[l] & ~LMPC_LL_CLAMPED) != 0) return fail("a reachable target raised a flag", r);
            const double* q = st.joint_pos + 3 * l;
            if (round_trip) {
                double p[3], back[3];
                lmpc_ll::fk(cfg.kin.rho_fix[l], cfg.kin.rho_opt[l], q, p);
                lmpc_ll::inv_kin(cfg.kin.rho_fix[l], p, q, back);
                for (int k = 0; k < 3; ++k) worst_rt = std::fmax(worst_rt, std::fabs(back[k] - q[k]));
            }
            // J w = R' (v_des - v)
            double J[9];
            lmpc_common::foot_jacobian(cfg.kin.rho_fix[l], cfg.kin.rho_opt[l], q, J);
            for (int i = 0; i < 3; ++i) {
                double v = 0.0, Jw = 0.0;
                for (int k = 0; k < 3; ++k) {
                    v += R[3 * k + i] * (tg.foot_vel_des[3 * l + k] - st.lin_vel[k]);
                    Jw += J[3 * i + k] * o.joint_vel_tgt[3 * l + k];
                }
                worst_lu = std::fmax(worst_lu, std::fabs(Jw - v));
            }
            bool any = false;
            for (int k = 0; k < 3; ++k) {
                const int j = 3 * l + k;
                double want = cfg.kp[l][k] * (o.joint_ang_tgt[j] - q[k]) +
                              cfg.kd[l][k] * (o.joint_vel_tgt[j] - st.joint_vel[j]) + o.joint_tau_tgt[j];
                const double lim = cfg.tau_limit[k];
                if (lim > 0.0 && std::fabs(want) > lim) want = want > 0.0 ? lim : -lim, any = true, ++clamped;
                else ++free;
                if (o.tau[j] != want) return fail("tau is not clamp(kp da + kd dw + feed-forward)", r);
            }
            if (any != ((o.flags[l] & LMPC_LL_CLAMPED) != 0)) return fail("the clamp's flag", r);
        }
        // mode 0: the feed-forward torque alone (clamped), the same one
        lmpc_lowlevel_out o0;
        lmpc_ll::robot(cfg, st, tg, 0, o0);
        for (int j = 0; j < 12; ++j) {
            const double lim = cfg.tau_limit[j % 3], ff = o0.joint_tau_tgt[j];
            const double want = lim > 0.0 && std::fabs(ff) > lim ? (ff > 0.0 ? lim : -lim) : ff;
            if (o0.tau[j] != want) return fail("mode 0", r);
        }
        if (std::memcmp(o0.joint_tau_tgt, o.joint_tau_tgt, sizeof o0.tau) != 0 ||
            std::memcmp(o0.joint_ang_tgt, st.joint_pos, sizeof o0.tau) != 0 ||
            std::memcmp(o0.joint_vel_tgt, st.joint_vel, sizeof o0.tau) != 0)
            return fail("mode 0", r);
    }
    return 0;
}

}  // namespace

int main() {
    const lmpc_lowlevel_cfg cfg = toy_cfg(15.0, 0.4);
    const int robots = 300;
    double worst_rt = 0.0, worst_lu = 0.0;
    int clamped = 0, free = 0;
    if (run_pool(cfg, robots, true, worst_rt, worst_lu, clamped, free)) return 1;
    if (clamped != 0) return fail("a clamp without a limit", -1);
    if (run_pool(skew_cfg(), robots, false, worst_rt, worst_lu, clamped, free)) return 1;
    if (clamped == 0 || free == 0) return fail("the three limits never bite, or always", -1);
    if (!(worst_rt <= 1e-9)) return fail("inv_kin(fk(q), q) != q", -1);
    if (!(worst_lu <= 1e-9)) return fail("J w != v", -1);

    // hand cases
    lmpc_rbd_state st;
    lmpc_wbc_target tg;
    draw(cfg, st, tg);
    lmpc_lowlevel_out o;
    {  // FL's target 1 m from its hip: out of reach
        lmpc_wbc_target t = tg;
        t.foot_pos_des[0] += 1.0;
        lmpc_ll::robot(cfg, st, t, 1, o);
        if (o.flags[0] != LMPC_LL_IK_NAN || std::memcmp(o.joint_ang_tgt, st.joint_pos, 3 * sizeof(double)) != 0)
            return fail("out-of-reach target", -1);
        if (o.flags[1] | o.flags[2] | o.flags[3]) return fail("out-of-reach target leaked into another leg", -1);
    }
    {  // a NaN force on RL
        lmpc_wbc_target t = tg;
        t.forces_des[7] = std::numeric_limits<double>::quiet_NaN();
        lmpc_ll::robot(cfg, st, t, 1, o);
        if (o.flags[2] != LMPC_LL_TAU_NONFINITE || (o.flags[0] | o.flags[1] | o.flags[3])) return fail("NaN force", -1);
    }
    {  // an infinite velocity target: the solve turns it into a NaN (the fallback) or passes it on to tau
        lmpc_wbc_target t = tg;
        t.foot_vel_des[3] = std::numeric_limits<double>::infinity();
        lmpc_ll::robot(cfg, st, t, 1, o);
        if (!(o.flags[1] & (LMPC_LL_VEL_NAN | LMPC_LL_TAU_NONFINITE))) return fail("infinite velocity target", -1);
    }
    {  // a singular leg (zero-length links): the solve divides by zero pivots, nothing reads out of bounds
        lmpc_lowlevel_cfg flat = cfg;
        flat.kin.rho_fix[3][2] = flat.kin.rho_fix[3][3] = flat.kin.rho_fix[3][4] = 0.0;
        lmpc_ll::robot(flat, st, tg, 1, o);
        if (o.flags[3] == 0) return fail("singular leg raised no flag", -1);
    }
    {  // the clamp
        lmpc_lowlevel_cfg lim = cfg;
        lim.tau_limit[0] = lim.tau_limit[1] = lim.tau_limit[2] = 5.0;
        lmpc_wbc_target t = tg;
        for (int l = 0; l < 4; ++l) t.forces_des[3 * l + 2] = 150.0;
        lmpc_ll::robot(lim, st, t, 1, o);
        int clamped = 0;
        for (int l = 0; l < 4; ++l) clamped += (o.flags[l] & LMPC_LL_CLAMPED) != 0;
        for (int j = 0; j < 12; ++j)
            if (!(std::fabs(o.tau[j]) <= 5.0)) return fail("clamp", -1);
        if (clamped == 0) return fail("clamp flag", -1);
    }
    std::printf("lowlevel_host_check ok: 2 x %d robots, round trip %.2e rad, J w - v %.2e, %d torques clamped, %d not\n",
                robots, worst_rt, worst_lu, clamped, free);
    return 0;
}
