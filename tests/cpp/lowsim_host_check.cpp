// lowsim_host_check.cpp -- a stand-alone program over csrc/lmpc_lowsim_common.h (no HIP, no liblmpc): it runs
// lmpc_lowsim_run's host function (lmpc_lowsim::run_robot, which lmpc_lowsim.hip exports under that name) on a few
// robots next to the explicit loop -- candidates, lmpc_ll::robot, lmpc_sim::solve_robot per tick -- so that the
// composition can run under the host compiler's sanitizers (-fsanitize=address,undefined; tests/test_lowsim_host.py
// builds and runs it).  Every buffer and log array is on the heap at its exact size: the sanitizer watches the bounds.
// The two must agree byte for byte, with full, partial and no logs; the argument checks must touch nothing.  The robots
// run three times: the mirror-image model on one pair of gains; a model and a cfg with no two legs, gains or limits alike,
// a rho_opt and the ground off zero; and that one with the bilateral plant.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lmpc_lowsim_common.h"

namespace {

// a small trunk-and-four-legs model of lmpc_sim_common.h's class (tests/cpp/sim_host_check.cpp's)
// skew: no two legs alike -- every length and mass scaled per leg -- still inside lmpc_leg_kin_from_model's class
lmpc_rbd_model toy_model(bool skew) {
    lmpc_rbd_model m{};
    m.gravity = skew ? 9.7 : 9.81;
    m.mass[0] = 5.0;
    m.com[0][0] = 0.01;
    m.inertia[0][0] = 0.02, m.inertia[0][3] = 0.07, m.inertia[0][5] = 0.08;
    for (int leg = 0; leg < 4; ++leg) {
        const double sx = (leg & 2) ? -1.0 : 1.0, sy = (leg & 1) ? -1.0 : 1.0;
        const double mass[3] = {0.6, 0.9, 0.2}, cz[3] = {0.0, -0.03, -0.12};
        for (int k = 0; k < 3; ++k) {
            const int b = 1 + 3 * leg + k;
            m.mass[b] = mass[k];
            m.com[b][1] = 0.01 * sy, m.com[b][2] = cz[k];
            m.inertia[b][0] = 0.003, m.inertia[b][3] = 0.003, m.inertia[b][5] = 0.001, m.inertia[b][1] = 1e-5 * sy;
        }
        m.joint_origin[3 * leg][0] = 0.19 * sx, m.joint_origin[3 * leg][1] = 0.05 * sy;
        m.joint_origin[3 * leg + 1][1] = 0.08 * sy;
        m.joint_origin[3 * leg + 2][2] = -0.21;
        m.foot[leg][2] = -0.21;
        if (skew) {
            const double ox[4] = {0.86, 1.02, 1.13, 1.29}, oy[4] = {0.91, 1.04, 1.17, 1.26}, d[4] = {0.88, 0.97, 1.12, 1.31};
            const double lt[4] = {0.87, 1.01, 1.16, 1.28}, lc[4] = {0.81, 0.99, 1.21, 1.34}, ms[4] = {0.7, 1.0, 1.4, 1.9};
            m.joint_origin[3 * leg][0] *= ox[leg], m.joint_origin[3 * leg][1] *= oy[leg];
            m.joint_origin[3 * leg + 1][1] *= d[leg];
            m.joint_origin[3 * leg + 2][2] *= lt[leg];
            m.foot[leg][2] *= lc[leg];
            for (int k = 0; k < 3; ++k) m.mass[1 + 3 * leg + k] *= ms[leg] * (1.0 + 0.03 * k);
        }
    }
    return m;
}

// the controller's kinematics of that model (lmpc_leg_kin_from_model's rule)
lmpc_lowlevel_cfg toy_cfg(const lmpc_rbd_model& m, double kp, double kd) {
    lmpc_lowlevel_cfg c{};
    for (int l = 0; l < 4; ++l) {
        const double rf[5] = {m.joint_origin[3 * l][0], m.joint_origin[3 * l][1], m.joint_origin[3 * l + 1][1],
                              -m.joint_origin[3 * l + 2][2], -m.foot[l][2]};
        std::memcpy(c.kin.rho_fix[l], rf, sizeof rf);
        for (int k = 0; k < 3; ++k) c.kp[l][k] = kp, c.kd[l][k] = kd;
    }
    return c;
}

// the same kinematics with 12 different kp, 12 different kd, three limits and a rho_opt (the sign of rho_opt[l][1] is
// the leg's d's)
lmpc_lowlevel_cfg skew_cfg(const lmpc_rbd_model& m) {
    lmpc_lowlevel_cfg c = toy_cfg(m, 0.0, 0.0);
    const double ro[4][3] = {{0.007, 0.014, -0.011}, {0.010, -0.015, -0.020}, {-0.019, 0.016, 0.017}, {-0.012, -0.009, -0.013}};
    const double kp[4][3] = {{5.8, 9.7, 0.5}, {12.4, 8.4, 13.7}, {1.8, 3.1, 7.1}, {15.0, 4.5, 11.0}};
    const double kd[4][3] = {{0.45, 0.27, 0.49}, {0.56, 0.53, 0.24}, {0.60, 0.35, 0.31}, {0.38, 0.20, 0.42}};
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

template <class T>
bool same(const T& a, const T& b) {
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

}  // namespace

int main() {
    // pass 0: the mirror-image robot on one pair of gains, the ground at 0; pass 1: no two legs alike, no two gains or
    // limits alike, a rho_opt, the ground off zero and 1.5 times the weight asked of the stance feet (so that the limits
    // bite); pass 2: the same, bilateral
    const int robots = 6;
    int released = 0, failed_steps = 0, clamped = 0, pulling = 0;
    lmpc_rbd_model md{};
    lmpc_lowlevel_cfg cfg{};
    lmpc_sim_cfg sc{};
    for (int pr = 0; pr < 3 * robots; ++pr) {
        const int pass = pr / robots, r = pr % robots;
        md = toy_model(pass > 0);
        cfg = pass > 0 ? skew_cfg(md) : toy_cfg(md, 15.0, 0.4);
        sc.dt = 0.00125, sc.ground_z = pass > 0 ? -0.23 : 0.0, sc.unilateral = pass < 2;
        const bool uni = sc.unilateral != 0;
        const int ticks = r % 2 ? 8 : 3, substeps = r % 3 == 0 ? 3 : 1;
        lmpc_rbd_state st{};
        st.euler[0] = uniform(-3.0, 3.0), st.euler[1] = uniform(-0.05, 0.05), st.euler[2] = uniform(-0.05, 0.05);
        for (int l = 0; l < 4; ++l) {
            st.joint_pos[3 * l] = uniform(-0.1, 0.1), st.joint_pos[3 * l + 1] = uniform(0.7, 0.9);
            st.joint_pos[3 * l + 2] = uniform(-1.7, -1.5);
        }
        // the feet of this pose, to put the lowest one on the ground
        const double zero[12] = {};
        const int32_t none[4] = {0, 0, 0, 0};
        lmpc_sim_out fd;
        if (lmpc_sim::solve_robot(md, st, zero, none, true, false, 0.0, 0.0, nullptr, fd) != 0) return fail("pose", r);
        double lowest = fd.foot_pos[2];
        for (int l = 1; l < 4; ++l) lowest = fd.foot_pos[3 * l + 2] < lowest ? fd.foot_pos[3 * l + 2] : lowest;
        st.pos[2] = sc.ground_z - lowest + (r == 2 ? 2e-4 : -1e-6);  // robot 2 starts above the ground
        lmpc_wbc_target tg{};
        lmpc_sim_out so{};
        for (int l = 0; l < 4; ++l) {
            const bool swing = l == (r & 1) || l == 3 - (r & 1);
            for (int i = 0; i < 3; ++i) tg.foot_pos_des[3 * l + i] = fd.foot_pos[3 * l + i] + (i < 2 ? st.pos[i] : st.pos[2]);
            if (swing) tg.foot_pos_des[3 * l + 2] += 0.03;
            tg.forces_des[3 * l + 2] = swing ? 0.0 : (pass > 0 ? 90.0 : 30.0);
            so.held[l] = so.touch[l] = fd.foot_pos[3 * l + 2] + st.pos[2] <= sc.ground_z;
        }
        if (r == robots - 1) tg.forces_des[4] = std::nan("");  // the plant fails on every tick
        const int32_t gait = r == 4 ? LMPC_GAIT_STAND : 0;

        // the explicit loop
        std::vector<lmpc_rbd_state> e_states(ticks);
        std::vector<lmpc_sim_out> e_outs(ticks);
        std::vector<lmpc_lowlevel_out> e_ll(ticks);
        std::vector<int32_t> e_cand(4 * ticks);
        lmpc_rbd_state es = st;
        lmpc_sim_out eo = so;
        for (int i = 0; i < ticks; ++i) {
            for (int l = 0; l < 4; ++l) e_cand[4 * i + l] = lmpc_ll::candidate(eo.held[l], eo.touch[l]);
            lmpc_ll::robot(cfg, es, tg, gait == LMPC_GAIT_STAND ? 0 : 1, e_ll[i]);
            for (int s = 0; s < substeps; ++s) {
                const int status = lmpc_sim::solve_robot(md, es, e_ll[i].tau, &e_cand[4 * i], uni, true, sc.dt, sc.ground_z,
                                                         &es, eo);
                failed_steps += status;
            }
            for (int l = 0; l < 4; ++l) {
                released += e_cand[4 * i + l] == 1 && eo.status == 0 && eo.held[l] == 0;
                clamped += (e_ll[i].flags[l] & LMPC_LL_CLAMPED) != 0;
                pulling += !uni && eo.status == 0 && eo.held[l] == 1 && eo.force[3 * l + 2] < 0.0;
            }
            e_states[i] = es, e_outs[i] = eo;
        }

        // lmpc_lowsim_run: all logs, only the states, none
        for (int variant = 0; variant < 3; ++variant) {
            std::vector<lmpc_rbd_state> states(ticks);
            std::vector<lmpc_sim_out> outs(ticks);
            std::vector<lmpc_lowlevel_out> lls(ticks);
            std::vector<int32_t> cands(4 * ticks);
            std::vector<int32_t> cand(4);
            std::vector<lmpc_lowlevel_out> ll(1);
            std::vector<lmpc_rbd_state> s1(1, st);
            std::vector<lmpc_sim_out> o1(1, so);
            lmpc_lowsim_log log{states.data(), variant == 0 ? outs.data() : nullptr, variant == 0 ? lls.data() : nullptr,
                                variant == 0 ? cands.data() : nullptr};
            const int rc = lmpc_lowsim::run_robot(&md, &sc, &cfg, s1.data(), &tg, &gait, o1.data(), cand.data(), ll.data(),
                                                  ticks, substeps, variant == 2 ? nullptr : &log);
            if (rc != LMPC_OK) return fail("return code", r);
            if (!same(s1[0], es) || !same(o1[0], eo) || !same(ll[0], e_ll[ticks - 1]) ||
                std::memcmp(cand.data(), &e_cand[4 * (ticks - 1)], 16) != 0)
                return fail("the final buffers differ from the explicit loop's", r);
            if (variant < 2 && std::memcmp(states.data(), e_states.data(), ticks * sizeof(lmpc_rbd_state)) != 0)
                return fail("logged states", r);
            if (variant == 0 && (std::memcmp(outs.data(), e_outs.data(), ticks * sizeof(lmpc_sim_out)) != 0 ||
                                 std::memcmp(lls.data(), e_ll.data(), ticks * sizeof(lmpc_lowlevel_out)) != 0 ||
                                 std::memcmp(cands.data(), e_cand.data(), 16 * ticks) != 0))
                return fail("logged outs / ll_outs / candidates", r);
        }
    }
    if (released == 0) return fail("no foot was released by the unilateral rule: the inputs are too tame", -1);
    if (failed_steps == 0) return fail("the NaN force did not fail the plant", -1);
    if (clamped == 0) return fail("no torque limit was reached", -1);
    if (pulling == 0) return fail("no held foot pulls in the bilateral pass", -1);

    // argument checks: nothing is touched
    lmpc_rbd_state st{};
    lmpc_sim_out so{};
    lmpc_wbc_target tg{};
    lmpc_lowlevel_out ll;
    int32_t cand[4] = {7, 7, 7, 7};
    std::memset(&ll, 0xA5, sizeof ll);
    const lmpc_rbd_state st0 = st;
    lmpc_sim_cfg bad = sc;
    bad.dt = 0.0;
    if (lmpc_lowsim::run_robot(&md, &sc, &cfg, &st, &tg, nullptr, &so, cand, &ll, -1, 1, nullptr) != LMPC_ERR_ARG ||
        lmpc_lowsim::run_robot(&md, &sc, &cfg, &st, &tg, nullptr, &so, cand, &ll, 2, 0, nullptr) != LMPC_ERR_ARG ||
        lmpc_lowsim::run_robot(&md, &bad, &cfg, &st, &tg, nullptr, &so, cand, &ll, 2, 1, nullptr) != LMPC_ERR_ARG ||
        lmpc_lowsim::run_robot(nullptr, &sc, &cfg, &st, &tg, nullptr, &so, cand, &ll, 2, 1, nullptr) != LMPC_ERR_ARG ||
        lmpc_lowsim::run_robot(&md, &sc, &cfg, nullptr, &tg, nullptr, &so, cand, &ll, 2, 1, nullptr) != LMPC_ERR_ARG ||
        lmpc_lowsim::run_robot(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                               nullptr) != LMPC_OK)
        return fail("argument checks", -1);
    if (!same(st, st0) || cand[0] != 7 || ((unsigned char*)&ll)[0] != 0xA5) return fail("a refused call wrote", -1);
    std::printf("lowsim_host_check ok: 3 x %d robots, %d releases by the unilateral rule, %d failed plant steps, %d clamped "
                "legs, %d pulling feet\n", robots, released, failed_steps, clamped, pulling);
    return 0;
}
