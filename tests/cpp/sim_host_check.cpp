// sim_host_check.cpp -- a stand-alone program over csrc/lmpc_sim_common.h (no HIP, no liblmpc): it steps a few robots
// through the header's host path, so that the shared arithmetic can run under the host compiler's sanitizers
// (-fsanitize=address,undefined; tests/test_sim_host.py builds and runs it).  It checks what needs no reference:
// status 0, held feet with zero velocity after the step, released feet with zero force, finite states; and that a
// singular configuration comes back with status 1, a zero block and the state unchanged.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lmpc_sim_common.h"

namespace {

// a small trunk-and-four-legs model of the header's class (Go1-like round numbers)
lmpc_rbd_model toy_model() {
    lmpc_rbd_model m{};
    m.gravity = 9.81;
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
    }
    return m;
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

}  // namespace

int main() {
    const lmpc_rbd_model md = toy_model();
    lmpc_sim_cfg cfg{};
    cfg.dt = 0.002, cfg.ground_z = 0.0, cfg.unilateral = 1;
    const int robots = 6, steps = 5;
    for (int r = 0; r < robots; ++r) {
        lmpc_rbd_state st{};
        st.euler[0] = uniform(-3.0, 3.0), st.euler[1] = uniform(-0.5, 0.5), st.euler[2] = uniform(-0.5, 0.5);
        st.pos[2] = 0.3;
        for (int l = 0; l < 4; ++l) {
            st.joint_pos[3 * l] = uniform(-0.3, 0.3), st.joint_pos[3 * l + 1] = uniform(0.4, 1.2);
            st.joint_pos[3 * l + 2] = uniform(-2.0, -1.0);
        }
        for (int i = 0; i < 3; ++i) st.omega[i] = uniform(-0.5, 0.5), st.lin_vel[i] = uniform(-0.5, 0.5);
        for (int i = 0; i < 12; ++i) st.joint_vel[i] = uniform(-2.0, 2.0);
        double tau[12];
        for (int i = 0; i < 12; ++i) tau[i] = uniform(-5.0, 5.0);
        int32_t contact[4];
        for (int l = 0; l < 4; ++l) contact[l] = ((r + 1) >> l) & 1;
        if (r == robots - 1) contact[0] = contact[1] = contact[2] = contact[3] = 1;
        std::vector<lmpc_sim_out> outs(steps);  // on the heap: the sanitizer watches its bounds
        lmpc_sim_out fd;
        if (lmpc_sim::solve_robot(md, st, tau, contact, true, false, 0.0, 0.0, nullptr, fd) != 0 || fd.status != 0)
            return fail("forward dynamics status", r);
        for (int s = 0; s < steps; ++s) {
            lmpc_sim_out& o = outs[s];
            const bool unilateral = s % 2 == 0;
            if (lmpc_sim::solve_robot(md, st, tau, contact, unilateral, true, cfg.dt, cfg.ground_z, &st, o) != 0)
                return fail("step status", r);
            for (int l = 0; l < 4; ++l) {
                if (o.held[l] && !contact[l]) return fail("a foot held that was no candidate", r);
                if (!unilateral && o.held[l] != (contact[l] != 0)) return fail("bilateral set changed", r);
                for (int i = 0; i < 3; ++i) {
                    if (o.held[l] && std::fabs(o.foot_vel[3 * l + i]) > 1e-9) return fail("held foot moves", r);
                    if (!o.held[l] && o.force[3 * l + i] != 0.0) return fail("released foot carries force", r);
                }
                if (unilateral && o.held[l] && o.force[3 * l + 2] < 0.0) return fail("held foot pulls", r);
            }
            const double* x = reinterpret_cast<const double*>(&st);
            for (int i = 0; i < 36; ++i)
                if (!std::isfinite(x[i])) return fail("non-finite state", r);
        }
    }
    // singular: zero-length legs on coincident hips give two held feet identical Jacobian rows
    lmpc_rbd_model flat = md;
    std::memset(flat.joint_origin, 0, sizeof flat.joint_origin);
    std::memset(flat.foot, 0, sizeof flat.foot);
    lmpc_rbd_state st{}, next{};
    st.pos[2] = 0.3;
    const double tau[12] = {};
    const int32_t contact[4] = {1, 1, 0, 0};
    lmpc_sim_out o;
    std::memset(&o, 0xA5, sizeof o);
    if (lmpc_sim::solve_robot(flat, st, tau, contact, false, true, cfg.dt, cfg.ground_z, &next, o) != 1 || o.status != 1)
        return fail("singular configuration not reported", -1);
    const lmpc_sim_out zero{};
    o.status = 0;
    if (std::memcmp(&o, &zero, sizeof o) != 0 || std::memcmp(&st, &next, sizeof st) != 0)
        return fail("singular configuration: block not zero or state changed", -1);
    std::printf("sim_host_check ok: %d robots x %d steps\n", robots, steps);
    return 0;
}
