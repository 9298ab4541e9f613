// contact_host_check.cpp -- a stand-alone program over csrc/lmpc_contact_common.h (no HIP, no liblmpc): it steps a few
// robots through the header's host path and solves a few bare problems, so that the shared arithmetic can run under
// the host compiler's sanitizers (-fsanitize=address,undefined; tests/test_contact_host.py builds and runs it).  It
// checks what needs no reference: status 0 with residuals within the tolerances, forces inside the pyramid, no force on
// feet outside the mask, the mode consistent with P, finite states; that caps of 0 come back flagged (status 2); and
// that a singular configuration comes back with status 1, zero blocks and the state unchanged.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lmpc_contact_common.h"

namespace {

// a small trunk-and-four-legs model of the header's class (Go1-like round numbers), as sim_host_check.cpp's
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

lmpc_contact_cfg config() {
    lmpc_contact_cfg c{};
    c.dt = 0.002, c.ground_z = 0.0, c.mu = 0.6, c.recover_speed = 0.0, c.force_threshold = 50.0;
    c.tol_p = c.tol_d = 1e-9, c.use_gap = 1, c.touch_rule = 0, c.max_sweeps = 16, c.max_polish = 8;
    return c;
}

}  // namespace

int main() {
    const lmpc_rbd_model md = toy_model();
    const int robots = 6, steps = 5;
    int modes_seen[11] = {};
    for (int r = 0; r < robots; ++r) {
        lmpc_contact_cfg cfg = config();
        cfg.mu = r % 2 ? 0.3 : 0.6, cfg.use_gap = r % 3 != 0, cfg.touch_rule = r % 2;
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
        int32_t mask[4];
        for (int l = 0; l < 4; ++l) mask[l] = r < 2 ? 1 : ((r + 1) >> l) & 1;
        std::vector<lmpc_sim_out> outs(steps);  // on the heap: the sanitizer watches its bounds
        std::vector<lmpc_contact_out> couts(steps);
        for (int s = 0; s < steps; ++s) {
            lmpc_sim_out& o = outs[s];
            lmpc_contact_out& co = couts[s];
            if (lmpc_contact::step_robot(md, cfg, st, tau, mask, &st, o, s % 2 ? &co : nullptr) != 0 || o.status != 0)
                return fail("step status", r);
            if (s % 2 == 0) continue;
            if (co.status != 0 || !(co.res_primal <= cfg.tol_p) || !(co.res_dual <= cfg.tol_d)) return fail("certificate", r);
            for (int l = 0; l < 4; ++l) {
                const double* F = o.force + 3 * l;
                ++modes_seen[co.mode[l]];
                if ((co.mode[l] == LMPC_CONTACT_MODE_NONE) != (mask[l] == 0)) return fail("mode outside the mask", r);
                if (!mask[l] && (F[0] != 0.0 || F[1] != 0.0 || F[2] != 0.0)) return fail("force outside the mask", r);
                if (co.mode[l] >= LMPC_CONTACT_MODE_APEX && (F[0] != 0.0 || F[1] != 0.0 || F[2] != 0.0)) return fail("apex force", r);
                const double slack = std::fmin(cfg.mu * F[2] - std::fabs(F[0]), cfg.mu * F[2] - std::fabs(F[1]));
                if (slack < -1e-9 * std::fmax(1.0, std::fabs(F[2]))) return fail("force outside the pyramid", r);
                if (o.held[l] != (F[2] > 0.0)) return fail("held flag", r);
            }
            const double* x = reinterpret_cast<const double*>(&st);
            for (int i = 0; i < 36; ++i)
                if (!std::isfinite(x[i])) return fail("non-finite state", r);
        }
        // caps of 0: nothing is verified, unless nothing was to be done
        lmpc_contact_cfg capped = cfg;
        capped.max_sweeps = capped.max_polish = 0;
        lmpc_rbd_state next{};
        lmpc_sim_out o;
        lmpc_contact_out co;
        const int32_t all[4] = {1, 1, 1, 1};
        const int status = lmpc_contact::step_robot(md, capped, st, tau, all, &next, o, &co);
        if (status == 1 || co.sweeps != 0 || co.polish != 0) return fail("caps of 0", r);
    }
    // a bare problem: K = a diagonally dominant symmetric matrix, c pushing every foot into the ground and sideways
    {
        std::vector<double> K(144), c(12), P(12);
        for (int i = 0; i < 12; ++i)
            for (int j = 0; j <= i; ++j) K[i * 12 + j] = K[j * 12 + i] = i == j ? 2.0 + 0.1 * i : 0.05 * std::cos(i + 2 * j);
        for (int l = 0; l < 4; ++l) c[3 * l] = 0.5 * (l - 1.5), c[3 * l + 1] = 0.1 * l, c[3 * l + 2] = l == 3 ? 1.0 : -1.0;
        const int32_t mask[4] = {1, 1, 1, 1};
        lmpc_contact_out co;
        const lmpc_contact_cfg cfg = config();
        if (lmpc_contact::solve_bare(cfg, K.data(), c.data(), mask, P.data(), co) != 0) return fail("bare status", -1);
        if (co.mode[3] != LMPC_CONTACT_MODE_APEX || P[11] != 0.0) return fail("bare: the lifting foot", -1);
        for (int l = 0; l < 3; ++l)
            if (!(P[3 * l + 2] > 0.0)) return fail("bare: a pressed foot carries no force", -1);
    }
    // singular: zero-length legs on coincident hips give two feet of the mask identical Jacobian rows
    lmpc_rbd_model flat = md;
    std::memset(flat.joint_origin, 0, sizeof flat.joint_origin);
    std::memset(flat.foot, 0, sizeof flat.foot);
    lmpc_rbd_state st{}, next{};
    st.pos[2] = 0.3;
    const double tau[12] = {};
    const int32_t mask[4] = {1, 1, 0, 0};
    lmpc_sim_out o;
    lmpc_contact_out co;
    std::memset(&o, 0xA5, sizeof o);
    std::memset(&co, 0xA5, sizeof co);
    lmpc_contact_cfg cfg = config();
    cfg.use_gap = 0;
    if (lmpc_contact::step_robot(flat, cfg, st, tau, mask, &next, o, &co) != 1 || o.status != 1 || co.status != 1)
        return fail("singular configuration not reported", -1);
    const lmpc_sim_out zero{};
    const lmpc_contact_out czero{};
    o.status = 0, co.status = 0;
    if (std::memcmp(&o, &zero, sizeof o) != 0 || std::memcmp(&co, &czero, sizeof co) != 0 ||
        std::memcmp(&st, &next, sizeof st) != 0)
        return fail("singular configuration: block not zero or state changed", -1);
    int distinct = 0;
    for (int m = 0; m < 11; ++m) distinct += modes_seen[m] > 0;
    std::printf("contact_host_check ok: %d robots x %d steps, %d distinct modes\n", robots, steps, distinct);
    return 0;
}
