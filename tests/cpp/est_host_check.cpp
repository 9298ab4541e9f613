// est_host_check.cpp -- a stand-alone program over csrc/lmpc_est_common.h (no HIP, no liblmpc): it runs a few filters
// through the header's host path, so that the shared arithmetic can run under the host compiler's sanitizers
// (-fsanitize=address,undefined; tests/test_est_host.py builds and runs it).  It checks what needs no reference:
// status 0, a symmetric P with a positive diagonal, finite estimates, noise that repeats for a key; and that a NaN
// reading comes back with status 1, zero outputs and the filter unchanged.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lmpc_est_common.h"

namespace {

// a small trunk-and-four-legs model of the header's class (Go1-like round numbers; the filter reads the kinematics only)
lmpc_rbd_model toy_model() {
    lmpc_rbd_model m{};
    m.gravity = 9.81;
    m.mass[0] = 5.0;
    for (int leg = 0; leg < 4; ++leg) {
        const double sx = (leg & 2) ? -1.0 : 1.0, sy = (leg & 1) ? -1.0 : 1.0;
        for (int k = 0; k < 3; ++k) m.mass[1 + 3 * leg + k] = 0.5;
        m.joint_origin[3 * leg][0] = 0.19 * sx, m.joint_origin[3 * leg][1] = 0.05 * sy;
        m.joint_origin[3 * leg + 1][1] = 0.08 * sy;
        m.joint_origin[3 * leg + 2][2] = -0.21;
        m.foot[leg][2] = -0.21;
    }
    return m;
}

int fail(const char* what, int robot) {
    std::printf("FAIL: %s (robot %d)\n", what, robot);
    return 1;
}

}  // namespace

int main() {
    const lmpc_rbd_model md = toy_model();
    lmpc_est_cfg cfg{};
    cfg.dt = 0.00125, cfg.noise_pimu = cfg.noise_vimu = cfg.noise_pfoot = 0.01;
    cfg.noise_pimu_rel_foot = 0.001, cfg.noise_vimu_rel_foot = 0.1, cfg.noise_zfoot = 0.001;
    cfg.gravity = 9.81, cfg.drift_threshold = 1e-6, cfg.drift_divisor = 10.0, cfg.init_P = 3.0;
    cfg.assume_flat_ground = 1;
    cfg.sigma_acc = 0.05, cfg.sigma_gyro = 0.01, cfg.sigma_joint_vel = 0.02, cfg.seed = 99;
    const int robots = 6, ticks = 40;
    for (int r = 0; r < robots; ++r) {
        std::vector<lmpc_est_filter> fs(1);  // on the heap: the sanitizer watches its bounds
        std::vector<lmpc_est_sensors> sns(ticks);
        lmpc_est_filter& f = fs[0];
        lmpc_rbd_state st{};
        lmpc_sim_out so{};
        st.euler[0] = 0.4 * r, st.euler[1] = 0.05 * r, st.euler[2] = -0.03 * r;
        st.pos[2] = 0.3;
        for (int t = 0; t < ticks; ++t) {
            for (int l = 0; l < 4; ++l) {
                st.joint_pos[3 * l] = 0.1 * std::sin(0.1 * t + l), st.joint_pos[3 * l + 1] = 0.8 + 0.1 * std::cos(0.07 * t);
                st.joint_pos[3 * l + 2] = -1.6 + 0.2 * std::sin(0.05 * t + r);
                st.joint_vel[3 * l + 1] = 0.5 * std::cos(0.2 * t);
                so.touch[l] = ((r + t / 10) >> l) & 1;
            }
            so.qdd[0] = 0.3 * std::sin(0.3 * t), so.qdd[2] = 0.1;
            st.omega[2] = 0.2;
            lmpc_est_sensors& sn = sns[t];
            lmpc_est::sensors_from_plant(md, cfg, st, so, r, (uint32_t)t, r == robots - 1, sn);
            lmpc_est_sensors again;
            lmpc_est::sensors_from_plant(md, cfg, st, so, r, (uint32_t)t, r == robots - 1, again);
            if (std::memcmp(&sn, &again, sizeof sn) != 0) return fail("noise does not repeat for its key", r);
            if (t == 0) {
                const double pos0[3] = {0.0, 0.0, 0.3};
                lmpc_est::init_robot(md, cfg, sn, r % 2 ? pos0 : nullptr, f);
            }
            lmpc_rbd_state se;
            lmpc_est_out out;
            if (lmpc_est::update_robot(md, cfg, sn, f, &se, &out) != 0 || out.status != 0) return fail("update status", r);
            for (int i = 0; i < LMPC_EST_NX; ++i) {
                if (!std::isfinite(f.x[i]) || !(f.P[i * LMPC_EST_NX + i] > 0.0)) return fail("x or P's diagonal", r);
                for (int j = 0; j < LMPC_EST_NX; ++j)
                    if (f.P[i * LMPC_EST_NX + j] != f.P[j * LMPC_EST_NX + i]) return fail("P not symmetric", r);
            }
            lmpc_sim_out shadow;
            lmpc_est::feedback_robot(so, out, shadow);
            if (shadow.qdd[2] != so.qdd[2] || shadow.foot_pos[5] != out.foot_pos_world[5]) return fail("feedback", r);
        }
        if (f.ticks != ticks) return fail("tick count", r);
        // a NaN reading: status 1, zero outputs, the filter untouched
        lmpc_est_sensors bad = sns[ticks - 1];
        bad.imu_acc[1] = std::nan("");
        const lmpc_est_filter before = f;
        lmpc_rbd_state se;
        lmpc_est_out out;
        std::memset(&se, 0xA5, sizeof se), std::memset(&out, 0xA5, sizeof out);
        if (lmpc_est::update_robot(md, cfg, bad, f, &se, &out) != 1 || out.status != 1) return fail("NaN not reported", r);
        const lmpc_rbd_state zs{};
        lmpc_est_out zo{};
        zo.status = 1;
        if (std::memcmp(&f, &before, sizeof f) != 0 || std::memcmp(&se, &zs, sizeof se) != 0 ||
            std::memcmp(&out, &zo, sizeof out) != 0)
            return fail("NaN: filter changed or outputs not zero", r);
    }
    std::printf("est_host_check ok: %d robots x %d ticks\n", robots, ticks);
    return 0;
}
