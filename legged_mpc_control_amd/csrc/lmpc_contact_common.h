// lmpc_contact_common.h -- the friction-pyramid contact problem and the plant step of include/lmpc/lmpc_contact.h,
// written once and compiled for the host (one robot, the feet in a loop: solve_quad() / step_robot() below) and for
// gfx950 (lmpc_contact.hip: one lane per foot).  It builds on lmpc_sim_common.h (the elimination, K = J M^-1 J', the
// 3 x 3 block tools and the plant step's front and back halves, which the two plants share), and has no HIP runtime
// call: a plain C++ program can include it (tests/cpp/contact_host_check.cpp).
//
// The problem, per robot:  min 1/2 P' K P + P' c  over the feet of the mask, |P_x| <= mu P_z, |P_y| <= mu P_z per foot,
// with the 3 x 3 blocks K_lm of K and c_l = u_free_l + b_l.  The pieces, each a function of one foot (one lane):
//   mode_basis()   a mode's basis T (3 x 3, columns of dropped coordinates zero): P_l = T y_l
//   foot_subqp()   one foot's problem with the others fixed, solved exactly: the ten modes in closed form (T' A T by a
//                  3 x 3 Cholesky padded with the identity), the feasible one of least objective taken
//   reduce_blk()   T_l' K_lm T_m, the identity on the dropped coordinates of a diagonal block: with these blocks
//                  lmpc_sim_common.h's block Cholesky over the legs solves the problem restricted to given modes
//   foot_cert()    the certificate's violations for one foot, from P_l, w_l and the mode alone
// Every sum over feet runs in the order FL, FR, RL, RR.
//
// No function here contracts a * b + c (LMPC_NO_FMA): host and device differ only through sin / cos.
#pragma once
#include "lmpc/lmpc_contact.h"
#include "lmpc_sim_common.h"

namespace lmpc_contact {
using namespace lmpc_sim;
using lmpc_sim::finite;  // not <math.h>'s

constexpr int MODE_FREE = LMPC_CONTACT_MODE_FREE, MODE_APEX = LMPC_CONTACT_MODE_APEX, MODE_NONE = LMPC_CONTACT_MODE_NONE;

// by components: a ?: on the structs themselves selects between their addresses, which puts them into scratch
LMPC_HD inline V3 sel(bool take, const V3& a, const V3& b) { return V3{take ? a.x : b.x, take ? a.y : b.y, take ? a.z : b.z}; }
LMPC_HD inline double max3abs(const V3& a) { return fmax(fmax(fabs(a.x), fabs(a.y)), fabs(a.z)); }

struct Caps {
    double mu, tol_p, tol_d;
    int max_sweeps, max_polish;
};

// ---- modes ---------------------------------------------------------------------------------------------------------
// sx, sy: the side of the pyramid the mode holds P_x / P_y on (0: not held); on: the foot carries a force at all
LMPC_HD inline void mode_signs(int mode, int& sx, int& sy, bool& on) {
    on = mode < MODE_APEX;
    sx = (mode == 1 || mode == 5 || mode == 6) ? 1 : ((mode == 2 || mode == 7 || mode == 8) ? -1 : 0);
    sy = (mode == 3 || mode == 5 || mode == 7) ? 1 : ((mode == 4 || mode == 6 || mode == 8) ? -1 : 0);
}
// T = [ax 0 cx; 0 ay cy; 0 0 az]: y = (y_x, y_y, y_z) -> P = (ax y_x + cx y_z, ay y_y + cy y_z, az y_z)
struct Basis {
    double ax, ay, az, cx, cy;
};
LMPC_HD inline Basis mode_basis(int mode, double mu) {
    int sx, sy;
    bool on;
    mode_signs(mode, sx, sy, on);
    Basis b;
    b.ax = (on && sx == 0) ? 1.0 : 0.0;
    b.ay = (on && sy == 0) ? 1.0 : 0.0;
    b.az = on ? 1.0 : 0.0;
    b.cx = !on ? 0.0 : (sx > 0 ? mu : (sx < 0 ? -mu : 0.0));
    b.cy = !on ? 0.0 : (sy > 0 ? mu : (sy < 0 ? -mu : 0.0));
    return b;
}
LMPC_HD inline V3 basis_apply(const Basis& b, const V3& y) {  // T y
    LMPC_NO_FMA
    return V3{b.ax * y.x + b.cx * y.z, b.ay * y.y + b.cy * y.z, b.az * y.z};
}
LMPC_HD inline V3 basis_tmul(const Basis& b, const V3& v) {  // T' v
    LMPC_NO_FMA
    return V3{b.ax * v.x, b.ay * v.y, (b.cx * v.x + b.cy * v.y) + b.az * v.z};
}
// Tm' K Tn; a diagonal block gets the identity on the coordinates its basis drops
LMPC_HD inline void reduce_blk(const Blk& k, const Basis& m, const Basis& n, bool diagonal, Blk& r) {
    LMPC_NO_FMA
    V3 kt[3];  // rows of K Tn
#pragma unroll
    for (int i = 0; i < 3; ++i)
        kt[i] = V3{k.a[i][0] * n.ax, k.a[i][1] * n.ay, (k.a[i][0] * n.cx + k.a[i][1] * n.cy) + k.a[i][2] * n.az};
    const V3 r0 = scale(m.ax, kt[0]), r1 = scale(m.ay, kt[1]);
    const V3 r2 = add(add(scale(m.cx, kt[0]), scale(m.cy, kt[1])), scale(m.az, kt[2]));
    r.a[0][0] = diagonal ? r0.x + (1.0 - m.ax) : r0.x, r.a[0][1] = r0.y, r.a[0][2] = r0.z;
    r.a[1][0] = r1.x, r.a[1][1] = diagonal ? r1.y + (1.0 - m.ay) : r1.y, r.a[1][2] = r1.z;
    r.a[2][0] = r2.x, r.a[2][1] = r2.y, r.a[2][2] = diagonal ? r2.z + (1.0 - m.az) : r2.z;
}
// the reduced right-hand side -T' c
LMPC_HD inline V3 reduce_rhs(const Basis& b, const V3& c) {
    const V3 t = basis_tmul(b, c);
    return V3{-t.x, -t.y, -t.z};
}

// ---- one foot --------------------------------------------------------------------------------------------------------
// the smallest of the four pyramid slacks mu P_z -+ P_x, mu P_z -+ P_y
LMPC_HD inline double min_slack(const V3& p, double mu) {
    LMPC_NO_FMA
    const double m = mu * p.z;
    return fmin(fmin(m - p.x, m + p.x), fmin(m - p.y, m + p.y));
}
// c + sum_k K[k] P[k] over the feet in leg order, the term of foot `skip` left out (skip < 0: none)
LMPC_HD inline V3 row_sum(const Blk K[4], const V3 P[4], const V3& c, int skip) {
    V3 a = c;
#pragma unroll
    for (int k = 0; k < 4; ++k) a = sel(k == skip, a, add(a, mul3(K[k].a, P[k])));
    return a;
}
// min 1/2 p' A p + p' r over the pyramid: every mode's minimiser in closed form, the feasible one of least objective.
// The optimum is the minimiser of its own mode and every feasible candidate lies at or above it, so this is exact.
LMPC_HD inline void foot_subqp(const Blk& A, const V3& r, double mu, V3& P, int& mode) {
    LMPC_NO_FMA
    P = v3(0.0, 0.0, 0.0), mode = MODE_APEX;
    double fbest = 0.0;
#pragma unroll 1
    for (int m = 0; m < MODE_APEX; ++m) {
        const Basis b = mode_basis(m, mu);
        Blk R;
        reduce_blk(A, b, b, true, R);
        Chol3 L;
        const bool ok = chol3(R.a, v3(0.0, 0.0, 0.0), L);
        const V3 p = basis_apply(b, chol3_solve(L, reduce_rhs(b, r)));
        const double s = mu * p.z;
        const bool feasible = ok && s - p.x >= 0.0 && s + p.x >= 0.0 && s - p.y >= 0.0 && s + p.y >= 0.0;
        const double f = 0.5 * dot(p, mul3(A.a, p)) + dot(p, r);
        const bool take = feasible && f < fbest;
        P = sel(take, p, P), mode = take ? m : mode, fbest = take ? f : fbest;
    }
}
// The certificate for one foot: pv = the largest violation of a pyramid slack, dv = the dual violation by mode.
LMPC_HD inline void foot_cert(int mode, const V3& P, const V3& w, double mu, double& pv, double& dv) {
    LMPC_NO_FMA
    int sx, sy;
    bool on;
    mode_signs(mode, sx, sy, on);
    const bool in = mode != MODE_NONE, hx = sx != 0, hy = sy != 0;
    const double ms = min_slack(P, mu);
    pv = (in && ms < 0.0) ? -ms : 0.0;
    // least-squares multipliers of the active faces' normals n_x = (-sx, 0, mu), n_y = (0, -sy, mu)
    const double dx = (double)sx, dy = (double)sy, m2 = mu * mu, nn = 1.0 + m2;
    const double rx = mu * w.z - dx * w.x, ry = mu * w.z - dy * w.y, det = nn * nn - m2 * m2;
    const double lx = !hx ? 0.0 : (hy ? (nn * rx - m2 * ry) / det : rx / nn);
    const double ly = !hy ? 0.0 : (hx ? (nn * ry - m2 * rx) / det : ry / nn);
    const V3 e = V3{w.x + lx * dx, w.y + ly * dy, w.z - mu * (lx + ly)};
    const double dvon = fmax(max3abs(e), fmax(hx ? -lx : 0.0, hy ? -ly : 0.0));
    const double a = w.z - mu * (fabs(w.x) + fabs(w.y));
    dv = !in ? 0.0 : (on ? dvon : (a < 0.0 ? -a : 0.0));
}
LMPC_HD inline double foot_scale(const V3& P, const V3& c, bool in) { return in ? fmax(max3abs(P), max3abs(c)) : 0.0; }

// c = u_free + b from leg_rows()'s rhs (= -u_free) and the gap
LMPC_HD inline V3 contact_c(const V3& rhs, double gap, bool use_gap, double recover_speed, double dt) {
    LMPC_NO_FMA
    const double bz = use_gap ? fmax(gap, -(recover_speed * dt)) / dt : 0.0;
    return V3{-rhs.x, -rhs.y, bz - rhs.z};
}
LMPC_HD inline int touch_flag(int rule, double foot_z, double ground_z, const V3& force, double threshold) {
    LMPC_NO_FMA
    return rule == 0 ? (foot_z <= ground_z ? 1 : 0) : (sqrt(dot(force, force)) > threshold ? 1 : 0);
}

LMPC_HD inline int start_mode(bool in, bool sticking) { return !in ? MODE_NONE : (sticking ? MODE_FREE : MODE_APEX); }

// ---- host: one robot, the feet in a loop ---------------------------------------------------------------------------
// The problem restricted to given modes (lmpc_sim_common.h's solve_contacts() on the reduced blocks; the lower blocks
// K[m][k], k <= m, are read).  false: a non-positive pivot.
inline bool solve_modes(const Blk K[4][4], const V3 c[4], const int mode[4], double mu, V3 P[4]) {
    Blk B[4][4];
    Chol3 Ld[4];
    V3 t[4], floor[4];
    Basis bs[4];
    bool ok = true;
    for (int m = 0; m < 4; ++m) bs[m] = mode_basis(mode[m], mu);
    for (int m = 0; m < 4; ++m) {
        for (int k = 0; k <= m; ++k) reduce_blk(K[m][k], bs[m], bs[k], m == k, B[m][k]);
        floor[m] = blk_floor(B[m][m]);
        t[m] = reduce_rhs(bs[m], c[m]);
    }
    for (int k = 0; k < 4; ++k) {
        ok = chol3(B[k][k].a, floor[k], Ld[k]) && ok;
        for (int m = k + 1; m < 4; ++m) blk_trsm(B[m][k], Ld[k]);
        for (int j = k + 1; j < 4; ++j)
            for (int m = j; m < 4; ++m) blk_update(B[m][j], B[m][k], B[j][k]);
    }
    for (int k = 0; k < 4; ++k) {  // L y = t
        t[k] = chol3_fwd(Ld[k], t[k]);
        for (int m = k + 1; m < 4; ++m) t[m] = sub(t[m], mul3(B[m][k].a, t[k]));
    }
    V3 y[4];
    for (int k = 3; k >= 0; --k) {  // L' y = t
        V3 a = t[k];
        for (int m = k + 1; m < 4; ++m) a = sub(a, mul3t(B[m][k].a, y[m]));
        y[k] = chol3_bwd(Ld[k], a);
    }
    for (int m = 0; m < 4; ++m) P[m] = sel(mode[m] < MODE_APEX, basis_apply(bs[m], y[m]), v3(0.0, 0.0, 0.0));
    return ok;
}

// w of every foot and the certificate's two residuals (relative to s) for P with the given modes
inline void certify(const Blk K[4][4], const V3 c[4], const bool in[4], const int mode[4], const V3 P[4], double mu,
                    V3 w[4], double& rp, double& rd) {
    double s = 1.0, pvm = 0.0, dvm = 0.0;
    for (int l = 0; l < 4; ++l) {
        w[l] = sel(in[l], row_sum(K[l], P, c[l], -1), v3(0.0, 0.0, 0.0));
        double pv, dv;
        foot_cert(mode[l], P[l], w[l], mu, pv, dv);
        pvm = fmax(pvm, pv), dvm = fmax(dvm, dv), s = fmax(s, foot_scale(P[l], c[l], in[l]));
    }
    rp = pvm / s, rd = dvm / s;
}

struct Sol {
    V3 P[4], w[4];
    int mode[4], sweeps, polish;
    double res_p, res_d;
    bool bad, certified;
};
// K: all sixteen blocks.  The loop of include/lmpc/lmpc_contact.h's "Solver".
inline void solve_quad(const Blk K[4][4], const V3 c[4], const bool in[4], const Caps& cp, Sol& s) {
    // the first trial: every foot of the mask sticking (with no polish round to try it in: P = 0, every foot at the apex)
    for (int l = 0; l < 4; ++l) s.P[l] = v3(0.0, 0.0, 0.0), s.mode[l] = start_mode(in[l], cp.max_polish > 0);
    s.sweeps = s.polish = 0, s.bad = false;
    bool done = false;
    for (int it = 0; it <= cp.max_sweeps && !done; ++it) {
        if (it > 0) {
            for (int k = 0; k < 4; ++k)
                if (in[k]) foot_subqp(K[k][k], row_sum(K[k], s.P, c[k], k), cp.mu, s.P[k], s.mode[k]);
            ++s.sweeps;
        }
        V3 cand[4] = {s.P[0], s.P[1], s.P[2], s.P[3]}, w[4];
        if (s.polish < cp.max_polish) {
            s.bad = !solve_modes(K, c, s.mode, cp.mu, cand) || s.bad;
            ++s.polish;
        }
        double rp, rd;
        certify(K, c, in, s.mode, cand, cp.mu, w, rp, rd);
        const bool pfeas = rp <= cp.tol_p;
        if (pfeas)
            for (int l = 0; l < 4; ++l) s.P[l] = cand[l];
        else if (it == 0)  // the trial is dropped: back to P = 0, whose mode is the apex
            for (int l = 0; l < 4; ++l) s.mode[l] = start_mode(in[l], false);
        done = (pfeas && rd <= cp.tol_d) || s.bad;
    }
    certify(K, c, in, s.mode, s.P, cp.mu, s.w, s.res_p, s.res_d);
    s.certified = s.res_p <= cp.tol_p && s.res_d <= cp.tol_d;
}

// the caps bound a loop that every lane of a wavefront runs: a larger one is an argument error, not a longer kernel
constexpr int MAX_CAP = LMPC_CONTACT_MAX_CAP;
inline bool positive(double x) { return x > 0.0 && finite(x); }
inline bool not_negative(double x) { return x >= 0.0 && finite(x); }
inline bool good_solver_cfg(const lmpc_contact_cfg& c) {
    return positive(c.mu) && positive(c.tol_p) && positive(c.tol_d) && c.max_sweeps >= 0 && c.max_sweeps <= MAX_CAP &&
           c.max_polish >= 0 && c.max_polish <= MAX_CAP;
}
inline bool good_step_cfg(const lmpc_contact_cfg& c) {
    return good_solver_cfg(c) && positive(c.dt) && finite(c.ground_z) && not_negative(c.recover_speed) &&
           not_negative(c.force_threshold) && (c.touch_rule == 0 || c.touch_rule == 1);
}
inline Caps caps_of(const lmpc_contact_cfg& c) { return Caps{c.mu, c.tol_p, c.tol_d, c.max_sweeps, c.max_polish}; }

inline void zero_cout(lmpc_contact_out& o, int status) {
    o = lmpc_contact_out{};
    o.status = status;
}

// The bare problem: K 12 x 12 row-major, c (12), mask (4) -> P (12), out.  Returns the status.
inline int solve_bare(const lmpc_contact_cfg& cfg, const double* Kd, const double* cd, const int32_t* mask, double* Pd,
                      lmpc_contact_out& out) {
    Blk K[4][4];
    V3 c[4];
    bool in[4];
    for (int m = 0; m < 4; ++m) {
        for (int k = 0; k < 4; ++k)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) K[m][k].a[i][j] = Kd[(3 * m + i) * 12 + 3 * k + j];
        c[m] = v3(cd[3 * m], cd[3 * m + 1], cd[3 * m + 2]);
        in[m] = mask[m] != 0;
    }
    Sol s;
    solve_quad(K, c, in, caps_of(cfg), s);
    bool bad = s.bad;
    for (int l = 0; l < 4; ++l) bad = bad || !finite(s.P[l]) || !finite(s.w[l]);
    if (bad) {
        zero_cout(out, 1);
        for (int i = 0; i < 12; ++i) Pd[i] = 0.0;
        return 1;
    }
    zero_cout(out, s.certified ? 0 : 2);
    for (int l = 0; l < 4; ++l) {
        Pd[3 * l] = s.P[l].x, Pd[3 * l + 1] = s.P[l].y, Pd[3 * l + 2] = s.P[l].z;
        out.w[3 * l] = s.w[l].x, out.w[3 * l + 1] = s.w[l].y, out.w[3 * l + 2] = s.w[l].z;
        out.mode[l] = s.mode[l];
    }
    out.res_primal = s.res_p, out.res_dual = s.res_d, out.sweeps = s.sweeps, out.polish = s.polish;
    return out.status;
}

// One plant step of the frictional plant: lmpc_sim_common.h's plant_terms() / plant_back() / plant_finish() with the
// contact problem between them, where solve_robot() has the unilateral rule.
// Returns the status; on 1, `out` and `cout` are zero and `next` = `st`.  `next` may alias `st`; `cout` may be null.
inline int step_robot(const lmpc_rbd_model& md, const lmpc_contact_cfg& cfg, const lmpc_rbd_state& st, const double* tau,
                      const int32_t* mask, lmpc_rbd_state* next, lmpc_sim_out& out, lmpc_contact_out* cout) {
    const double dt = cfg.dt;
    PlantTerms t;
    plant_terms(md, st, tau, dt, true, t);
    V3 c[4], xl[4];
    bool in[4];
    double gap[4], xb[6];
    for (int l = 0; l < 4; ++l) {
        in[l] = mask[l] != 0;
        gap[l] = (st.pos[2] + t.g[l].foot.z) - cfg.ground_z;
        c[l] = contact_c(t.w[l].rhs, gap[l], cfg.use_gap != 0, cfg.recover_speed, dt);
    }
    Sol s;
    solve_quad(t.K, c, in, caps_of(cfg), s);
    bool bad = plant_back(t, s.P, t.bad || s.bad, xb, xl);
    for (int l = 0; l < 4; ++l) bad = bad || !finite(s.w[l]);
    const int status = bad ? 1 : (s.certified ? 0 : 2);
    plant_finish(t, st, true, dt, xb, xl, s.P, status, next, out);
    if (cout) zero_cout(*cout, status);
    if (bad) return 1;
    for (int l = 0; l < 4; ++l) {
        const V3 force = v3(out.force[3 * l], out.force[3 * l + 1], out.force[3 * l + 2]);
        out.held[l] = s.P[l].z > 0.0;
        out.touch[l] = touch_flag(cfg.touch_rule, out.foot_pos[3 * l + 2], cfg.ground_z, force, cfg.force_threshold);
        if (!cout) continue;
        cout->w[3 * l] = s.w[l].x, cout->w[3 * l + 1] = s.w[l].y, cout->w[3 * l + 2] = s.w[l].z;
        cout->gap[l] = gap[l], cout->mode[l] = s.mode[l];
    }
    if (cout) cout->res_primal = s.res_p, cout->res_dual = s.res_d, cout->sweeps = s.sweeps, cout->polish = s.polish;
    return status;
}

}  // namespace lmpc_contact
