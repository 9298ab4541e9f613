// lmpc_sim_common.h -- the contact-constrained forward dynamics and the plant step of include/lmpc/lmpc_sim.h, written
// once and compiled for the host (one robot, the legs in a loop: plant_terms() / plant_back() / plant_finish() below,
// which both plants' host steps are made of -- solve_robot() here, lmpc_contact_common.h's step_robot()) and for gfx950
// (lmpc_sim_device.h: one lane per leg, the same three pieces).  It builds on lmpc_rbd_common.h's leg_pass() / base_pass() and has no HIP runtime call: a plain C++
// program can include it (tests/cpp/sim_host_check.cpp).
//
// The system, for the increment x (qdd, or v+ - v), the multipliers P (F, or the impulse), s = 1 or dt:
//     base rows      Mbb xb + sum_l Mbl_l xl_l - sum_{l in C} Y_l' P_l = -s nle_b
//     leg l's rows   Mbl_l' xb + Mll_l xl_l - [l in C] Jl_l' P_l       = s (tau_l - nle_l)           =: rl_l
//     foot l in C    Y_l xb + Jl_l xl_l                                = -dJv_l  or  -foot_vel_l     =: c_l
// with Y_l = [1 (3 x 3), Jb_l] the base columns of foot l's Jacobian.  Elimination order (every factor symmetric
// positive definite, no pivoting):
//   1. leg_reduce()   per leg, with G = Mll^-1 by a 3 x 3 Cholesky: the joints xl = G (rl - Mbl' xb + Jl' P) leave
//                     Cs = Mbl G Mbl', rbc = Mbl G rl, D = Y - Jl G Mbl' (3 x 6), A = Jl G Jl', cl = c - Jl G rl
//   2. base_factor()  Sb = Mbb - Cs_FL - Cs_FR - Cs_RL - Cs_RR = Ls Ls' (6 x 6: M's Schur complement on the base),
//                     yb = Ls^-1 (-s nle_b - rbc_FL - ... - rbc_RR)
//   3. leg_rows()     Z = (Ls^-1 D')' (3 x 6), rhs = cl - Z yb; the 12 x 12 matrix K = J M^-1 J' has the 3 x 3 blocks
//                     K_lm = Z_l Z_m' (+ A_l on the diagonal).  Nothing up to here depends on the contact set.
//   4. per pass of the unilateral rule: rows and columns of feet outside C replaced by the identity (their P is 0), a
//      block Cholesky of K over the four legs (blk_*: leg l owns block row l, K_l0 .. K_ll), P from two block
//      triangular solves
//   5. base_back(), leg_back()   xb = Ls^-T (yb + Z_FL' P_FL + ... + Z_RR' P_RR), then xl
// K is the inverse inertia seen at the held feet: it stays well conditioned (cond <= 65 over the joint range) where a
// single leg's A = Jl G Jl' does not (a foot on its hip axis), because the base gives the foot its missing mobility.
// Every sum over legs runs in the order FL, FR, RL, RR.
//
// No function here contracts a * b + c (LMPC_NO_FMA): host and device differ only through sin / cos.
#pragma once
#include "lmpc/lmpc_sim.h"
#include "lmpc_rbd_common.h"

namespace lmpc_sim {
using namespace lmpc_rbd;

LMPC_HD inline bool finite(double x) {
    LMPC_NO_FMA
    return x - x == 0.0;
}
LMPC_HD inline bool finite(const V3& a) { return finite(a.x) && finite(a.y) && finite(a.z); }

// A pivot of K that is not above PIVOT_REL times the diagonal entry it started from counts as non-positive: K is then
// singular to rounding (two held feet with the same Jacobian rows leave a pivot of a few ulp of either sign).  A
// pivot is at least the smallest eigenvalue and the diagonal at most the largest, so cond(K) < 1e10 never trips it.
constexpr double PIVOT_REL = 1e-10;

// ---- 3 x 3 ------------------------------------------------------------------------------------------------------
// lower Cholesky factor of a symmetric 3 x 3 (the upper triangle is read)
struct Chol3 {
    double l00, l10, l11, l20, l21, l22;
};
// false: a pivot was not above its floor (0, or PIVOT_REL times the entry it started from); the factor is then unusable
LMPC_HD inline bool chol3(const double A[3][3], const V3& floor, Chol3& c) {
    LMPC_NO_FMA
    bool ok = A[0][0] > floor.x;
    c.l00 = sqrt(A[0][0]);
    c.l10 = A[0][1] / c.l00;
    c.l20 = A[0][2] / c.l00;
    const double d1 = A[1][1] - c.l10 * c.l10;
    ok = ok && d1 > floor.y;
    c.l11 = sqrt(d1);
    c.l21 = (A[1][2] - c.l20 * c.l10) / c.l11;
    const double d2 = (A[2][2] - c.l20 * c.l20) - c.l21 * c.l21;
    ok = ok && d2 > floor.z;
    c.l22 = sqrt(d2);
    return ok;
}
LMPC_HD inline V3 chol3_fwd(const Chol3& c, const V3& b) {  // L^-1 b
    LMPC_NO_FMA
    const double y0 = b.x / c.l00;
    const double y1 = (b.y - c.l10 * y0) / c.l11;
    const double y2 = ((b.z - c.l20 * y0) - c.l21 * y1) / c.l22;
    return V3{y0, y1, y2};
}
LMPC_HD inline V3 chol3_bwd(const Chol3& c, const V3& y) {  // L^-T y
    LMPC_NO_FMA
    const double x2 = y.z / c.l22;
    const double x1 = (y.y - c.l21 * x2) / c.l11;
    const double x0 = ((y.x - c.l10 * x1) - c.l20 * x2) / c.l00;
    return V3{x0, x1, x2};
}
LMPC_HD inline V3 chol3_solve(const Chol3& c, const V3& b) { return chol3_bwd(c, chol3_fwd(c, b)); }

LMPC_HD inline V3 row3(const double A[3][3], int i) { return V3{A[i][0], A[i][1], A[i][2]}; }
LMPC_HD inline V3 col3(const double A[3][3], int k) { return V3{A[0][k], A[1][k], A[2][k]}; }
LMPC_HD inline V3 mul3(const double A[3][3], const V3& x) { return V3{dot(row3(A, 0), x), dot(row3(A, 1), x), dot(row3(A, 2), x)}; }
LMPC_HD inline V3 mul3t(const double A[3][3], const V3& x) { return V3{dot(col3(A, 0), x), dot(col3(A, 1), x), dot(col3(A, 2), x)}; }

// ---- 6 x 6 ------------------------------------------------------------------------------------------------------
constexpr int NC = 21;  // upper triangle of a symmetric 6 x 6, entry (i <= k) at k (k + 1) / 2 + i
struct Chol6 {
    double L[6][6];  // lower: L[i][j], j <= i
};
LMPC_HD inline bool chol6(const double S[NC], Chol6& f) {
    LMPC_NO_FMA
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int i = j; i < 6; ++i) {
            double v = S[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - f.L[i][k] * f.L[j][k];
            if (i == j) {
                ok = ok && v > 0.0;
                f.L[j][j] = sqrt(v);
            } else {
                f.L[i][j] = v / f.L[j][j];
            }
        }
    }
    return ok;
}
LMPC_HD inline void chol6_fwd(const Chol6& f, const double b[6], double y[6]) {  // L^-1 b
    LMPC_NO_FMA
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - f.L[i][k] * y[k];
        y[i] = v / f.L[i][i];
    }
}
LMPC_HD inline void chol6_bwd(const Chol6& f, const double y[6], double x[6]) {  // L^-T y
    LMPC_NO_FMA
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - f.L[k][i] * x[k];
        x[i] = v / f.L[i][i];
    }
}
LMPC_HD inline double dot6(const double* a, const double* b) {
    LMPC_NO_FMA
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}
// m - a - b - c - d, left to right: a base entry minus the four legs' contributions in leg order
LMPC_HD inline double minus4(double m, double a, double b, double c, double d) {
    LMPC_NO_FMA
    return (((m - a) - b) - c) - d;
}
LMPC_HD inline double plus4(double m, double a, double b, double c, double d) {
    LMPC_NO_FMA
    return (((m + a) + b) + c) + d;
}

// ---- 1. one leg's joints eliminated ---------------------------------------------------------------------------------
// column k of (Mbl', Y)
LMPC_HD inline V3 col_a(const LegOut& g, int k) { return V3{g.Mbl[k][0], g.Mbl[k][1], g.Mbl[k][2]}; }
LMPC_HD inline V3 col_b(const LegOut& g, int k) {
    return k < 3 ? V3{k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0} : col3(g.Jb, k - 3);
}

// rl = s (tau - nle), c = -dJv (acceleration level) or -foot_vel (velocity level)
LMPC_HD inline void leg_rhs(const LegOut& g, const double* tau3, double s, bool step, V3& rl, V3& c) {
    LMPC_NO_FMA
    rl = V3{s * (tau3[0] - g.nle[0]), s * (tau3[1] - g.nle[1]), s * (tau3[2] - g.nle[2])};
    const V3 d = step ? g.foot_vel : g.dJv;
    c = V3{-d.x, -d.y, -d.z};
}

struct LegRed {
    Chol3 Lm;           // Mll
    bool okm;
    double Cs[NC + 6];  // Mbl G Mbl' (upper triangle), then rbc = Mbl G rl: what the base block needs of the leg
    V3 D[6];            // columns of Y - Jl G Mbl'
    double A[3][3];     // Jl G Jl'
    V3 cl;              // c - Jl G rl
};
LMPC_HD inline void leg_reduce(const LegOut& g, const V3& rl, const V3& c, LegRed& r) {
    LMPC_NO_FMA
    r.okm = chol3(g.Mll, v3(0.0, 0.0, 0.0), r.Lm);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const V3 t = chol3_solve(r.Lm, col_a(g, k));
#pragma unroll
        for (int i = 0; i <= k; ++i) r.Cs[k * (k + 1) / 2 + i] = dot(col_a(g, i), t);
        r.D[k] = sub(col_b(g, k), mul3(g.Jl, t));
    }
    const V3 tr = chol3_solve(r.Lm, rl);
#pragma unroll
    for (int i = 0; i < 6; ++i) r.Cs[NC + i] = dot(col_a(g, i), tr);
    r.cl = sub(c, mul3(g.Jl, tr));
    V3 W[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) W[i] = chol3_solve(r.Lm, row3(g.Jl, i));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) r.A[i][j] = r.A[j][i] = dot(row3(g.Jl, i), W[j]);
}

// ---- 2. the base ---------------------------------------------------------------------------------------------------
// the base's own entries: Mbb (upper triangle, NC) then -s nle_b (6)
LMPC_HD inline void base_entries(const BaseOut& base, double s, double e[NC + 6]) {
    LMPC_NO_FMA
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int i = 0; i <= k; ++i) e[k * (k + 1) / 2 + i] = base.Mbb[i][k];
        e[NC + k] = -(s * base.nle[k]);
    }
}
// e: base_entries minus the four legs' Cs (minus4).  false: a non-positive pivot.
LMPC_HD inline bool base_factor(const double e[NC + 6], Chol6& Ls, double yb[6]) {
    const bool ok = chol6(e, Ls);
    chol6_fwd(Ls, e + NC, yb);
    return ok;
}

// ---- 3. one leg's rows of K -------------------------------------------------------------------------------------------
struct Blk {
    double a[3][3];
};
struct LegRows {
    double Z[3][6];
    V3 rhs;
};
LMPC_HD inline void leg_rows(const LegRed& r, const Chol6& Ls, const double yb[6], LegRows& w) {
    LMPC_NO_FMA
    const double d0[6] = {r.D[0].x, r.D[1].x, r.D[2].x, r.D[3].x, r.D[4].x, r.D[5].x};
    const double d1[6] = {r.D[0].y, r.D[1].y, r.D[2].y, r.D[3].y, r.D[4].y, r.D[5].y};
    const double d2[6] = {r.D[0].z, r.D[1].z, r.D[2].z, r.D[3].z, r.D[4].z, r.D[5].z};
    chol6_fwd(Ls, d0, w.Z[0]);
    chol6_fwd(Ls, d1, w.Z[1]);
    chol6_fwd(Ls, d2, w.Z[2]);
    w.rhs = V3{r.cl.x - dot6(w.Z[0], yb), r.cl.y - dot6(w.Z[1], yb), r.cl.z - dot6(w.Z[2], yb)};
}
// K_lm = Z_l Z_m' (+ A_l if l == m)
LMPC_HD inline void blk_of(const double Zl[3][6], const double Zm[3][6], const double A[3][3], bool diagonal, Blk& b) {
    LMPC_NO_FMA
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = dot6(Zl[i], Zm[j]);
            b.a[i][j] = diagonal ? A[i][j] + v : v;
        }
}
// the floors of a diagonal block's pivots, from the block before any update
LMPC_HD inline V3 blk_floor(const Blk& b) {
    LMPC_NO_FMA
    return V3{PIVOT_REL * b.a[0][0], PIVOT_REL * b.a[1][1], PIVOT_REL * b.a[2][2]};
}

// ---- 4. block Cholesky of K: leg m owns K_m0 .. K_mm ---------------------------------------------------------------
// the masked block: K_mk if both feet are held, else the identity's block
LMPC_HD inline void blk_mask(const Blk& k, bool both, bool diagonal, Blk& b) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) b.a[i][j] = both ? k.a[i][j] : (diagonal && i == j ? 1.0 : 0.0);
}
// B <- B L^-T (L of the diagonal block above it): every row r of B becomes L^-1 r
LMPC_HD inline void blk_trsm(Blk& b, const Chol3& L) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const V3 x = chol3_fwd(L, row3(b.a, i));
        b.a[i][0] = x.x, b.a[i][1] = x.y, b.a[i][2] = x.z;
    }
}
// B_mj <- B_mj - L_mk L_jk'
LMPC_HD inline void blk_update(Blk& mj, const Blk& mk, const Blk& jk) {
    LMPC_NO_FMA
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) mj.a[i][j] = mj.a[i][j] - dot(row3(mk.a, i), row3(jk.a, j));
}

// ---- 5. back-substitution ------------------------------------------------------------------------------------------
// Z' P: the leg's term of the base's right-hand side
LMPC_HD inline void leg_zp(const LegRows& w, const V3& P, double zp[6]) {
    LMPC_NO_FMA
#pragma unroll
    for (int i = 0; i < 6; ++i) zp[i] = (w.Z[0][i] * P.x + w.Z[1][i] * P.y) + w.Z[2][i] * P.z;
}
// t: yb plus the four legs' zp (plus4)
LMPC_HD inline void base_back(const Chol6& Ls, const double t[6], double xb[6]) { chol6_bwd(Ls, t, xb); }
// xl = G (rl - Mbl' xb + Jl' P)
LMPC_HD inline V3 leg_back(const LegOut& g, const LegRed& r, const V3& rl, const double xb[6], const V3& P) {
    LMPC_NO_FMA
    V3 a = rl;
#pragma unroll
    for (int k = 0; k < 6; ++k) a = sub(a, scale(xb[k], col_a(g, k)));
    return chol3_solve(r.Lm, add(a, mul3t(g.Jl, P)));
}

// ---- after the solve --------------------------------------------------------------------------------------------
// The base's part of the next state: v+ = v + x, q+ = q + dt v+, omega+ = E(euler+) rates+.
struct BaseNext {
    V3 euler, pos, omega, vlin, rates;
    double qdd[6];
};
LMPC_HD inline void base_advance(const BaseKin& bk, const V3& euler, const V3& pos, const double xb[6], double dt,
                                 BaseNext& n) {
    LMPC_NO_FMA
    n.vlin = add(bk.vlin, v3(xb[0], xb[1], xb[2]));
    n.rates = add(bk.rates, v3(xb[3], xb[4], xb[5]));
    n.pos = add(pos, scale(dt, n.vlin));
    n.euler = add(euler, scale(dt, n.rates));
    const double sz = sin(n.euler.x), cz = cos(n.euler.x), sy = sin(n.euler.y), cy = cos(n.euler.y);
    const V3 e0 = v3(0.0, 0.0, 1.0), e1 = v3(-sz, cz, 0.0), e2 = v3(cz * cy, sz * cy, -sy);
    n.omega = add(add(scale(n.rates.x, e0), scale(n.rates.y, e1)), scale(n.rates.z, e2));
    const V3 dl = sub(n.vlin, bk.vlin), dr = sub(n.rates, bk.rates);
    n.qdd[0] = dl.x / dt, n.qdd[1] = dl.y / dt, n.qdd[2] = dl.z / dt;
    n.qdd[3] = dr.x / dt, n.qdd[4] = dr.y / dt, n.qdd[5] = dr.z / dt;
}

struct LegNext {
    V3 jp, jv, qdd, force, foot_pos, foot_vel;
};
// jp, jv: the leg's joint angles and rates before the step; pos: the base position before the step
LMPC_HD inline void leg_advance(const LegOut& g, const V3& jp, const V3& jv, const V3& xl, const V3& P, double dt,
                                const BaseNext& bn, const V3& pos, LegNext& n) {
    LMPC_NO_FMA
    n.jv = add(jv, xl);
    n.jp = add(jp, scale(dt, n.jv));
    const V3 d = sub(n.jv, jv);
    n.qdd = V3{d.x / dt, d.y / dt, d.z / dt};
    n.force = V3{P.x / dt, P.y / dt, P.z / dt};
    // J(q) v+ = vlin+ + Jb rates+ + Jl jv+
    n.foot_vel = add(add(bn.vlin, mul3(g.Jb, bn.rates)), mul3(g.Jl, n.jv));
    n.foot_pos = add(add(pos, g.foot), scale(dt, n.foot_vel));
}

// ---- host: one robot, the legs in a loop ------------------------------------------------------------------------
inline void zero_out(lmpc_sim_out& o, int status) {
    o = lmpc_sim_out{};
    o.status = status;
}

// Step 4 for one contact set: P of every leg (0.0 outside the set).  false: a non-positive pivot.
inline bool solve_contacts(const Blk K[4][4], const V3 rhs[4], const bool held[4], V3 P[4]) {
    Blk B[4][4];
    Chol3 Ld[4];
    V3 t[4], floor[4];
    bool ok = true;
    for (int m = 0; m < 4; ++m) {
        for (int k = 0; k <= m; ++k) blk_mask(K[m][k], held[m] && held[k], m == k, B[m][k]);
        floor[m] = blk_floor(B[m][m]);
        t[m] = held[m] ? rhs[m] : v3(0.0, 0.0, 0.0);
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
    for (int k = 3; k >= 0; --k) {  // L' P = y
        V3 a = t[k];
        for (int m = k + 1; m < 4; ++m) a = sub(a, mul3t(B[m][k].a, P[m]));
        P[k] = chol3_bwd(Ld[k], a);
    }
    for (int m = 0; m < 4; ++m)
        if (!held[m]) P[m] = v3(0.0, 0.0, 0.0);
    return ok;
}

// Steps 1-3 for one robot: everything the contact solve and the back-substitution read.  None of it depends on the
// contact set, so both plants (solve_robot() below, lmpc_contact_common.h's step_robot()) build it by plant_terms().
struct PlantTerms {
    BaseKin bk;
    LegOut g[4];
    LegRed r[4];
    V3 rl[4];
    Chol6 Ls;
    double yb[6];
    LegRows w[4];  // w[l].rhs: the right-hand side of foot l's rows of K
    Blk K[4][4];   // all sixteen blocks (solve_contacts() reads the lower ones)
    bool bad;      // a non-positive pivot so far
};
// s = 1 (step = false: the forward dynamics) or dt
inline void plant_terms(const lmpc_rbd_model& md, const lmpc_rbd_state& st, const double* tau, double s, bool step,
                        PlantTerms& t) {
    t.bk = base_kin(st);
    for (int l = 0; l < 4; ++l) leg_pass(md, st, t.bk, l, t.g[l]);
    BaseOut base;
    base_pass(t.bk, total_part(trunk_part(md, t.bk), t.g[0].sum, t.g[1].sum, t.g[2].sum, t.g[3].sum), base);
    t.bad = false;
    for (int l = 0; l < 4; ++l) {
        V3 c;
        leg_rhs(t.g[l], tau + 3 * l, s, step, t.rl[l], c);
        leg_reduce(t.g[l], t.rl[l], c, t.r[l]);
        t.bad = t.bad || !t.r[l].okm;
    }
    double e[NC + 6];
    base_entries(base, s, e);
    for (int n = 0; n < NC + 6; ++n) e[n] = minus4(e[n], t.r[0].Cs[n], t.r[1].Cs[n], t.r[2].Cs[n], t.r[3].Cs[n]);
    t.bad = !base_factor(e, t.Ls, t.yb) || t.bad;
    for (int l = 0; l < 4; ++l) leg_rows(t.r[l], t.Ls, t.yb, t.w[l]);
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < 4; ++k) blk_of(t.w[m].Z, t.w[k].Z, t.r[m].A, m == k, t.K[m][k]);
}

// Step 5 for the multipliers P of either plant's contact solve: xb, xl.  Returns `bad`, or that one of xb, xl, P is not
// finite.
inline bool plant_back(const PlantTerms& t, const V3 P[4], bool bad, double xb[6], V3 xl[4]) {
    double zp[4][6], y[6];
    for (int l = 0; l < 4; ++l) leg_zp(t.w[l], P[l], zp[l]);
    for (int i = 0; i < 6; ++i) y[i] = plus4(t.yb[i], zp[0][i], zp[1][i], zp[2][i], zp[3][i]);
    base_back(t.Ls, y, xb);
    for (int l = 0; l < 4; ++l) xl[l] = leg_back(t.g[l], t.r[l], t.rl[l], xb, P[l]);
    for (int i = 0; i < 6; ++i) bad = bad || !finite(xb[i]);
    for (int l = 0; l < 4; ++l) bad = bad || !finite(xl[l]) || !finite(P[l]);
    return bad;
}

// What the solve leaves in `out` and `next`, for either plant.  status 1 (failed): `out` is zero and, when step, `next`
// = `st`.  Else every field of `out` but held and touch (left 0: the plants' rules for them differ) and, when step, the
// state after it in `next` (step = false: the forward dynamics, dt unused, `next` untouched).  `next` may alias `st`,
// which is not read after it is written.  Returns the status.
inline int plant_finish(const PlantTerms& t, const lmpc_rbd_state& st, bool step, double dt, const double xb[6],
                        const V3 xl[4], const V3 P[4], int status, lmpc_rbd_state* next, lmpc_sim_out& out) {
    zero_out(out, status);
    if (status == 1) {
        if (step && next != &st) *next = st;
        return 1;
    }
    const V3 pos = v3(st.pos[0], st.pos[1], st.pos[2]);
    if (!step) {
        for (int i = 0; i < 6; ++i) out.qdd[i] = xb[i];
        for (int l = 0; l < 4; ++l) {
            const V3 fp = add(pos, t.g[l].foot);
            const double q[3] = {xl[l].x, xl[l].y, xl[l].z}, F[3] = {P[l].x, P[l].y, P[l].z};
            const double p[3] = {fp.x, fp.y, fp.z}, v[3] = {t.g[l].foot_vel.x, t.g[l].foot_vel.y, t.g[l].foot_vel.z};
            for (int i = 0; i < 3; ++i) {
                out.qdd[6 + 3 * l + i] = q[i], out.force[3 * l + i] = F[i];
                out.foot_pos[3 * l + i] = p[i], out.foot_vel[3 * l + i] = v[i];
            }
        }
        return status;
    }
    BaseNext bn;
    base_advance(t.bk, v3(st.euler[0], st.euler[1], st.euler[2]), pos, xb, dt, bn);
    lmpc_rbd_state n;
    n.euler[0] = bn.euler.x, n.euler[1] = bn.euler.y, n.euler[2] = bn.euler.z;
    n.pos[0] = bn.pos.x, n.pos[1] = bn.pos.y, n.pos[2] = bn.pos.z;
    n.omega[0] = bn.omega.x, n.omega[1] = bn.omega.y, n.omega[2] = bn.omega.z;
    n.lin_vel[0] = bn.vlin.x, n.lin_vel[1] = bn.vlin.y, n.lin_vel[2] = bn.vlin.z;
    for (int i = 0; i < 6; ++i) out.qdd[i] = bn.qdd[i];
    for (int l = 0; l < 4; ++l) {
        LegNext a;
        leg_advance(t.g[l], v3(st.joint_pos[3 * l], st.joint_pos[3 * l + 1], st.joint_pos[3 * l + 2]),
                    v3(st.joint_vel[3 * l], st.joint_vel[3 * l + 1], st.joint_vel[3 * l + 2]), xl[l], P[l], dt, bn, pos, a);
        const double jp[3] = {a.jp.x, a.jp.y, a.jp.z}, jv[3] = {a.jv.x, a.jv.y, a.jv.z};
        const double q[3] = {a.qdd.x, a.qdd.y, a.qdd.z}, F[3] = {a.force.x, a.force.y, a.force.z};
        const double p[3] = {a.foot_pos.x, a.foot_pos.y, a.foot_pos.z}, v[3] = {a.foot_vel.x, a.foot_vel.y, a.foot_vel.z};
        for (int i = 0; i < 3; ++i) {
            n.joint_pos[3 * l + i] = jp[i], n.joint_vel[3 * l + i] = jv[i];
            out.qdd[6 + 3 * l + i] = q[i], out.force[3 * l + i] = F[i];
            out.foot_pos[3 * l + i] = p[i], out.foot_vel[3 * l + i] = v[i];
        }
    }
    *next = n;
    return status;
}

// One forward dynamics (step = false: dt and ground_z unused, `next` untouched) or one plant step of the default plant:
// the unilateral rule between plant_terms() and plant_back().  Returns the status; on 1, `out` is zero and `next` =
// `st`.  `next` may alias `st`.
inline int solve_robot(const lmpc_rbd_model& md, const lmpc_rbd_state& st, const double* tau, const int32_t* contact,
                       bool unilateral, bool step, double dt, double ground_z, lmpc_rbd_state* next, lmpc_sim_out& out) {
    PlantTerms t;
    plant_terms(md, st, tau, step ? dt : 1.0, step, t);
    V3 rhs[4], P[4], xl[4];
    bool held[4];
    for (int l = 0; l < 4; ++l) rhs[l] = t.w[l].rhs, held[l] = contact[l] != 0;
    bool bad = t.bad;
    for (int pass = 0; pass < 4; ++pass) {
        bad = !solve_contacts(t.K, rhs, held, P) || bad;
        if (bad || !unilateral) break;
        bool released = false;
        for (int l = 0; l < 4; ++l)
            if (held[l] && P[l].z < 0.0) held[l] = false, released = true;
        if (!released) break;
    }
    // a fourth pass that still released a foot has emptied the set (every pass released at least one of at most four
    // candidates): no foot is held, every P is 0, and no further solve is needed
    for (int l = 0; l < 4; ++l)
        if (!held[l]) P[l] = v3(0.0, 0.0, 0.0);
    double xb[6];
    bad = plant_back(t, P, bad, xb, xl);
    if (plant_finish(t, st, step, dt, xb, xl, P, bad ? 1 : 0, next, out) != 0) return 1;
    for (int l = 0; l < 4; ++l) {
        out.held[l] = held[l];
        if (step) out.touch[l] = out.foot_pos[3 * l + 2] <= ground_z;
    }
    return 0;
}

inline bool good_dt(double dt) { return dt > 0.0 && finite(dt); }

}  // namespace lmpc_sim
