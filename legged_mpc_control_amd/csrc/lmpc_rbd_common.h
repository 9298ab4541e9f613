// lmpc_rbd_common.h -- the floating-base rigid-body dynamics of include/lmpc/lmpc_rbd.h, written once and compiled
// for the host (one robot, the legs in a loop) and for gfx950 (lmpc_rbd.hip: one lane per leg).
//
// Everything is expressed in world-aligned axes with positions relative to the base origin (the base position
// enters only foot_pos and com), so a robot's precision does not depend on where it stands.  The base's three Euler
// joints have the world-frame axes e0 = z, e1 = Rz y, e2 = Rz Ry x (the columns of E, omega = E rates), which makes
// the generalised force / Jacobian column / inertia column of Euler coordinate k the projection on e_k of the
// corresponding moment about the base origin.
//
//   leg_pass()    one leg: forward kinematics, velocities and the accelerations at qdd = 0, each body's
//                 Newton-Euler wrench, the composite bodies of the three subtrees (mass, first moment, inertia about
//                 the base origin), the leg's 3 x 3 block of M, its 6 x 3 coupling block, its Jacobian columns, dJv,
//                 nle of its joints -- and the leg's totals (LegOut::sum), the only thing the base block needs from it
//   base_pass()   trunk + the four legs' totals in leg order: M's 6 x 6 block, nle[0:6], CoM, the centroidal block
//   base_accel()  wbc.cpp:195-203 from the centroidal block and the desired forces
//
// No function here contracts a * b + c (LMPC_NO_FMA): host and device differ only through sin / cos.
#pragma once
#include <cmath>
#include <cstdint>

#include "lmpc/lmpc_rbd.h"

#if defined(__HIPCC__)
#define LMPC_HD __host__ __device__
#else
#define LMPC_HD
#endif
#ifndef LMPC_NO_FMA
#define LMPC_NO_FMA _Pragma("clang fp contract(off)")
#endif

namespace lmpc_rbd {

struct V3 {
    double x, y, z;
};
struct Sym3 {  // symmetric 3 x 3
    double xx, xy, xz, yy, yz, zz;
};
struct M3 {  // columns
    V3 cx, cy, cz;
};

LMPC_HD inline V3 v3(double x, double y, double z) { return V3{x, y, z}; }
LMPC_HD inline V3 add(const V3& a, const V3& b) {
    LMPC_NO_FMA
    return V3{a.x + b.x, a.y + b.y, a.z + b.z};
}
LMPC_HD inline V3 sub(const V3& a, const V3& b) {
    LMPC_NO_FMA
    return V3{a.x - b.x, a.y - b.y, a.z - b.z};
}
LMPC_HD inline V3 scale(double s, const V3& a) {
    LMPC_NO_FMA
    return V3{s * a.x, s * a.y, s * a.z};
}
LMPC_HD inline double dot(const V3& a, const V3& b) {
    LMPC_NO_FMA
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
LMPC_HD inline V3 cross(const V3& a, const V3& b) {
    LMPC_NO_FMA
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
LMPC_HD inline V3 mul(const M3& m, const V3& a) {  // m a
    LMPC_NO_FMA
    return V3{m.cx.x * a.x + m.cy.x * a.y + m.cz.x * a.z, m.cx.y * a.x + m.cy.y * a.y + m.cz.y * a.z,
              m.cx.z * a.x + m.cy.z * a.y + m.cz.z * a.z};
}
LMPC_HD inline V3 mul(const Sym3& s, const V3& a) {
    LMPC_NO_FMA
    return V3{s.xx * a.x + s.xy * a.y + s.xz * a.z, s.xy * a.x + s.yy * a.y + s.yz * a.z,
              s.xz * a.x + s.yz * a.y + s.zz * a.z};
}
LMPC_HD inline Sym3 add(const Sym3& a, const Sym3& b) {
    LMPC_NO_FMA
    return Sym3{a.xx + b.xx, a.xy + b.xy, a.xz + b.xz, a.yy + b.yy, a.yz + b.yz, a.zz + b.zz};
}
// m (|c|^2 1 - c c'): the inertia of a point mass m at c about the origin
LMPC_HD inline Sym3 point_inertia(double m, const V3& c) {
    LMPC_NO_FMA
    return Sym3{m * (c.y * c.y + c.z * c.z), -(m * (c.x * c.y)), -(m * (c.x * c.z)),
                m * (c.x * c.x + c.z * c.z), -(m * (c.y * c.z)), m * (c.x * c.x + c.y * c.y)};
}
LMPC_HD inline Sym3 sub(const Sym3& a, const Sym3& b) {
    LMPC_NO_FMA
    return Sym3{a.xx - b.xx, a.xy - b.xy, a.xz - b.xz, a.yy - b.yy, a.yz - b.yz, a.zz - b.zz};
}
// R I R' for the body inertia I = (ixx ixy ixz iyy iyz izz)
LMPC_HD inline Sym3 rotate_inertia(const M3& R, const double* I) {
    LMPC_NO_FMA
    const Sym3 s{I[0], I[1], I[2], I[3], I[4], I[5]};
    // columns of I R' are I applied to the rows of R
    const V3 r0{R.cx.x, R.cy.x, R.cz.x}, r1{R.cx.y, R.cy.y, R.cz.y}, r2{R.cx.z, R.cy.z, R.cz.z};
    const V3 t0 = mul(s, r0), t1 = mul(s, r1), t2 = mul(s, r2);
    return Sym3{dot(r0, t0), dot(r0, t1), dot(r0, t2), dot(r1, t1), dot(r1, t2), dot(r2, t2)};
}
// w' x (w' x d) + wd x d: acceleration of a point at d from a frame's origin (angular velocity w, acceleration wd)
LMPC_HD inline V3 point_accel(const V3& w, const V3& wd, const V3& d) { return add(cross(wd, d), cross(w, cross(w, d))); }

// What is additive over bodies: mass, first moment and inertia about the base origin; force and moment about the
// base origin of the Newton-Euler wrench at qdd = 0 (gravity included).
struct Part {
    double m;
    V3 mc;
    Sym3 Io;
    V3 F, N;
};
LMPC_HD inline Part add(const Part& a, const Part& b) {
    LMPC_NO_FMA
    return Part{a.m + b.m, add(a.mc, b.mc), add(a.Io, b.Io), add(a.F, b.F), add(a.N, b.N)};
}

// One body at (R, p) moving with (w, wd) and origin acceleration ap.
LMPC_HD inline Part body_part(const lmpc_rbd_model& md, int b, const M3& R, const V3& p, const V3& w, const V3& wd,
                              const V3& ap, double gravity) {
    LMPC_NO_FMA
    const double m = md.mass[b];
    const V3 rc = mul(R, v3(md.com[b][0], md.com[b][1], md.com[b][2]));
    const V3 c = add(p, rc);
    const Sym3 Iw = rotate_inertia(R, md.inertia[b]);
    V3 ac = add(ap, point_accel(w, wd, rc));
    ac.z = ac.z + gravity;
    const V3 f = scale(m, ac);
    const V3 n = add(mul(Iw, wd), cross(w, mul(Iw, w)));
    return Part{m, scale(m, c), add(Iw, point_inertia(m, c)), f, add(n, cross(c, f))};
}

struct BaseKin {
    M3 R;
    V3 e0, e1, e2;  // world axes of the yaw, pitch, roll coordinates (columns of E)
    V3 rates;       // (yaw, pitch, roll) rates
    V3 vlin;
    V3 w, wd;       // world angular velocity E rates; its derivative at qdd = 0
};

LMPC_HD inline BaseKin base_kin(const lmpc_rbd_state& s) {
    LMPC_NO_FMA
    BaseKin k;
    const double sz = sin(s.euler[0]), cz = cos(s.euler[0]), sy = sin(s.euler[1]), cy = cos(s.euler[1]);
    const double sx = sin(s.euler[2]), cx = cos(s.euler[2]);
    k.R.cx = v3(cz * cy, sz * cy, -sy);
    k.R.cy = v3(cz * sy * sx - sz * cx, sz * sy * sx + cz * cx, cy * sx);
    k.R.cz = v3(cz * sy * cx + sz * sx, sz * sy * cx - cz * sx, cy * cx);
    k.e0 = v3(0.0, 0.0, 1.0);
    k.e1 = v3(-sz, cz, 0.0);
    k.e2 = k.R.cx;
    // getEulerAnglesZyxDerivativesFromGlobalAngularVelocity (wbc.cpp:54): rates = E^-1 omega
    const double wx = s.omega[0], wy = s.omega[1], wz = s.omega[2];
    const double planar = cz * wx + sz * wy;
    k.rates = v3(sy * planar / cy + wz, cz * wy - sz * wx, planar / cy);
    k.vlin = v3(s.lin_vel[0], s.lin_vel[1], s.lin_vel[2]);
    // the three Euler joints as a chain: w accumulates e_k rate_k, wd the (w_parent x e_k) rate_k terms
    const V3 w0 = scale(k.rates.x, k.e0);
    const V3 w1 = add(w0, scale(k.rates.y, k.e1));
    k.w = add(w1, scale(k.rates.z, k.e2));
    k.wd = add(scale(k.rates.y, cross(w0, k.e1)), scale(k.rates.z, cross(w1, k.e2)));
    return k;
}

LMPC_HD inline Part trunk_part(const lmpc_rbd_model& md, const BaseKin& k) {
    return body_part(md, 0, k.R, v3(0.0, 0.0, 0.0), k.w, k.wd, v3(0.0, 0.0, 0.0), md.gravity);
}

// Everything one leg contributes.
struct LegOut {
    double Mll[3][3];  // the leg's own block of M (symmetric, both triangles)
    double Mbl[6][3];  // rows 0-5 of M, the leg's three columns
    double Jb[3][3];   // d foot / d (yaw, pitch, roll): column k = e_k x r_foot  (Jb[row][k])
    double Jl[3][3];   // d foot / d leg joints (Jl[row][k])
    V3 foot;           // relative to the base origin
    V3 foot_vel, dJv;
    double nle[3];
    Part sum;          // the whole leg
};

// R Rot(axis, q): axis x for the hip, y for thigh and calf
LMPC_HD inline M3 joint_rot(const M3& R, bool about_x, double q) {
    LMPC_NO_FMA
    const double s = sin(q), c = cos(q);
    M3 o;
    if (about_x) {
        o.cx = R.cx;
        o.cy = add(scale(c, R.cy), scale(s, R.cz));
        o.cz = sub(scale(c, R.cz), scale(s, R.cy));
    } else {
        o.cx = sub(scale(c, R.cx), scale(s, R.cz));
        o.cy = R.cy;
        o.cz = add(scale(s, R.cx), scale(c, R.cz));
    }
    return o;
}

LMPC_HD inline void leg_pass(const lmpc_rbd_model& md, const lmpc_rbd_state& st, const BaseKin& bk, int leg, LegOut& o) {
    LMPC_NO_FMA
    // forward: the three links
    M3 R = bk.R;
    V3 p = v3(0.0, 0.0, 0.0), vp = bk.vlin, ap = v3(0.0, 0.0, 0.0), w = bk.w, wd = bk.wd;
    V3 pj[3], ax[3];
    Part body[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = 3 * leg + k;
        const V3 d = mul(R, v3(md.joint_origin[j][0], md.joint_origin[j][1], md.joint_origin[j][2]));
        p = add(p, d);
        vp = add(vp, cross(w, d));
        ap = add(ap, point_accel(w, wd, d));
        const V3 a = k == 0 ? R.cx : R.cy;  // the joint frame is the parent's, unrotated
        const double qd = st.joint_vel[j];
        wd = add(wd, scale(qd, cross(w, a)));
        w = add(w, scale(qd, a));
        R = joint_rot(R, k == 0, st.joint_pos[j]);
        pj[k] = p;
        ax[k] = a;
        body[k] = body_part(md, 1 + j, R, p, w, wd, ap, md.gravity);
    }
    const V3 rf = mul(R, v3(md.foot[leg][0], md.foot[leg][1], md.foot[leg][2]));
    o.foot = add(p, rf);
    o.foot_vel = add(vp, cross(w, rf));
    o.dJv = add(ap, point_accel(w, wd, rf));
    // backward: subtree composites calf, calf + thigh, calf + thigh + hip
    Part tree[3];
    tree[2] = body[2];
    tree[1] = add(tree[2], body[1]);
    tree[0] = add(tree[1], body[0]);
    o.sum = tree[0];
    V3 lin[3], ang[3];  // momentum of subtree j per unit rate of joint j: linear, angular about the base origin
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        lin[j] = cross(ax[j], sub(tree[j].mc, scale(tree[j].m, pj[j])));
        ang[j] = sub(mul(tree[j].Io, ax[j]), cross(tree[j].mc, cross(ax[j], pj[j])));
        o.nle[j] = dot(ax[j], sub(tree[j].N, cross(pj[j], tree[j].F)));
        o.Mbl[0][j] = lin[j].x;
        o.Mbl[1][j] = lin[j].y;
        o.Mbl[2][j] = lin[j].z;
        o.Mbl[3][j] = dot(bk.e0, ang[j]);
        o.Mbl[4][j] = dot(bk.e1, ang[j]);
        o.Mbl[5][j] = dot(bk.e2, ang[j]);
        const V3 jc = cross(ax[j], sub(o.foot, pj[j]));
        o.Jl[0][j] = jc.x;
        o.Jl[1][j] = jc.y;
        o.Jl[2][j] = jc.z;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i <= j; ++i) {
            const double mij = dot(ax[i], sub(ang[j], cross(pj[i], lin[j])));
            o.Mll[i][j] = mij;
            o.Mll[j][i] = mij;
        }
    const V3 b0 = cross(bk.e0, o.foot), b1 = cross(bk.e1, o.foot), b2 = cross(bk.e2, o.foot);
    o.Jb[0][0] = b0.x, o.Jb[1][0] = b0.y, o.Jb[2][0] = b0.z;
    o.Jb[0][1] = b1.x, o.Jb[1][1] = b1.y, o.Jb[2][1] = b1.z;
    o.Jb[0][2] = b2.x, o.Jb[1][2] = b2.y, o.Jb[2][2] = b2.z;
}

struct BaseOut {
    double mass;
    double Mbb[6][6];  // M's base block
    double nle[6];
    V3 com;            // relative to the base origin
    double Aw[3][3];   // Ab[3:6, 3:6] = I_com E  (Ab[0:3, :] = Mbb[0:3, :], Ab[3:6, 0:3] = 0)
};

// trunk + FL + FR + RL + RR, in this order
LMPC_HD inline Part total_part(const Part& trunk, const Part& l0, const Part& l1, const Part& l2, const Part& l3) {
    return add(add(add(add(trunk, l0), l1), l2), l3);
}

LMPC_HD inline void base_pass(const BaseKin& bk, const Part& t, BaseOut& o) {
    LMPC_NO_FMA
    o.mass = t.m;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) o.Mbb[i][j] = 0.0;
    o.Mbb[0][0] = o.Mbb[1][1] = o.Mbb[2][2] = t.m;
    const V3 e[3] = {bk.e0, bk.e1, bk.e2};
    V3 Ie[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3 l = cross(e[k], t.mc);  // linear momentum per unit rate of Euler coordinate k
        o.Mbb[0][3 + k] = o.Mbb[3 + k][0] = l.x;
        o.Mbb[1][3 + k] = o.Mbb[3 + k][1] = l.y;
        o.Mbb[2][3 + k] = o.Mbb[3 + k][2] = l.z;
        Ie[k] = mul(t.Io, e[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i <= k; ++i) o.Mbb[3 + i][3 + k] = o.Mbb[3 + k][3 + i] = dot(e[i], Ie[k]);
    o.nle[0] = t.F.x, o.nle[1] = t.F.y, o.nle[2] = t.F.z;
    o.nle[3] = dot(e[0], t.N), o.nle[4] = dot(e[1], t.N), o.nle[5] = dot(e[2], t.N);
    o.com = v3(t.mc.x / t.m, t.mc.y / t.m, t.mc.z / t.m);
    const Sym3 Icom = sub(t.Io, point_inertia(t.m, o.com));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3 a = mul(Icom, e[k]);
        o.Aw[0][k] = a.x, o.Aw[1][k] = a.y, o.Aw[2][k] = a.z;
    }
}

// A^-1 b for a 3 x 3 A by the adjugate
LMPC_HD inline V3 solve3(const double A[3][3], const V3& b) {
    LMPC_NO_FMA
    const V3 c0{A[0][0], A[1][0], A[2][0]}, c1{A[0][1], A[1][1], A[2][1]}, c2{A[0][2], A[1][2], A[2][2]};
    const V3 c12 = cross(c1, c2), c20 = cross(c2, c0), c01 = cross(c0, c1);
    const double det = dot(c0, c12);
    return V3{dot(c12, b) / det, dot(c20, b) / det, dot(c01, b) / det};
}

// hdot_ang's term of one foot: (foot - com) x f
LMPC_HD inline V3 foot_moment(const V3& foot, const V3& com, const double* f) {
    return cross(sub(foot, com), v3(f[0], f[1], f[2]));
}

// wbc.cpp:195-203.  mom = the four feet's foot_moment summed in leg order; forces = forces_des (12).
LMPC_HD inline void base_accel(const BaseKin& bk, const BaseOut& bo, double gravity, const double* forces, const V3& mom,
                               double b[6]) {
    LMPC_NO_FMA
    V3 hl = v3(forces[0], forces[1], forces[2]);
#pragma unroll
    for (int i = 1; i < 4; ++i) hl = add(hl, v3(forces[3 * i], forces[3 * i + 1], forces[3 * i + 2]));
    hl.z = hl.z + bo.mass * (-gravity);
    V3 ba = solve3(bo.Aw, mom);
    // linear rows of Ab: m b_lin + sum_k (e_k x mc) b_ang[k] = hdot_lin
    const V3 bl{(hl.x - (bo.Mbb[0][3] * ba.x + bo.Mbb[0][4] * ba.y + bo.Mbb[0][5] * ba.z)) / bo.mass,
                (hl.y - (bo.Mbb[1][3] * ba.x + bo.Mbb[1][4] * ba.y + bo.Mbb[1][5] * ba.z)) / bo.mass,
                (hl.z - (bo.Mbb[2][3] * ba.x + bo.Mbb[2][4] * ba.y + bo.Mbb[2][5] * ba.z)) / bo.mass};
    const V3 aw{bo.Aw[0][0] * bk.w.x + bo.Aw[0][1] * bk.w.y + bo.Aw[0][2] * bk.w.z,
                bo.Aw[1][0] * bk.w.x + bo.Aw[1][1] * bk.w.y + bo.Aw[1][2] * bk.w.z,
                bo.Aw[2][0] * bk.w.x + bo.Aw[2][1] * bk.w.y + bo.Aw[2][2] * bk.w.z};
    ba = sub(ba, solve3(bo.Aw, cross(bk.w, aw)));
    b[0] = bl.x, b[1] = bl.y, b[2] = bl.z, b[3] = ba.x, b[4] = ba.y, b[5] = ba.z;
}

// kp (p_des - p) + kd (v_des - v), one component (wbc.cpp:239)
LMPC_HD inline double swing_accel(double kp, double kd, double p_des, double p, double v_des, double v) {
    LMPC_NO_FMA
    return kp * (p_des - p) + kd * (v_des - v);
}

}  // namespace lmpc_rbd
