// lmpc_qp_step.h -- the steps of the interior point / polish state machine that are not linear algebra, written once
// for the four QP kernels (lmpc_kernels.hip, lmpc_lq_kernel.h, lmpc_dense_kernel.h with lmpc_dense_common.h,
// lmpc_gi.hip): the prologue's frames and G0, the hand-over test, and per stance leg-step the starting point, the
// complementarity gap, the active-set guess, the barrier terms, the predictor / corrector steps, the gradient from the
// costate, the KKT certificate, the retry ladder's step and the output.
//
// Every function here is per-lane arithmetic on ONE leg-step: the callers loop over their leg-steps, guard by `st`
// (stance) where the function says "stance leg-step", and keep every cross-lane operation (quad_sum, wave_*, __ballot,
// __any) in their own uniform control flow -- dense_took and qp_store_forces, which hold one each, are called by
// every lane unconditionally.  Sums are accumulated into the caller's variable, so a kernel with two leg-steps per
// lane adds in the order it always did.  Inverse slacks come in as an argument `is` indexed by face: the dense kernel
// passes the array it keeps, the Riccati kernels RecipOf{s}, which computes rcp_nr(s[i]) where it is read (a value kept
// across their outlined calls spills).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lmpc/lmpc.h"
#include "lmpc_device.h"
#include "lmpc_kernel_common.h"

namespace lmpc {

// ---- prologue -----------------------------------------------------------------------------------------------------

// "A dense-path kernel took this QP": it has 1..DENSE_MAX_LS stance leg-steps (H <= 16 where prm.dense is set) and,
// where the dense kernel flags the QPs it solved (dense_done), its flag is set -- the ones it left (step cap,
// non-finite step, no verified optimum) are solved by the caller.  Wave-uniform; every lane calls it.
__device__ __forceinline__ bool dense_took(const DevParams& prm, const uint8_t* __restrict__ contact,
                                           const uint8_t* __restrict__ dense_done, int qp, int H, int lane) {
    if (!prm.dense) return false;
    const bool stl = lane < 4 * H && contact[(size_t)qp * 4 * H + lane] != 0;
    const int n = __popcll(__ballot(stl));
    return n >= 1 && n <= DENSE_MAX_LS && (!dense_done || dense_done[qp]);
}

// Contact frame R (row-major, third column the unit normal) of a terrain normal n: the same closed form as
// lmpc_terrain_frame (lmpc_host.cpp).  R = I for n = e_z.
__device__ __forceinline__ void terrain_frame(const double* __restrict__ n, double (&R)[9]) {
    const double n0 = n[0], n1 = n[1], n2 = n[2];
    const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double nx = n0 / nn, ny = n1 / nn, c = n2 / nn;
    const double h = 1.0 / (1.0 + c);
    R[0] = 1.0 - nx * nx * h; R[1] = -nx * ny * h;      R[2] = nx;
    R[3] = -nx * ny * h;      R[4] = 1.0 - ny * ny * h; R[5] = ny;
    R[6] = -nx;               R[7] = -ny;               R[8] = c;
}

// A leg's input Hessian block in its contact frame, R' diag(r) R, packed [xx xy xz yy yz zz]
template <class PR, class PO>
__device__ __forceinline__ void rotated_weights(const double* r, PR R, PO rb) {
    const double r0 = r[0], r1 = r[1], r2 = r[2];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) rb[e++] = r0 * R[a] * R[b] + r1 * R[3 + a] * R[3 + b] + r2 * R[6 + a] * R[6 + b];
}

// iw = (R I_b R')^-1, the world-frame inverse inertia (R: the record's body rotation, row-major)
template <class PR>
__device__ __forceinline__ void world_inertia_inv(PR R, const double* Ib, double (&iw)[9]) {
    double RI[9], Iw[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            RI[i * 3 + j] = R[i * 3 + 0] * Ib[0 * 3 + j] + R[i * 3 + 1] * Ib[1 * 3 + j] + R[i * 3 + 2] * Ib[2 * 3 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Iw[i * 3 + j] = RI[i * 3 + 0] * R[j * 3 + 0] + RI[i * 3 + 1] * R[j * 3 + 1] + RI[i * 3 + 2] * R[j * 3 + 2];
    const double c00 = Iw[4] * Iw[8] - Iw[5] * Iw[7];
    const double c01 = Iw[5] * Iw[6] - Iw[3] * Iw[8];
    const double c02 = Iw[3] * Iw[7] - Iw[4] * Iw[6];
    const double id = 1.0 / (Iw[0] * c00 + Iw[1] * c01 + Iw[2] * c02);
    iw[0] = c00 * id;
    iw[1] = (Iw[2] * Iw[7] - Iw[1] * Iw[8]) * id;
    iw[2] = (Iw[1] * Iw[5] - Iw[2] * Iw[4]) * id;
    iw[3] = c01 * id;
    iw[4] = (Iw[0] * Iw[8] - Iw[2] * Iw[6]) * id;
    iw[5] = (Iw[2] * Iw[3] - Iw[0] * Iw[5]) * id;
    iw[6] = c02 * id;
    iw[7] = (Iw[1] * Iw[6] - Iw[0] * Iw[7]) * id;
    iw[8] = (Iw[0] * Iw[4] - Iw[1] * Iw[3]) * id;
}

// cos / sin of the reference yaw of every step: cs[2k], cs[2k + 1] (xr: x_ref, 12 per step)
template <class PX, class PC>
__device__ __forceinline__ void yaw_cos_sin(PX xr, PC cs, int H, int lane) {
    for (int k = lane; k < H; k += 64) {
        double sn, cn;
        sincos(xr[12 * k + 2], &sn, &cn);
        cs[2 * k] = cn;
        cs[2 * k + 1] = sn;
    }
}

// Entry e = 12 r + 3 j + cc of G0 = dt [I_w^-1 skew(r_j); I/m] (ConvexQPSolver.cpp:198-212; Utils::skew,
// Utils.cpp:89-95), on terrain of G0 blkdiag(R_j) (tf: the legs' frames, 9 each).  a0..a2: row r of I_w^-1 (r < 3) --
// the caller's to read: by selects in the LDS Riccati kernel (a dynamically indexed private array would live in
// scratch memory), by index in the dense prologue.  dt and the mass are read from prm here, not passed by value: an
// argument is loaded at the call, ahead of the branch that uses it, and that one load moved a spill.
template <bool TERRAIN, class PH, class PT>
__device__ __forceinline__ double g0_entry(const DevParams& prm, int e, double a0, double a1, double a2, PH hdr,
                                           PT tf) {
    const double dt = prm.dt;
    const int r = e / 12, c = e % 12, j = c / 3, cc = c % 3;
    double w[3];
    if (r < 3) {
        const auto ft = hdr + LMPC_REC_FEET + 3 * j;
        w[0] = dt * (a1 * ft[2] - a2 * ft[1]);
        w[1] = dt * (-a0 * ft[2] + a2 * ft[0]);
        w[2] = dt * (a0 * ft[1] - a1 * ft[0]);
    } else {
        w[0] = w[1] = w[2] = 0.0;
        w[r - 3] = dt / prm.mass;
    }
    double v = w[cc];
    if constexpr (TERRAIN) {
        const auto Rj = tf + 9 * j;
        v = w[0] * Rj[cc] + w[1] * Rj[3 + cc] + w[2] * Rj[6 + cc];
    }
    return v;
}

// ---- interior point, one leg-step -----------------------------------------------------------------------------------

// Starting point: a stance leg carries its share of the weight (fz = m g / cnt, cnt = the stage's stance legs, capped
// at fmax / 2) and no tangential force; slacks from the constraints, z = 1/s centred (s z = 1).  A swing leg: f = 0,
// s = z = 1.  Measured: ~0.9 fewer interior-point iterations on average than fz = fmax/2, z = 1
// (tools/variant_sweep.py, profiles/r01_init_sweep.log).
__device__ __forceinline__ void ipm_start(bool st, double cnt, double weight, double mu, double fzmax, double (&f)[3],
                                          double (&s)[5], double (&z)[5]) {
    f[0] = f[1] = 0.0;
    f[2] = st ? fmin(0.5 * fzmax, weight / cnt) : 0.0;
    double o[5];
    cons_resid(f, mu, fzmax, o);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        s[i] = st ? -o[i] : 1.0;
        z[i] = 1.0 / s[i];
    }
}

// The inverse slacks of a leg-step, computed where they are read: what the Riccati kernels pass for `is` below
struct RecipOf {
    const double (&s)[5];
    __device__ __forceinline__ double operator[](int i) const { return rcp_nr(s[i]); }
};

// loc += s'z of a stance leg-step (the complementarity gap's local sum)
__device__ __forceinline__ void ipm_gap(const double (&s)[5], const double (&z)[5], double& loc) {
#pragma unroll
    for (int i = 0; i < 5; ++i) loc += s[i] * z[i];
}

// Active set of a stance leg-step guessed from the interior point: z > LMPC_ACT_RATIO s; a lift-off leg -> the apex
__device__ __forceinline__ int ipm_guess_active(const double (&f)[3], const double (&s)[5], const double (&z)[5],
                                                double fzmax) {
    int act = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (z[i] > LMPC_ACT_RATIO * s[i]) act |= 1 << i;
    const double fm = fmax(fabs(f[0]), fmax(fabs(f[1]), fabs(f[2])));
    if (fm < 1e-6 * fzmax) act = 15;
    return act;
}

// Barrier terms of a stage's leg (st: stance; a swing leg has W = 0): Rt = Rb + C'WC with W = diag(z / s), packed
// [xx xy xz yy yz zz], and rt = C'W(s - b) (predictor).  DIAG: Rb = diag(rb[0..2]) (flat ground, where the
// off-diagonal entries take no addition); otherwise rb is the packed block (the dense kernel, whose R is inside H,
// passes zeros).
template <bool DIAG, class IS, class PR>
__device__ __forceinline__ void ipm_barrier(bool st, const double (&s)[5], const IS& is, const double (&z)[5],
                                            double mu, double fzmax, PR rb, double (&Rt)[6], double (&rt)[3]) {
    double W[5] = {0, 0, 0, 0, 0}, wv[5] = {0, 0, 0, 0, 0};
    if (st) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            W[i] = z[i] * is[i];
            wv[i] = W[i] * (s[i] - (i == 4 ? fzmax : 0.0));
        }
    }
    const double sx = W[0] + W[1], sy = W[2] + W[3];
    if constexpr (DIAG) {
        Rt[0] = rb[0] + sx;
        Rt[1] = 0.0;
        Rt[2] = mu * (W[0] - W[1]);
        Rt[3] = rb[1] + sy;
        Rt[4] = mu * (W[2] - W[3]);
        Rt[5] = rb[2] + mu * mu * (sx + sy) + W[4];
    } else {
        Rt[0] = rb[0] + sx;
        Rt[1] = rb[1];
        Rt[2] = rb[2] + mu * (W[0] - W[1]);
        Rt[3] = rb[3] + sy;
        Rt[4] = rb[4] + mu * (W[2] - W[3]);
        Rt[5] = rb[5] + mu * mu * (sx + sy) + W[4];
    }
    cons_tw(wv, mu, rt);
}

// Predictor (affine) step of a stance leg-step from the Newton solution u: dsa, dza, and amax = min(amax, its
// distance to the boundary) -- the hardware reciprocal estimate is ample for the fraction to the boundary.
template <class IS>
__device__ __forceinline__ void ipm_pred_leg(const double (&u)[3], const double (&s)[5], const IS& is,
                                             const double (&z)[5], double mu, double fzmax, double (&dsa)[5],
                                             double (&dza)[5], double& amax) {
    double o[5];
    cons_resid(u, mu, fzmax, o);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        dsa[i] = -o[i] - s[i];
        dza[i] = -z[i] - z[i] * is[i] * dsa[i];
        if (dsa[i] < 0.0) amax = fmin(amax, -s[i] * __builtin_amdgcn_rcp(dsa[i]));
        if (dza[i] < 0.0) amax = fmin(amax, -z[i] * __builtin_amdgcn_rcp(dza[i]));
    }
}

// loc += (s + aa dsa)'(z + aa dza) of a stance leg-step: the gap after the predictor step of length aa
__device__ __forceinline__ void ipm_aff_gap(const double (&s)[5], const double (&z)[5], const double (&dsa)[5],
                                            const double (&dza)[5], double aa, double& loc) {
#pragma unroll
    for (int i = 0; i < 5; ++i) loc += (s[i] + aa * dsa[i]) * (z[i] + aa * dza[i]);
}

// Centring of the corrector: sigma mu with sigma = ratio^3, ratio = the predictor's gap over the iterate's
__device__ __forceinline__ double ipm_centring(double ratio, double mu_c) { return ratio * ratio * ratio * mu_c; }

// Corrector right-hand side of a stance leg-step: rt = C'w, w = (z (s - b) + smu - dsa dza) / s
template <class IS>
__device__ __forceinline__ void ipm_corr_rhs(const double (&s)[5], const IS& is, const double (&z)[5],
                                             const double (&dsa)[5], const double (&dza)[5], double smu, double mu,
                                             double fzmax, double (&rt)[3]) {
    double wv[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) wv[i] = (z[i] * (s[i] - (i == 4 ? fzmax : 0.0)) + smu - dsa[i] * dza[i]) * is[i];
    cons_tw(wv, mu, rt);
}

// Corrector step of a stance leg-step from the Newton solution u (ua: the predictor's, from which its step is
// recomputed): ds, dz, and the primal (amax: s) and dual (dmax: z) distances to the boundary
template <class IS>
__device__ __forceinline__ void ipm_corr_leg(const double (&u)[3], const double (&ua)[3], const double (&s)[5],
                                             const IS& is, const double (&z)[5], double smu, double mu,
                                             double fzmax, double (&ds)[5], double (&dz)[5], double& amax,
                                             double& dmax) {
    double o[5], oa[5];
    cons_resid(u, mu, fzmax, o);
    cons_resid(ua, mu, fzmax, oa);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double isi = is[i];
        const double dsa = -oa[i] - s[i];
        const double dza = -z[i] - z[i] * isi * dsa;
        ds[i] = -o[i] - s[i];
        dz[i] = (smu - z[i] * s[i] - dsa * dza - z[i] * ds[i]) * isi;
        if (ds[i] < 0.0) amax = fmin(amax, -s[i] * __builtin_amdgcn_rcp(ds[i]));
        if (dz[i] < 0.0) dmax = fmin(dmax, -z[i] * __builtin_amdgcn_rcp(dz[i]));
    }
}

// The two step lengths of the corrector: LMPC_STEP_FRAC of the (wave-wide) distance to the boundary, at most 1
__device__ __forceinline__ double ipm_step_length(double dist) { return fmin(1.0, LMPC_STEP_FRAC * dist); }

// ---- polish verification, one leg-step --------------------------------------------------------------------------

// Gradient of a leg-step's force from the costate: g = Rb u + G0_j' lam (G0_j: columns 3 j .. 3 j + 2 of G0; lam: the six
// velocity costates of the next state); gloc = max(gloc, |g|_inf).  DIAG: Rb = diag(rb[0..2]), else packed.
template <bool DIAG, class PR, class PG, class PL>
__device__ __forceinline__ void leg_gradient(PR rb, const double (&u)[3], PG G0, int j, PL lam, double (&g)[3],
                                             double& gloc) {
    double ru[3];  // input-Hessian block times u
    if constexpr (DIAG) {
#pragma unroll
        for (int p = 0; p < 3; ++p) ru[p] = rb[p] * u[p];
    } else {
        ru[0] = rb[0] * u[0] + rb[1] * u[1] + rb[2] * u[2];
        ru[1] = rb[1] * u[0] + rb[3] * u[1] + rb[4] * u[2];
        ru[2] = rb[2] * u[0] + rb[4] * u[1] + rb[5] * u[2];
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        double v = ru[p];
#pragma unroll
        for (int m = 0; m < 6; ++m) v += G0[m * 12 + 3 * j + p] * lam[m];
        g[p] = v;
        gloc = fmax(gloc, fabs(v));
    }
}

// Primal feasibility of a leg-step's force u: the most violated face outside `act` (by more than tol), or -1
__device__ __forceinline__ int leg_violated(const double (&u)[3], int act, double mu, double fzmax, double tol) {
    double o[5];
    cons_resid(u, mu, fzmax, o);
    int imax = -1;
    double vmax = tol;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (!((act >> i) & 1) && o[i] > vmax) {
            vmax = o[i];
            imax = i;
        }
    return imax;
}

// What the certificate asks of a stance leg-step: `act` after it (changed: it differs), and the stationarity
// residual where the multipliers were formed (0 elsewhere).
struct LegCert {
    bool changed;
    int act;
    double res;
};
// Dual side, at the gradient g (told = tol_d x the gradient scale).  At the apex the cone test is the whole
// certificate (f = 0, every direction bound): a gradient outside the polar cone flips the set to the two faces g points
// out of.  Elsewhere the least-squares multipliers of the active faces (leg_kkt; act = 0: none, the residual is g
// itself): the most negative one below -told is dropped.
__device__ __forceinline__ LegCert leg_certify_dual(const double (&g)[3], int act, bool apex, double mu, double told) {
    LegCert c{false, act, 0.0};
    if (apex) {
        if (g[2] / mu < fabs(g[0]) + fabs(g[1]) - told) {
            c.act = (g[0] < 0.0 ? 2 : 1) | (g[1] < 0.0 ? 8 : 4);
            c.changed = true;
        }
        return c;
    }
    const LegKkt kk = leg_kkt(act, g, mu, -told);
    if (kk.drop >= 0) {
        c.act = act & ~(1 << kk.drop);
        c.changed = true;
    }
    c.res = kk.res;
    return c;
}
// The whole certificate of a stance leg-step: a violated face (by more than tolp) enters first -- the most violated
// one, one per round -- and only a feasible leg-step is asked about its multipliers.
__device__ __forceinline__ LegCert leg_certify(const double (&u)[3], const double (&g)[3], int act, bool apex, double mu,
                                               double fzmax, double tolp, double told) {
    const int imax = leg_violated(u, act, mu, fzmax, tolp);
    if (imax >= 0) return LegCert{true, act | (1 << imax), 0.0};
    return leg_certify_dual(g, act, apex, mu, told);
}

// The retry ladder's step after a polish that did not verify: the next attempt's interior-point stop (retry_tol) and
// iteration budget.  False when the attempts are used up.
__device__ __forceinline__ bool ipm_retry(const DevParams& prm, int& att, double& tol, int& it_end) {
    if (++att >= prm.max_attempts) return false;
    tol = retry_tol(tol, att);
    it_end += prm.max_iter;
    return true;
}

// ---- output ---------------------------------------------------------------------------------------------------------

// A leg's contact-frame force back in the world frame, f = R_j g (flat ground: f = g)
template <bool TERRAIN, class PT>
__device__ __forceinline__ void world_force(PT Rj, const double (&u)[3], double (&fo)[3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p) fo[p] = u[p];
    if constexpr (TERRAIN) {
#pragma unroll
        for (int p = 0; p < 3; ++p) fo[p] = Rj[3 * p] * u[0] + Rj[3 * p + 1] * u[1] + Rj[3 * p + 2] * u[2];
    }
}

// NaN guard (reference: NaN -> zeros, ConvexQPSolver.cpp:321-326) and the forces of the two Riccati kernels' QP
// (lane l owns leg-steps l + 64 t): world frame, zero on swing legs, all zero when any lane holds a NaN.  Returns that
// "any" (wave-uniform; every lane calls it).
template <int LS, bool TERRAIN, class PT>
__device__ __forceinline__ bool qp_store_forces(const bool (&valid)[LS], const bool (&st)[LS], const int (&lsj)[LS],
                                                const double (&u)[LS][3], PT tf, double* __restrict__ gout, int lane) {
    int bad = 0;
#pragma unroll
    for (int t = 0; t < LS; ++t)
        if (valid[t]) bad |= (u[t][0] != u[t][0] || u[t][1] != u[t][1] || u[t][2] != u[t][2]) ? 1 : 0;
    const bool anybad = __any(bad);
#pragma unroll
    for (int t = 0; t < LS; ++t) {
        if (!valid[t]) continue;
        const int ls = lane + 64 * t;
        double fo[3];
        world_force<TERRAIN>(tf + 9 * lsj[t], u[t], fo);
#pragma unroll
        for (int p = 0; p < 3; ++p) gout[3 * ls + p] = (anybad || !st[t]) ? 0.0 : fo[p];
    }
    return anybad;
}

// The QP's status and iteration words (interior-point iterations | polish rounds << 16)
__device__ __forceinline__ void qp_store_words(int32_t* __restrict__ status, int32_t* __restrict__ iters, int qp,
                                               int lane, bool anybad, int qstatus, int ipm_it, int prounds) {
    if (lane == 0) {
        if (status) status[qp] = anybad ? LMPC_QP_NAN : qstatus;
        if (iters) iters[qp] = ipm_it | (prounds << 16);
    }
}

}  // namespace lmpc
