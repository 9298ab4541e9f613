// lmpc_dense_common.h -- the condensed dense path's shared device code (gfx950), used by both
// dense-path kernels: lmpc_dense.hip (interior point + active-set polish on the condensed QP) and
// lmpc_gi.hip (dual active-set / Goldfarb-Idnani on the condensed QP).
//
// Variables of the condensed QP are the stance forces only, laid out 5 leg-steps (15 variables + 1
// padding slot) per 16-wide tile, so every 3x3 leg block sits inside one tile and N <= 64 fits 4x4
// tiles.  The Hessian H is kept in LDS as its upper tiles in the MFMA accumulator layout
// (lane l, register i <-> row (l>>4)+4i, column l&15).  Padding / unused slots carry identity rows.
//
// Prologue (record load, I_w^-1, B = G0, yaw cos/sin, per-leg R blocks; ConvexQPSolver.cpp:198-228)
// and condensation (ConvexQPSolver.cpp:254-313 in condensed form):
//   free response  c_{m+1} = A_m c_m - g dt e11,  c_0 = x0
//   adjoint        mu_m = Q (c_m - xref_{m-1}) + A_m' mu_{m+1}          -> g_i = B' mu_{i+1}
//   cost-to-go     P~_H = Q,  P~_m = Q + A_m' P~_{m+1} A_m
//   Hessian        H[i][j] = B' (A_j ... A_{i+1})' P~_{j+1} B  (i <= j), + R on the diagonal blocks,
//                  one column per lane: L = P~_{j+1} B e_c, then L <- A_{i+1}' L down the steps.
// The first three are not run as recursions (dense_condense).  Every A_m is I + N_m with N_m = dt blkdiag(Rz_m, I)
// from the velocities to the positions and N_j N_k = 0, so A_{n-1} ... A_m = I + N_m + ... + N_{n-1}: c_m, mu_m and
// the columns 6-11 of P~_m are sums over the steps of terms in cos / sin psi_j.  Lane l < H holds step l, and the
// sums are prefix / suffix scans of DPP row 0 (H <= 16).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lmpc/lmpc.h"
#include "lmpc_device.h"
#include "lmpc_kernel_common.h"
#include "lmpc_qp_step.h"

namespace lmpc {

constexpr int DN_TILE = 256;  // doubles per 16x16 tile
size_t dense_lds_bytes(int H);  // host: dynamic LDS of the dense-path carve (lmpc_dense.hip)

// packed index of the upper tile (r, c), r <= c < 4
__device__ __forceinline__ constexpr int tix(int r, int c) { return r * 4 - r * (r - 1) / 2 + (c - r); }
// index of the off-diagonal tile (a, b), a < b < 4
__device__ __forceinline__ constexpr int uix(int a, int b) { return a == 0 ? b - 1 : a == 1 ? b + 1 : 5; }
// element (r, c) of a tile in accumulator order (lane (r&3)*16 + c, register r>>2)
__device__ __forceinline__ int toff(int r, int c) { return (r >> 2) * 64 + (r & 3) * 16 + c; }
// variable of leg-step b, component a
__device__ __forceinline__ int vidx(int b, int a) { return 16 * (b / 5) + 3 * (b % 5) + a; }
// packed symmetric 3x3 [xx xy xz yy yz zz]
__device__ __forceinline__ int sym3(int p, int q) {
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    return lo == 0 ? hi : lo == 1 ? 2 + hi : 5;
}

// acc += X' Y on 16x16 tiles (4 MFMAs); sub: acc -= X' Y
__device__ __forceinline__ d4 tprod(const d4& X, const d4& Y, d4 acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = MFMA64(X[kk], Y[kk], acc);
    return acc;
}
__device__ __forceinline__ d4 tprod_sub(const d4& X, const d4& Y, d4 acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = MFMA64(-X[kk], Y[kk], acc);
    return acc;
}

typedef __attribute__((address_space(3))) int lint;

// sum over the 16 lanes of each DPP row (every lane gets its row's total)
__device__ __forceinline__ double row_sum(double v) {
    v += dpp_f64<DPP_QP_1032>(v);
    v += dpp_f64<DPP_QP_2301>(v);
    v += dpp_f64<DPP_ROR4>(v);
    v += dpp_f64<DPP_ROR8>(v);
    return v;
}

// row_sum of four registers at once (each lane gets all four row totals): a transposing butterfly -- after the
// xor-1 and xor-2 exchanges lane 4q + k holds the quad sum of p[k] only, two rotations finish the row, and a
// quad broadcast per register hands every total back -- 35 instructions instead of four row_sums' 48.
constexpr int DPP_QP_BC0 = 0x00, DPP_QP_BC1 = 0x55, DPP_QP_BC2 = 0xAA, DPP_QP_BC3 = 0xFF;  // quad_perm [k,k,k,k]
__device__ __forceinline__ void row_sum4(const double p[4], double out[4]) {
    const int lane = __lane_id();
    const bool odd = lane & 1, hi2 = lane & 2;
    const double sa = odd ? p[0] : p[1], sb = odd ? p[2] : p[3];
    const double ka = odd ? p[1] : p[0], kb = odd ? p[3] : p[2];
    const double s0 = ka + dpp_f64<DPP_QP_1032>(sa);  // p[lane & 1] over the pair
    const double s1 = kb + dpp_f64<DPP_QP_1032>(sb);  // p[2 + (lane & 1)] over the pair
    const double sc = hi2 ? s0 : s1, kc = hi2 ? s1 : s0;
    double t = kc + dpp_f64<DPP_QP_2301>(sc);          // p[lane & 3] over the quad
    t += dpp_f64<DPP_ROR4>(t);
    t += dpp_f64<DPP_ROR8>(t);                          // ... over the row
    out[0] = dpp_f64<DPP_QP_BC0>(t);
    out[1] = dpp_f64<DPP_QP_BC1>(t);
    out[2] = dpp_f64<DPP_QP_BC2>(t);
    out[3] = dpp_f64<DPP_QP_BC3>(t);
}

// v + v(lane ^ W), W = 16 or 32: v_permlane{16,32}_swap of each dword with a copy of itself returns the lane's own
// and its partner's value in its two outputs (which one is which depends on the half), so their sum needs no select.
// The copy is opaque: with the same value in both operands hipcc (ROCm 7.2) merged the swaps of different
// registers into one (tools/ubench/permlane_probe.hip).
__device__ __forceinline__ unsigned opaque_u32(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <int W>
__device__ __forceinline__ double xor_pair_sum(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    unsigned l0, l1, h0, h1;
    if constexpr (W == 32) {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, opaque_u32(lo), false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, opaque_u32(hi), false, false);
        l0 = l[0]; l1 = l[1]; h0 = h[0]; h1 = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, opaque_u32(lo), false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, opaque_u32(hi), false, false);
        l0 = l[0]; l1 = l[1]; h0 = h[0]; h1 = h[1];
    }
    const double d0 = __builtin_bit_cast(double, ((unsigned long long)h0 << 32) | l0);
    const double d1 = __builtin_bit_cast(double, ((unsigned long long)h1 << 32) | l1);
    return d0 + d1;
}
// sum over the four row groups (lanes c, 16+c, 32+c, 48+c); bitwise the same in all four (fp addition commutes)
__device__ __forceinline__ double group_sum4(double v) { return xor_pair_sum<16>(xor_pair_sum<32>(v)); }

struct DSmem {
    ldouble* hdr;   // 40: x0(12) R(9) feet(12)
    ldouble* G0;    // 72: B rows 6-11 (terrain: G0 blkdiag(R_j))
    ldouble* rb;    // 24: per-leg input Hessian block, packed symmetric
    ldouble* tf;    // 36: terrain frames R_j (row-major)
    ldouble* cs;    // 2H
    ldouble* xr;    // 12H
    ldouble* Ht;    // 10 tiles: upper tiles of H
    ldouble* gv;    // 64: condensed gradient
    ldouble* vec;   // 64: right-hand side in / solution out
    ldouble* vec2;  // 64: matvec operand / result
    ldouble* blk;   // 180: per-leg-step 3x3 block (D in the IPM, T in the polish)
    ldouble* lup;   // 60: polish particular solution up per leg-step (kept out of registers)
    ldouble* lua;   // 64: predictor step u_aff per leg-step (interior point) | the last factorised polish round's
                    //     solution y0 by variable (polish, range-space rounds: lmpc_dense_kernel.h)
    ldouble* lhg;   // 64: H up + g of the last factorised polish round (range-space rounds' new directions)
    ldouble* scr;   // union: condensation: mu by step (96), P~ sums by step (85), the H columns' store sinks (DN_SINK..)
                    //        | diag_inverse: T, W staging (256) W' (272) | h_matvec (48)
                    //        | range-space rounds: h_matvec (48), entries (48..120), solves and column vectors (128..512)
    ldouble* bt;    // 32 x DN_BT_ROW: the leg bases of all 32 face words (basis_table_build, once per QP), row a =
                    //     leg_basis(a): [T0 T1 T3 T4 T6 T7 up0 up1 up2] -- T's third column and the apex flag follow from
                    //     the face word (basis_table_read).  The odd row stride puts the 32 rows' element e on 32 different
                    //     8-byte bank pairs, so lanes reading different face words do not conflict under ds_read_b64
                    //     (two-way at most where the compiler pairs the loads: 32-dword banking) and equal ones broadcast
    lint* lsm;      // 20: stance leg-step b -> 4k + j
    lint* fb;       // H+1: first stance leg-step of step k
};
constexpr int DN_BT_ROW = 9, DN_BT = 32 * DN_BT_ROW;  // the face-set table of leg bases (DSmem::bt)
static_assert(DN_BT_ROW % 2 == 1, "an odd row stride keeps the 32 rows on 32 different 8-byte bank pairs");
constexpr int DN_EL = 16 * 17;               // staging of one 16x16 tile, column stride 17
constexpr int DN_SCR_MIN = 256 + DN_EL;  // diag_inverse: staging of T and W (128 each) | W'
// condensation's sinks: lane l's predicated-off H stores go to DN_SINK + l + {0, 1, 2, 16, 32}, past the step sums
constexpr int DN_SINK = 192;
static_assert(6 * DENSE_MAX_H + 5 * (DENSE_MAX_H + 1) <= DN_SINK && DN_SINK + 63 + 32 < DN_SCR_MIN, "condensation scratch");

typedef double __attribute__((ext_vector_type(2))) dpair;
typedef __attribute__((address_space(3))) dpair lpair;

// DPP row shifts by 1, 2, 4, 8 lanes; a lane whose source lies outside its 16-lane row reads 0 (dpp_f64's bound_ctrl)
constexpr int DPP_ROW_SHL1 = 0x101, DPP_ROW_SHL2 = 0x102, DPP_ROW_SHL4 = 0x104, DPP_ROW_SHL8 = 0x108;  // from lane + n
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;  // from lane - n
// inclusive scans over a 16-lane row: row_prefix sums the lanes up to this one, row_suffix those from this one on
__device__ __forceinline__ double row_prefix(double v) {
    v += dpp_f64<DPP_ROW_SHR1>(v);
    v += dpp_f64<DPP_ROW_SHR2>(v);
    v += dpp_f64<DPP_ROW_SHR4>(v);
    v += dpp_f64<DPP_ROW_SHR8>(v);
    return v;
}
__device__ __forceinline__ double row_suffix(double v) {
    v += dpp_f64<DPP_ROW_SHL1>(v);
    v += dpp_f64<DPP_ROW_SHL2>(v);
    v += dpp_f64<DPP_ROW_SHL4>(v);
    v += dpp_f64<DPP_ROW_SHL8>(v);
    return v;
}

__device__ __forceinline__ DSmem dcarve(double* sm, int H) {
    DSmem s;
    ldouble* p = (ldouble*)sm;
    s.hdr = p; p += 40;
    s.G0 = p; p += 72;
    s.rb = p; p += 24;
    s.tf = p; p += 36;
    s.Ht = p; p += 10 * DN_TILE;
    s.gv = p; p += 64;
    s.vec = p; p += 64;
    s.vec2 = p; p += 64;
    s.blk = p; p += 180;
    s.lup = p; p += 60;
    s.lua = p; p += 64;
    s.cs = p; p += 2 * H;
    s.xr = p; p += 12 * H;
    s.lhg = p; p += 64;
    s.scr = p; p += DN_SCR_MIN;
    s.bt = p; p += DN_BT;
    lint* ip = (lint*)p;
    s.lsm = ip;
    s.fb = ip + 20;
    return s;
}

// ---------------------------------------------------------------------------
// Condensation: g and H (see the header comment).  Lane l < H = step l for the sums over the steps, then
// lane v = variable v.
// ---------------------------------------------------------------------------
#ifdef LMPC_STAMPS
// Diagnostic build only: cycles of the condensation's sub-phases per QP (tools/dense_check.py stamps).
__device__ unsigned long long lmpc_condense_stamps[4096][5];
#define CSTAMP(i) do { const unsigned long long _t = __builtin_readcyclecounter(); \
    if (lane == 0 && blockIdx.x < 4096) lmpc_condense_stamps[blockIdx.x][i] = _t - _cs_t0; _cs_t0 = _t; } while (0)
#define CSTAMP_DECL unsigned long long _cs_t0 = __builtin_readcyclecounter();
#else
#define CSTAMP(i) do {} while (0)
#define CSTAMP_DECL
#endif
// The H-column pass keeps G0's rows 0-2 in registers on flat ground (round 5: H columns 21.3 k -> 17.1 k cycles per
// QP, config 2 -0.7 % against LDS loads in the loop, profiles/r05/border/ab_hoist_g0.log).  Loading the step's yaw
// terms one iteration ahead there did not change its cycles and was not kept.  The sums over the steps and the
// hoisted store bookkeeping: condensation 31.9 k -> 15.2 k cycles per QP (profiles/condense/).
template <bool TERRAIN>
__device__ __forceinline__ void dense_condense(const DevParams& prm, const DSmem& S, int H, int nls,
                                               unsigned long long smask, int lane) {
    const double dt = prm.dt;
    CSTAMP_DECL
    // ---- step lanes: lane l < H holds step l's yaw terms; every sum over the steps is a scan of DPP row 0 ----
    const bool sl = lane < H;
    const int ls = sl ? lane : 0;
    const double ckl = S.cs[2 * ls], skl = S.cs[2 * ls + 1];
    const double ck = sl ? ckl : 0.0, sk = sl ? skl : 0.0;
    // free response: e = Q (c_{l+1} - xref_l) from C, Sn = sums of cos / sin psi over the steps 0..l
    double e[12];
    {
        double x[12], xr[12];
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            x[r] = S.hdr[r];
            xr[r] = S.xr[12 * ls + r];
        }
        const double C = row_prefix(ck), Sn = row_prefix(sk);
        const double n = (double)(lane + 1), gd = prm.grav * dt;
        double c[12];
        c[0] = x[0] + dt * (C * x[6] + Sn * x[7]);
        c[1] = x[1] + dt * (C * x[7] - Sn * x[6]);
        c[2] = x[2] + dt * (n * x[8]);
        c[3] = x[3] + dt * (n * x[9]);
        c[4] = x[4] + dt * (n * x[10]);
        c[5] = x[5] + dt * (n * x[11] - gd * (0.5 * n * (n - 1.0)));  // v_z falls after p_z has used it
        c[6] = x[6];
        c[7] = x[7];
        c[8] = x[8];
        c[9] = x[9];
        c[10] = x[10];
        c[11] = x[11] - n * gd;
#pragma unroll
        for (int r = 0; r < 12; ++r) e[r] = sl ? prm.q[r] * (c[r] - xr[r]) : 0.0;
    }
    CSTAMP(0);  // free response
    // variable of this lane
    const int vt = lane >> 4, vw = lane & 15;
    const int vb = 5 * vt + vw / 3, va = vw % 3;
    const bool vvalid = vw < 15 && vb < nls;
    LMPC_SYNC();
    int vk = 0, vj = 0;
    if (vvalid) {
        const int id = S.lsm[vb];
        vk = id >> 2;
        vj = id & 3;
    }
    const int vc = 3 * vj + va;
    // this variable's column of B (rows 6-11: G0) and its leg's input-Hessian row, loaded once up front (inside the
    // step loops they were loads under divergent branches, each waiting for its own LDS round trip)
    double gc[6], rbl[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) gc[q] = S.G0[q * 12 + vc];
#pragma unroll
    for (int ap = 0; ap < 3; ++ap) rbl[ap] = S.rb[6 * vj + sym3(ap, va)];
    // adjoint: lane l gets mu_{l+1}.  Rows 0-5 are the suffix sums E of e; rows 6-11 the suffix sums of
    // e[6:12] + N_{l+1}' E_{l+2}, whose second term lane l + 1 forms from its own yaw terms and E.
    {
        double E[6], mu[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) E[r] = row_suffix(e[r]);
        double t[6];
        t[0] = dt * (ck * E[0] - sk * E[1]);
        t[1] = dt * (sk * E[0] + ck * E[1]);
        t[2] = dt * E[2];
        t[3] = dt * E[3];
        t[4] = dt * E[4];
        t[5] = dt * E[5];
#pragma unroll
        for (int q = 0; q < 6; ++q) mu[q] = row_suffix(e[6 + q] + dpp_f64<DPP_ROW_SHL1>(t[q]));
        if (lane < DENSE_MAX_H) {
#pragma unroll
            for (int q = 0; q < 6; ++q) S.scr[6 * lane + q] = mu[q];
        }
    }
    CSTAMP(1);  // adjoint
    // ---- cost-to-go without its recursion ----
    // P~_m[:, 6:12] is block diagonal by axis.  Its z and linear entries are polynomials in H - m (taken where the
    // columns start below); the yaw-coupled x, y part of lane l's P~_l is, with rho_j = H - j,
    //   rows 0-1:  dt diag(q0, q1) [uc us; -us uc],  (uc, us) = sum_{j >= l} rho_j (cos, sin) psi_j
    //   rows 6-7:  (H - l + 1) diag(q6, q7) + dt^2 [sa sb; sb sd], the sums over j >= l of step j's
    //              rho_j Rz_j' diag(q0, q1) Rz_j + Rz_j' diag(q0, q1) U_{j+1} + its transpose.
    {
        const double rho = (double)(H - lane), q0 = prm.q[0], q1 = prm.q[1];
        const double uc = row_suffix(rho * ck), us = row_suffix(rho * sk);
        const double un = dpp_f64<DPP_ROW_SHL1>(uc), vn = dpp_f64<DPP_ROW_SHL1>(us);  // U_{l+1}
        const double hc = fma(rho, ck, un + un), hs = fma(rho, sk, vn + vn);
        const double da = q0 * (ck * hc) + q1 * (sk * hs);
        const double dd = q0 * (sk * hs) + q1 * (ck * hc);
        const double db = (q0 - q1) * fma(ck, fma(rho, sk, vn), sk * un);
        const double sa = row_suffix(da), sb = row_suffix(db), sd = row_suffix(dd);
        if (lane <= DENSE_MAX_H) {  // lane H (all zero: P~_H = Q) included
            ldouble* ps = S.scr + 6 * DENSE_MAX_H + 5 * lane;
            ps[0] = uc;
            ps[1] = us;
            ps[2] = sa;
            ps[3] = sb;
            ps[4] = sd;
        }
    }
    CSTAMP(2);  // P~ sums
    // ---- H: zero tiles, identity on padding / unused slots, then one column per lane ----
    {
        lpair* Hz = (lpair*)S.Ht;  // 16-byte stores (the carve keeps Ht 16-byte aligned)
        const dpair zero = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 10 * DN_TILE / 128; ++q) Hz[64 * q + lane] = zero;
    }
    LMPC_SYNC();
    {
        // identity on the diagonal of padding and unused variables (lane v = variable v)
        if (!vvalid) S.Ht[tix(vt, vt) * DN_TILE + toff(vw, vw)] = 1.0;
    }
    {
        // gradient g_v = (B e_v)' mu_{vk+1}, from the step lanes' mu
        const ldouble* mu = S.scr + 6 * vk;
        double gs = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) gs += gc[q] * mu[q];
        S.gv[lane] = vvalid ? gs : 0.0;
    }
    CSTAMP(3);  // H zero + identity, gradient
    {
        // Column v of H (this lane's variable: leg-step vb at step vk, leg vj, component va):
        //   L_i = (A_vk ... A_{i+1})' P~_{vk+1} B e_v for i = vk..0, and H[v'][v] = G0_j'^T L_i[6:12] for the stance
        //   variables v' of step i (+ R on the own 3x3 block).  The step loop is uniform (lanes with vk < i idle):
        //   the stance legs of step i come from the ballot (smask: bit 4k+j) in scalar registers, so no LDS load
        //   (first leg-step of the step, leg of the leg-step) sits ahead of the G0 loads.
        const double dtm = dt / prm.mass;
        const int vkk = vvalid ? vk : -1;  // padding / unused lanes take part in no step
        // Where this lane's stores go, fixed before the loop.  Leg-step bp's three values land in rows 3 (bp % 5)..
        // of tile (bp / 5, vt), a uniform offset on the lane's column pointer; the lane owns them for bp <= lastb
        // (through the last leg-step of its own step, inside its tile row) and mirrors them into its diagonal tile
        // for the mlen leg-steps from mlo on (its tile's leg-steps of earlier steps).  Any other lane stores to a
        // sink word of its own in the scratch: one address select per group of stores, no exec toggling.
        ldouble* const sink = S.scr + DN_SINK + lane;
        ldouble* const dcol = S.Ht + vt * DN_TILE + vw;
        ldouble* const mrow = S.Ht + tix(vt, vt) * DN_TILE + 16 * vw;
        const int mlo = 5 * vt;
        int lastb = -1, mlen = 0;
        if (vvalid) {
            const int f0 = S.fb[vk], f1 = S.fb[vk + 1];
            lastb = min(f1 - 1, mlo + 4);
            mlen = max(f0 - mlo, 0);
        }
        // L = P~_{k+1} B e_v from the sums of the step lanes (k = vk, r = H - 1 - k steps follow step k + 1)
        double L[12];
        {
            const ldouble* ps = S.scr + 6 * DENSE_MAX_H + 5 * (vk + 1);
            const double uc = ps[0], us = ps[1], sa = ps[2], sb = ps[3], sd = ps[4];
            const int r = H - 1 - vk;
            const double cnt = (double)(r + 1);
            const double w1 = (double)(r * (r + 1) / 2);                // sum of n, n = 0..r
            const double w2 = (double)(r * (r + 1) * (2 * r + 1) / 6);  // sum of n^2
            const double dt2 = dt * dt;
            L[0] = dt * prm.q[0] * (uc * gc[0] + us * gc[1]);
            L[1] = dt * prm.q[1] * (uc * gc[1] - us * gc[0]);
            L[6] = fma(cnt, prm.q[6] * gc[0], dt2 * (sa * gc[0] + sb * gc[1]));
            L[7] = fma(cnt, prm.q[7] * gc[1], dt2 * (sb * gc[0] + sd * gc[1]));
            L[2] = dt * prm.q[2] * w1 * gc[2];
            L[8] = fma(cnt, prm.q[8], dt2 * prm.q[2] * w2) * gc[2];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                L[3 + a] = dt * prm.q[3 + a] * w1 * gc[3 + a];
                L[9 + a] = fma(cnt, prm.q[9 + a], dt2 * prm.q[3 + a] * w2) * gc[3 + a];
            }
        }
        // flat ground: rows 0-2 of G0 in registers (loop-invariant; in the loop they are LDS loads the compiler cannot
        // hoist past the H stores, which may alias)
        double g0r[3][12];
        if constexpr (!TERRAIN) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int c = 0; c < 12; ++c) g0r[q][c] = S.G0[q * 12 + c];
        }
        for (int i = H - 1; i >= 0; --i) {
            if (i < vkk) {  // L <- A_{i+1}' L
                const double ck = S.cs[2 * (i + 1)], sk = S.cs[2 * (i + 1) + 1];
                const double l0 = L[0], l1 = L[1], l2 = L[2];
                L[6] += dt * (ck * l0 - sk * l1);
                L[7] += dt * (sk * l0 + ck * l1);
                L[8] += dt * l2;
                L[9] += dt * L[3];
                L[10] += dt * L[4];
                L[11] += dt * L[5];
            }
            const unsigned legs = (unsigned)(smask >> (4 * i)) & 15u;
            if (!legs) continue;  // uniform
            // first stance leg-step of step i, its tile row and slot: counted on from here, no division per leg-step
            int bp = __popcll(smask & ((1ull << (4 * i)) - 1ull));
            int tp = (bp * 13) >> 6, sp = bp - 5 * tp;  // bp / 5 for bp < 64
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                if (!((legs >> jp) & 1u)) continue;  // uniform
                double val[3];
#pragma unroll
                for (int ap = 0; ap < 3; ++ap) {
                    const int cp = 3 * jp + ap;
                    double v = 0.0;
                    if constexpr (TERRAIN) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) v = fma(S.G0[q * 12 + cp], L[6 + q], v);
                    } else {  // flat ground: rows 3-5 of G0 are dt/m I (dense_prologue) -- the same sum, bit for bit
#pragma unroll
                        for (int q = 0; q < 3; ++q) v = fma(g0r[q][cp], L[6 + q], v);
                        v = fma(dtm, L[9 + ap], v);
                    }
                    val[ap] = v;
                }
                // tiles (tp, vt) start 256 (3 tp - tp (tp - 1) / 2) doubles past tile (0, vt): 0, 3, 5, 6 tiles
                const int trow = (int)((0x0600050003000000ull >> (16 * tp)) & 0xffffull);
                ldouble* const pd = bp <= lastb ? dcol + (trow + 48 * sp) : sink;
                pd[0] = val[0];
                pd[16] = val[1];
                pd[32] = val[2];
                ldouble* const pm = (unsigned)(bp - mlo) < (unsigned)mlen ? mrow + 3 * sp : sink;
                pm[0] = val[0];
                pm[1] = val[1];
                pm[2] = val[2];
                ++bp;
                if (++sp == 5) {
                    sp = 0;
                    ++tp;
                }
            }
        }
        // + R on the lane's own 3x3 block (rows vw - va.. of its column in the diagonal tile), once after the loop
        if (vvalid) {
            ldouble* const pr = mrow + (vw - 16 * va);  // element (vw - va, vw)
#pragma unroll
            for (int ap = 0; ap < 3; ++ap) pr[16 * ap] += rbl[ap];
        }
    }
    LMPC_SYNC();
    CSTAMP(4);  // H columns
}

// ---------------------------------------------------------------------------
// Diagonal tile: U_bb^-1 (Ui, = L^-T) and its transpose (UiT, = L^-1) of M_bb = L L'.
// Block Cholesky by leg blocks (3x3 pivots), decoupled identity blocks (unused / padding / apex legs)
// skipped.  amask: coupled blocks (bits 0-4).
//
// The tile T and W = L^-1 (from I) stay in the MFMA accumulator layout (lane 16g + c, register i <->
// element (4i + g, c)).  Per pivot block P = T[o..o+2][o..o+2] (o = 3 blk):
//   the registers holding the three pivot rows of T and W go through LDS once (one write -> read round trip;
//   every lane stores, so the reads have static offsets);
//   every lane factors P = L_p L_p' itself (3 rsq + Newton);
//   lane 16k + m forms L_C[m][k] = (L_p^-1 T[o..o+2][m])_k for the rows m below the pivot (T symmetric)
//   and (L_p^-1 W[o..o+2][c])_k -- the MFMA A and B operands;
//   trailing update T -= L_C L_C' and W -= L_C (L_p^-1 W_p): one v_mfma_f64_16x16x4f64 each (rank 3 of 4);
//   the pivot rows of W become L_p^-1 W_p (Gauss-Jordan on [L | I]: W = L_n^-1 ... L_1^-1 = L^-1).
// Per pivot: 2 MFMAs, one LDS round trip, ~40 VALU -- the row-by-row elimination it replaces (one column
// per lane, three broadcast LDS reads per row and pivot) issued ~5x the LDS reads.
// ---------------------------------------------------------------------------
struct DiagInv {
    d4 ui, uit;
};
// Inlined at its call sites (round 3): outlined, the call cost the caller ~1.7 k cycles per tile in argument /
// result moves and in the caller-saved registers it had to park around the call (5.6 k cycles per tile in the
// kernel vs 3.9 k alone, tools/ubench/diag_parts.hip); inlined, config 2 runs 2 % faster (0.2304 -> 0.2259 ms,
// tools/ab_bench.sh, two alternating runs each; bit-identical results).
static __device__ __attribute__((always_inline)) DiagInv diag_inverse(ldouble* scr, d4 M, int amask, int lane) {
    amask = __builtin_amdgcn_readfirstlane(amask);  // uniform (tile_mask), but arguments arrive in VGPRs
    // staging of the registers that hold the pivot rows (i0, i1): every lane stores its value unconditionally, so
    // row r of register i sits at 16 (r & 3) + c (+64 for i1) -- static read offsets, no per-lane address select
    ldouble* sT = scr;        // 128: T
    ldouble* sW = scr + 128;  // 128: W
    ldouble* tr = scr + 256;  // 16 x 17: transpose staging of W
    const int c = lane & 15, g = lane >> 4;
    d4 T = M, W;
#pragma unroll
    for (int i = 0; i < 4; ++i) W[i] = (4 * i + g == c) ? 1.0 : 0.0;
#pragma unroll
    for (int blk = 0; blk < 5; ++blk) {
        if (!((amask >> blk) & 1)) continue;
        const int o = 3 * blk;
        // rows o..o+2 live in registers i0 = o>>2 and i1 = (o+2)>>2 (static); this lane's row of register i is 4i+g
        const int i0 = o >> 2, i1 = (o + 2) >> 2;
        const int ra = 4 * i0 + g - o, rb = 4 * i1 + g - o;
        const bool ina = ra >= 0 && ra < 3, inb = i1 != i0 && rb >= 0 && rb < 3;
        // staging offset of pivot row o+a (static)
        auto so = [&](int a) { return ((o + a) >> 2 == i0 ? 0 : 64) + 16 * ((o + a) & 3); };
        LMPC_SYNC();
        // publish the registers of T first: the T chain of this pivot waits only for the previous T update
        sT[lane] = T[i0];
        if (i1 != i0) sT[64 + lane] = T[i1];
        LMPC_SYNC();
        const double p00 = sT[so(0) + o], p10 = sT[so(1) + o], p11 = sT[so(1) + o + 1];
        const double p20 = sT[so(2) + o], p21 = sT[so(2) + o + 1], p22 = sT[so(2) + o + 2];
        const double t0 = sT[so(0) + c], t1 = sT[so(1) + c], t2 = sT[so(2) + c];  // T[o+a][c] = T[c][o+a]
        // then those of W, read while the pivot is factored; W's pivot rows are cleared so the MFMA below writes
        // L_p^-1 W_p into them
        sW[lane] = W[i0];
        if (i1 != i0) sW[64 + lane] = W[i1];
        W[i0] = ina ? 0.0 : W[i0];
        if (i1 != i0) W[i1] = inb ? 0.0 : W[i1];
        LMPC_SYNC();
        const double w0 = sW[so(0) + c], w1 = sW[so(1) + c], w2 = sW[so(2) + c];  // W[o+a][c]
        // P = L_p L_p' with the three pivot reciprocals from the leading minors, so their rsq chains run side by
        // side instead of one after the other: d1 = m11 / p00, d2 = det / m11 (m11 = p00 p11 - p10^2), hence
        // 1/sqrt(d1) = sqrt(p00) rsq(m11) and 1/sqrt(d2) = sqrt(m11) rsq(det).  (The pivots one after another: 12
        // fewer fp64 instructions, two more rsq latencies on the chain, 1.5 % slower on the dual active set -- DESIGN.md
        // 4b, v19.)
        const double m11 = fma(p00, p11, -p10 * p10);
        const double c00 = fma(p11, p22, -p21 * p21), c01 = fma(p10, p22, -p21 * p20), c02 = fma(p10, p21, -p11 * p20);
        const double det = fma(p00, c00, fma(-p10, c01, p20 * c02));
        const double i00 = rsq_nr(p00), r1 = rsq_nr(m11), r2 = rsq_nr(det);
        const double l10 = p10 * i00, l20 = p20 * i00;
        const double i11 = (p00 * i00) * r1;
        const double l21 = fma(-l20, l10, p21) * i11;
        const double i22 = (m11 * r1) * r2;
        // row c of L_C (zero in and above the pivot rows)
        const double x0 = t0 * i00;
        const double x1 = fma(-l10, x0, t1) * i11;
        const double x2 = fma(-l21, x1, fma(-l20, x0, t2)) * i22;
        const double xs = g == 0 ? x0 : g == 1 ? x1 : x2;
        const double av = (c > o + 2 && g < 3) ? xs : 0.0;
        // column c of L_p^-1 W_p
        const double v0 = w0 * i00;
        const double v1 = fma(-l10, v0, w1) * i11;
        const double v2 = fma(-l21, v1, fma(-l20, v0, w2)) * i22;
        const double vs = g == 0 ? v0 : g == 1 ? v1 : v2;
        const double bv = g < 3 ? vs : 0.0;
        // W's A operand: -L_C below the pivot, the unit rows of the pivot block (W_new pivot rows = L_p^-1 W_p)
        const bool cp = c >= o && c <= o + 2;
        const double aw = cp ? (g == c - o ? 1.0 : 0.0) : -av;
        T = MFMA64(-av, av, T);
        W = MFMA64(aw, bv, W);
    }
    // W = L^-1 (lower triangular): uit = W; ui = W' through LDS (column stride 17: distinct banks)
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[c * 17 + 4 * i + g] = W[i];
    LMPC_SYNC();
    DiagInv out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out.uit[i] = W[i];
        out.ui[i] = tr[(4 * i + g) * 17 + c];
    }
    return out;
}

// ---------------------------------------------------------------------------
// diag_inverse with T and W in one tile, for the interior-point / polish kernel (lmpc_dense_kernel.h); bit for bit
// diag_inverse's results.  At pivot block o the trailing update of T touches columns > o+2 only and that of W
// columns <= o+2 only (W = L^-1 is lower triangular and its rows from o on are still those of I to the right of
// column o-1), so one tile X holds both -- columns that have had their pivot are W's, the others T's -- and one MFMA
// updates both: its A operand is W's (-L_C below the pivot, unit rows in it), its B operand row c of L_C where
// column c is still T's and column c of L_p^-1 W_p where it is W's, W_p = I on the pivot columns themselves.  Every
// element sees the products it saw in its own tile.  Per pivot that is one MFMA, one LDS round trip and one
// substitution chain instead of two of each: a lone wave pays ~80 cycles per fp64 MFMA and the fp64 VALU does not
// run beside it (profiles/r01_ubench_latency.log, profiles/overlap/), so the second MFMA was pure chain length.
// What the shared tile costs: the pivot columns are cleared with the pivot rows ahead of the MFMA (T's entries
// there are spent, W's start from zero), and the pivot rows collect L_C' to the right of the pivot -- the strict
// upper triangle is zeroed once at the end.  The dual active set (lmpc_gi.hip) keeps diag_inverse.
// ---------------------------------------------------------------------------
static __device__ __attribute__((always_inline)) DiagInv diag_inverse_merged(ldouble* scr, d4 M, int amask, int lane) {
    amask = __builtin_amdgcn_readfirstlane(amask);  // uniform (tile_mask), but arguments arrive in VGPRs
    ldouble* sX = scr;        // 128: staging of the registers that hold the pivot rows (as in diag_inverse)
    ldouble* tr = scr + 256;  // 16 x 17: transpose staging of W
    const int c = lane & 15, g = lane >> 4;
    d4 X = M;
#pragma unroll
    for (int blk = 0; blk < 5; ++blk) {
        if (!((amask >> blk) & 1)) continue;
        const int o = 3 * blk;
        const int i0 = o >> 2, i1 = (o + 2) >> 2;
        const int ra = 4 * i0 + g - o, rb = 4 * i1 + g - o;
        const bool ina = ra >= 0 && ra < 3, inb = i1 != i0 && rb >= 0 && rb < 3;
        const bool cp = c >= o && c <= o + 2;  // a pivot column
        auto so = [&](int a) { return ((o + a) >> 2 == i0 ? 0 : 64) + 16 * ((o + a) & 3); };
        LMPC_SYNC();
        sX[lane] = X[i0];
        if (i1 != i0) sX[64 + lane] = X[i1];
        // the pivot rows and columns start from zero: the MFMA below writes L_p^-1 W_p into the rows and W's new
        // columns -L_C L_p^-1 under the pivot
#pragma unroll
        for (int i = 0; i < 4; ++i) X[i] = (cp || (i == i0 && ina) || (i == i1 && inb)) ? 0.0 : X[i];
        LMPC_SYNC();
        const double p00 = sX[so(0) + o], p10 = sX[so(1) + o], p11 = sX[so(1) + o + 1];
        const double p20 = sX[so(2) + o], p21 = sX[so(2) + o + 1], p22 = sX[so(2) + o + 2];
        // row o+a at this lane's column: T[o+a][c] = T[c][o+a] right of the pivot, W[o+a][c] left of it
        const double r0 = sX[so(0) + c], r1 = sX[so(1) + c], r2 = sX[so(2) + c];
        // P = L_p L_p' (diag_inverse's arithmetic)
        const double m11 = fma(p00, p11, -p10 * p10);
        const double c00 = fma(p11, p22, -p21 * p21), c01 = fma(p10, p22, -p21 * p20), c02 = fma(p10, p21, -p11 * p20);
        const double det = fma(p00, c00, fma(-p10, c01, p20 * c02));
        const double i00 = rsq_nr(p00), q1 = rsq_nr(m11), q2 = rsq_nr(det);
        const double l10 = p10 * i00, l20 = p20 * i00;
        const double i11 = (p00 * i00) * q1;
        const double l21 = fma(-l20, l10, p21) * i11;
        const double i22 = (m11 * q1) * q2;
        // L_p^-1 applied to this lane's column of the pivot rows (W_p = I on the pivot columns): row c of L_C right of
        // the pivot, column c of L_p^-1 W_p from the pivot leftwards
        const double s0 = cp ? (c == o ? 1.0 : 0.0) : r0;
        const double s1 = cp ? (c == o + 1 ? 1.0 : 0.0) : r1;
        const double s2 = cp ? (c == o + 2 ? 1.0 : 0.0) : r2;
        const double y0 = s0 * i00;
        const double y1 = fma(-l10, y0, s1) * i11;
        const double y2 = fma(-l21, y1, fma(-l20, y0, s2)) * i22;
        const double ys = g == 0 ? y0 : g == 1 ? y1 : y2;
        const double bv = g < 3 ? ys : 0.0;
        const double av = c > o + 2 ? bv : 0.0;
        const double aw = cp ? (g == c - o ? 1.0 : 0.0) : -av;
        X = MFMA64(aw, bv, X);
    }
    // W = L^-1 is X's lower triangle: uit = W; ui = W' through LDS (column stride 17: distinct banks)
    d4 W;
#pragma unroll
    for (int i = 0; i < 4; ++i) W[i] = 4 * i + g >= c ? X[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[c * 17 + 4 * i + g] = W[i];
    LMPC_SYNC();
    DiagInv out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out.uit[i] = W[i];
        out.ui[i] = tr[(4 * i + g) * 17 + c];
    }
    return out;
}


// Coupled-block masks of a factorisation's four tiles, computed once ahead of the tile loop: bit b = leg-step b is
// valid (b < nls) and coupled (bit b of `coupled`: all ones in the interior point and the dual active set, the
// ballot of T != 0 in a polish round).  Scalar: nothing is loaded or waited on between the tiles.
__device__ __forceinline__ unsigned tile_masks(int nls, unsigned coupled) {
    return __builtin_amdgcn_readfirstlane(((1u << nls) - 1u) & coupled);  // nls <= DENSE_MAX_LS = 20
}
// mask of tile t (bits 0-4: leg-steps 5t..5t+4)
__device__ __forceinline__ int tile_mask(unsigned masks, int t) { return (int)((masks >> (5 * t)) & 31u); }

// lane-wise y = H x for the variables (lane v = variable v; x in LDS by variable), H from its upper tiles in LDS,
// as VALU tile products in the accumulator layout (lane 16g + c, register i <-> tile element (4i + g, c)):
//   y_t gets T_rt' x_r for r <= t (the stored tile and the diagonal one): lane 16g + c sums T_rt[4i+g][c] x_r[4i+g]
//       over its rows, then over the four row groups -> column-indexed (group_sum4);
//   y_t gets T_tc x_c for c > t: lane 16g + c sums T_tc[4i+g][c] x_c[c] per register, then over its 16-lane row
//       (row_sum) -> row-indexed, handed to lane order through tmp (64 doubles of LDS).
// All loads are independent (one batch); until round 2 every lane walked its row of H with 64 dependent steps.
__device__ __forceinline__ double h_matvec(const DSmem& S, const ldouble* x, ldouble* tmp, int lane) {
    const int lc = lane & 15, lr = lane >> 4;
    double xr[4][4], xc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[b][i] = x[16 * b + 4 * i + lr];
        xc[b] = x[16 * b + lc];
    }
    double pc[4] = {0.0, 0.0, 0.0, 0.0};
    double pr[3][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = r; c < 4; ++c) {
            const int k = tix(r, c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double h = S.Ht[k * DN_TILE + i * 64 + lane];
                pc[c] = fma(h, xr[r][i], pc[c]);
                if (c > r) pr[r][i] = fma(h, xc[c], pr[r][i]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double rs[4];
        row_sum4(pr[r], rs);
        if (lc == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) tmp[16 * r + 4 * i + lr] = rs[i];
        }
    }
    double yc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) yc[c] = group_sum4(pc[c]);
    LMPC_SYNC();
    const double ys = lr == 0 ? yc[0] : lr == 1 ? yc[1] : lr == 2 ? yc[2] : yc[3];
    return ys + (lr < 3 ? tmp[lane < 48 ? lane : 0] : 0.0);
}

// lane v's element of H e for a vector e supported on leg-step b (components e3): the three elements H[v][w] of b's
// variables w, three loads and three FMAs instead of h_matvec's whole product.  Row tiles up to b's tile hold the
// element itself (the diagonal tiles are stored in full), the row tiles below it the transposed element of tile
// (tw, tv).  Padding / unused lanes get 0 (their rows are identity rows).
__device__ __forceinline__ double h_col3(const DSmem& S, int b, const double (&e3)[3], int lane) {
    const int tv = lane >> 4, vw = lane & 15;
    const int tw = b / 5, sw = 3 * (b - 5 * tw);
    const bool up = tv <= tw;
    const ldouble* T = S.Ht + (up ? tix(tv, tw) : tix(tw, tv)) * DN_TILE;
    double h = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) h = fma(T[up ? toff(vw, sw + q) : toff(sw + q, vw)], e3[q], h);
    return h;
}

// ---------------------------------------------------------------------------
// Prologue: record -> LDS, stance leg-step map (lsm, fb), terrain frames, I_w^-1, G0 = B rows 6-11,
// yaw cos/sin of every step, per-leg input Hessian blocks.  smask = ballot of stance leg-steps
// (lane 4k + j).  Returns this lane's rank among the stance leg-steps (valid when stl).
// ---------------------------------------------------------------------------
// The QP's record (33 + 12 H <= 4 x 64 doubles) in flight: lane l's elements l, l + 64, ...  Issued right after the
// contact bytes' load and ahead of the wait on them -- its address does not depend on the contacts, so the two global
// round trips at the head of the QP overlap.  A QP that leaves for the Riccati body drops the values.
struct DenseRec {
    double v[4];
};
static_assert(33 + 12 * DENSE_MAX_H <= 4 * 64, "DenseRec holds a whole record");
__device__ __forceinline__ DenseRec dense_rec_load(const double* __restrict__ rec, int qp, int H, int lane) {
    const int RL = 33 + 12 * H;
    const double* rin = rec + (size_t)qp * RL;
    DenseRec r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        r.v[q] = rin[i < RL ? i : 0];
    }
    return r;
}

template <bool TERRAIN>
__device__ __forceinline__ int dense_prologue(const DevParams& prm, const DSmem& S, const DenseRec& rv,
                                              const double* __restrict__ normals, int qp, int H,
                                              unsigned long long smask, bool stl, int lane) {
    const int RL = 33 + 12 * H;
    const double dt = prm.dt;
    // ---- record, leg-step map ----
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        if (i < 33) S.hdr[i] = rv.v[q];
        else if (i < RL) S.xr[i - 33] = rv.v[q];
    }
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(smask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)smask, 0));
    if (stl) S.lsm[rank] = lane;
    if (lane <= H) {
        // first stance leg-step of step `lane` = stance leg-steps with 4k + j < 4 lane
        const unsigned long long below = (lane >= 16) ? smask : (smask & ((1ull << (4 * lane)) - 1ull));
        S.fb[lane] = __popcll(below);
    }
    if (TERRAIN && lane < 4) {
        double R[9];
        terrain_frame(normals + (size_t)qp * 12 + 3 * lane, R);
#pragma unroll
        for (int e = 0; e < 9; ++e) S.tf[9 * lane + e] = R[e];
    }
    LMPC_SYNC();
    double iw[9];
    world_inertia_inv(S.hdr + LMPC_REC_ROT, prm.Ib, iw);
    yaw_cos_sin(S.xr, S.cs, H, lane);
    for (int e = lane; e < 72; e += 64) {
        const int r = e / 12;
        S.G0[e] = g0_entry<TERRAIN>(prm, e, iw[r * 3 + 0], iw[r * 3 + 1], iw[r * 3 + 2], S.hdr, S.tf);
    }
    if (lane < 4) {
        const double r0 = prm.r[3 * lane], r1 = prm.r[3 * lane + 1], r2 = prm.r[3 * lane + 2];
        if constexpr (TERRAIN) {
            rotated_weights(prm.r + 3 * lane, S.tf + 9 * lane, S.rb + 6 * lane);
        } else {
            S.rb[6 * lane + 0] = r0;
            S.rb[6 * lane + 1] = 0.0;
            S.rb[6 * lane + 2] = 0.0;
            S.rb[6 * lane + 3] = r1;
            S.rb[6 * lane + 4] = 0.0;
            S.rb[6 * lane + 5] = r2;
        }
    }
    S.vec[lane] = 0.0;
    S.vec2[lane] = 0.0;
    LMPC_SYNC();

    return rank;
}

}  // namespace lmpc
