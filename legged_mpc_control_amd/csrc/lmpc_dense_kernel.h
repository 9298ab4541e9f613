// lmpc_dense_kernel.h -- the condensed dense path's per-QP solve (dense_body), shared by the dense kernel
// (lmpc_dense.hip) and the fused dense + Riccati kernel (lmpc_lq.hip).  The algorithm is described at the top of
// lmpc_dense.hip.  The diagnostic hooks (DSTAMP*, LMPC_KKT_DIAG) are those of lmpc_dense.hip, which defines them
// before including this header; elsewhere they compile to nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "lmpc/lmpc.h"
#include "lmpc_device.h"
#include "lmpc_kernel_common.h"
#include "lmpc_qp_step.h"
#include "lmpc_dense_common.h"

#ifndef DSTAMP
#define DS_PARAMS
#define DS_ARGS
#define DSTAMP_DECL
#define DSTAMP(i) do {} while (0)
#define DSTAMP_FLUSH(qp) do {} while (0)
#endif

// Range-space (Schur complement) polish rounds after a factorised one (dense_body): 1 on, 0 every round refactors
// (the test-only "noschur" build, tests/test_gpu_kkt.py)
#ifndef LMPC_POLISH_SCHUR
#define LMPC_POLISH_SCHUR 1
#endif

namespace lmpc {

// A range-space round adds face rows and, where it drops factorised faces, new columns (the bordered system),
// LMPC_SCHUR_KMAX entries at most.  Cost rule in half-units of one solve: 2 per entry, LMPC_SCHUR_SLOPE2 per diagonal
// tile a refactorisation would keep, at most LMPC_SCHUR_LIM2 (config 2 0.1827 -> 0.1731 ms against accepting every
// qualifying round; rows-only rounds and a further charge per column's matvec were tried and dropped: DESIGN.md,
// "Experiments removed from the source").  Slope 4 / limit 10 priced a round with a full matvec per column and a
// padded 6 x 6 K; with the columns from h_col3 and K at its own size 3 / 11 is the fastest of the grid in
// profiles/schur/ (config 2 0.1468 -> 0.1397 ms, 0.1446 at 4 / 10; 2 / 12, 2 / 14, 3 / 14 and 0 / 12 are slower).
constexpr int LMPC_SCHUR_KMAX = 6;
constexpr int LMPC_SCHUR_SLOPE2 = 3;
constexpr int LMPC_SCHUR_LIM2 = 11;
// interior-point start: z = LMPC_DENSE_Z0 / s (complementarity LMPC_DENSE_Z0 per pair); 0.3 and 3 ran config 2 in
// 0.212 / 0.201 ms against 0.174 (profiles/r05, ab_z0.log)
constexpr double LMPC_DENSE_Z0 = 1.0;
// A verified range-space round whose stationarity residual is above LMPC_REFINE_SR of the gradient scale takes one
// step of iterative refinement and is certified again (round 6).  Over 8192 config-2 QPs (tools/refine_diag.py,
// profiles/r06/refine/) 1857 end on a range-space round; their residuals are <= 6.2e-13 of gscale except one at
// 3.4e-12 -- the QP whose forces sat 1.8e-9 from the optimum (the others' corrections <= 3e-10).  Refining every such
// QP cost config 2 +3.4 %; this trigger refines that one.  tools/refine_diag.py's build refines every round.
#ifdef LMPC_REFINE_DIAG
constexpr double LMPC_REFINE_SR = 0.0;
#else
constexpr double LMPC_REFINE_SR = 1e-12;
#endif

// range-space rounds' scratch (S.scr): h_matvec 0..47, entries U / uleg / utyp / Cb 48..119, the round's s 120..125
// (for its refinement) and K's smallest pivot ratio 126, W = M^-1 V and the columns' V from 128
static_assert(48 + 4 * LMPC_SCHUR_KMAX + 2 * LMPC_SCHUR_KMAX + LMPC_SCHUR_KMAX * LMPC_SCHUR_KMAX <= 120 &&
                  120 + LMPC_SCHUR_KMAX + 1 <= 128, "range-space scratch layout");
constexpr int DN_SCHUR_SV = 120;

// Leg bases from the QP's face-set table (DSmem::bt): 1 on, 0 every reader calls leg_basis (the test-only
// "basisdirect" build, tests/test_gpu_basis_table.py)
#ifndef LMPC_BASIS_TABLE
#define LMPC_BASIS_TABLE 1
#endif

// The face-set table of leg bases.  leg_basis is a function of the 5-bit face word and the context's (mu, f_max)
// alone, and a lone wave pays its five IEEE 1/sqrt (~3.5 k cycles) whenever one lane calls it; dense_body called it
// once in every polish round and once more in every range-space round.  Lane a < 32 evaluates leg_basis(a) once per
// QP -- the function itself, so a row holds the bits a call returns -- and the rounds read their rows from LDS.
__device__ __forceinline__ void basis_table_build(ldouble* bt, double mu, double fzmax, int lane) {
    if (lane < 32) {
        double T[9], up[3];
        (void)leg_basis(lane, mu, fzmax, T, up);
        ldouble* r = bt + DN_BT_ROW * lane;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            r[2 * p] = T[3 * p];
            r[2 * p + 1] = T[3 * p + 1];
            r[6 + p] = up[p];
        }
    }
}
// leg_basis(act, ...) from the table.  Not stored: T's third column, which leg_basis fills only for act = 0 (the
// identity), and the apex flag.
__device__ __forceinline__ bool basis_table_read(const ldouble* bt, int act, double T[9], double up[3]) {
    const int a = act & 31;
    const ldouble* r = bt + DN_BT_ROW * a;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        T[3 * p] = r[2 * p];
        T[3 * p + 1] = r[2 * p + 1];
        T[3 * p + 2] = 0.0;
        up[p] = r[6 + p];
    }
    T[8] = a == 0 ? 1.0 : 0.0;
    return (a & 3) == 3 || (a & 12) == 12;
}
// the rounds' leg basis: the table's row, or in the "basisdirect" build the call it replaces
__device__ __forceinline__ bool dense_leg_basis(const DSmem& S, int act, double mu, double fzmax, double T[9],
                                                double up[3]) {
#if LMPC_BASIS_TABLE
    (void)mu, (void)fzmax;
    return basis_table_read(S.bt, act, T, up);
#else
    (void)S;
    return leg_basis(act, mu, fzmax, T, up);
#endif
}

// nonzero columns of a leg basis (leg_basis puts them first)
template <typename P>
__device__ __forceinline__ int ncols3(const P* T) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) n += (T[q] != 0.0 || T[3 + q] != 0.0 || T[6 + q] != 0.0) ? 1 : 0;
    return n;
}
// sum over the wave of k in 0..7, and its exclusive prefix (lanes in `below`)
__device__ __forceinline__ int wave_count3(int k) {
    return __popcll(__ballot(k & 1)) + 2 * __popcll(__ballot(k & 2)) + 4 * __popcll(__ballot(k & 4));
}
__device__ __forceinline__ int wave_prefix3(int k, unsigned long long below) {
    return __popcll(__ballot(k & 1) & below) + 2 * __popcll(__ballot(k & 2) & below) +
           4 * __popcll(__ballot(k & 4) & below);
}

// One leg-step of a range-space polish round (dense_body): faces act (nap: an apex) against the factorised round's
// bact.  The kept faces cm = act & bact leave nc free directions,
// nb of them the factorised ones: kc = nc - nb new columns, kr rows (the added faces, each removing one free
// direction, or at a new apex the nc rows u = 0).  ok = false: the round refactorises.
struct SchurLeg {
    int kc, kr;
    bool ok;
};
// The counts come from the face words alone: leg_basis leaves no free direction at an apex and otherwise three less
// one per active face (its T has exactly that many nonzero columns), so no basis is built to evaluate the cost rule --
// a leg_basis (five IEEE 1/sqrt, ~3.5 k cycles of a lone wave) less in every polish round after the first.
__device__ __forceinline__ int leg_free(int a) { return ((a & 3) == 3 || (a & 12) == 12) ? 0 : 3 - __popc(a & 31); }
__device__ __forceinline__ SchurLeg schur_leg(bool chg, int act, int bact, bool nap) {
    SchurLeg r{0, 0, true};
    if (!chg) return r;
    const bool bap = (bact & 3) == 3 || (bact & 12) == 12;
    if (bap && nap) return r;  // the force stays zero
    const int cm = act & bact;
    const int nb = leg_free(bact), nc = leg_free(cm), nn = leg_free(act);
    r.kc = nc - nb;
    r.kr = nap ? nc : __popc(act & ~bact);
    // the factorised particular solution must lie in the kept space: no f_max face at an apex on either side
    r.ok = r.kc >= 0 && r.kc <= 3 && r.kr <= 3 && (!bap || !(cm & 16)) && (!nap || !((act | bact) & 16)) &&
           (nap || nn == nc - r.kr);
    return r;
}

// ---------------------------------------------------------------------------
// The dense-path solve of QP blockIdx.x, one wave.  Returns false for a QP it leaves to the Riccati kernel (more
// than 20 stance leg-steps, none, or no verified optimum: done_out[qp] = 0, nothing written), true otherwise.
// lmpc_dense_kernel (lmpc_dense.hip) runs it alone; lmpc_dense_lq_kernel (lmpc_lq.hip) runs the Riccati solve
// after it in the same wave where it returns false (one launch instead of two at one QP per SIMD).
// ---------------------------------------------------------------------------
template <bool TERRAIN>
__device__ __forceinline__ bool dense_body(const DevParams prm, const double* __restrict__ rec,
                                           const uint8_t* __restrict__ contact, const double* __restrict__ normals,
                                           int batch, double* __restrict__ grf, int32_t* __restrict__ status,
                                           int32_t* __restrict__ iters, uint8_t* __restrict__ done_out) {
    extern __shared__ __attribute__((aligned(16))) double dn_smem[];
    const int qp = blockIdx.x;
    if (qp >= batch) return true;
    const int lane = threadIdx.x;
    const int H = prm.H;
    // ---- stance leg-steps: ballot over lane i = 4k + j ----
    const uint8_t cbyte = contact[(size_t)qp * 4 * H + (lane < 4 * H ? lane : 0)];
    const DenseRec rv = dense_rec_load(rec, qp, H, lane);  // in flight while the contact bytes are waited on
    const bool stl = lane < 4 * H && cbyte != 0;
    const unsigned long long smask = __ballot(stl);
    const int nls = __popcll(smask);
    if (nls > DENSE_MAX_LS || nls == 0) return false;  // Riccati kernel (it also owns the all-swing QPs)
    const DSmem S = dcarve(dn_smem, H);
    const double mu = prm.mu, fzmax = prm.fmax, dt = prm.dt;
    DSTAMP_DECL

    const int rank = dense_prologue<TERRAIN>(prm, S, rv, normals, qp, H, smask, stl, lane);
    DSTAMP(0);  // prologue
    dense_condense<TERRAIN>(prm, S, H, nls, smask, lane);
    // Always four tiles: leg-steps beyond nls are identity padding (exact, and it keeps every tile
    // index static, so register liveness is exact across the predictor / corrector solves).
    constexpr int NT = 4;
    DSTAMP(1);  // condensation

    // ---- leg-step state: lane b = stance leg-step b ----
    const bool st = lane < nls;
    int lk = 0, lj = 0;
    if (st) {
        const int id = S.lsm[lane];
        lk = id >> 2;
        lj = id & 3;
    }
    double f[3], s[5], z[5], is[5];  // is = 1/s, refreshed whenever s changes (used 4x per iteration)
    {
        const double cnt = st ? (double)(S.fb[lk + 1] - S.fb[lk]) : 1.0;  // stance legs of this leg-step's stage
        ipm_start(st, cnt, prm.mass * prm.grav, mu, fzmax, f, s, is);  // is = 1/s: the centred z
#pragma unroll
        for (int i = 0; i < 5; ++i) z[i] = LMPC_DENSE_Z0 * is[i];
    }
    double u[3] = {0.0, 0.0, 0.0}, rt[3] = {0.0, 0.0, 0.0};
    int qstatus = LMPC_QP_CONVERGED, ipm_it = 0, prounds = 0;
    bool done = false;
    enum { PRED = 0, CORR = 1, POLISH = 2 };
    const double mc = 5.0 * nls, imc = 1.0 / mc;  // complementarity pairs
    double tol = prm.tol_mu;
    // first attempt: at most dense_polish_iter interior-point iterations before the polish (the polish verifies
    // the optimum exactly; a failed polish resumes the interior point with a tighter tolerance below)
    int att = 0, rd = 0, it_end = min(prm.max_iter, prm.dense_polish_iter), mode = PRED, act = 0;
    // polish rounds after a polish round: diagonal tiles before the first leg-step whose active set changed keep their
    // factors (their M tiles, and every panel and update feeding them, are bitwise those of the previous round)
    int keep_tiles = 0;
    // coupled leg-steps (T != 0) of the current factorised polish round: bit b = leg-step b (uniform)
    unsigned cmask = 0;
    bool apex = false;
#if LMPC_BASIS_TABLE
    // the face-set table is built at the QP's first polish round: at the top of the body, behind the contact-byte and
    // record loads, or after the hand-over test the launch was 0.6-0.9 % slower ("Leg bases from a
    // face-set table"; profiles/basis_table/ab_place.log)
    bool bt_built = false;
#endif
    // Range-space polish rounds (LMPC_POLISH_SCHUR): a round whose active set only adds faces to the set of the last
    // factorised round (bact, per leg-step lane) is that round's equality QP with k more rows A y = d on its
    // coordinates y, so y = y0 - M^-1 A' (A M^-1 A')^-1 (A y0 - d) from the factorisation in hand: k + 1 solves and
    // a k x k Cholesky instead of T'HT, its tiled Cholesky and one solve (tools/polish_schur_proto.py: 113 of 143
    // later rounds qualify on config 2).  The verification below is the same either way.
    int bact = 0;
    bool have_base = false, schur = false;
    int nsch = 0, ncol = 0;  // range-space entries (columns + rows) and columns of the current round
    double mu_c = 0.0, smu = 0.0, sz = 0.0;  // sz = sum of s'z at the iterate (mu_c = sz / mc)
    // factor tiles (register resident through the corrector): U's off-diagonal tiles in Tl, U_bb^-1, U_bb^-T
    d4 Tl[10], Ui[4], UiT[4];
    const int lc = lane & 15, lr = lane >> 4;
    // Diagonal-tile elements inside a 3x3 leg block: lane 16 lr + lc holds rows lr + 4i of column lc, and at most one
    // of them (register lblk_reg, -1 if none) lies in lc's block (rows 3 lblk_q .. 3 lblk_q + 2); lblk_off is its
    // offset in the leg-step's 9-entry block of S.blk
    int lblk_reg = -1, lblk_q = 0, lblk_off = 0, ldg_reg = -1;  // ldg_reg: the register holding element (lc, lc)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = lr + 4 * i;
        if (r < 15 && lc < 15 && r / 3 == lc / 3) {
            lblk_reg = i;
            lblk_q = r / 3;
            lblk_off = 3 * (r % 3) + lc % 3;
            if (r == lc) ldg_reg = i;
        }
    }
#if LMPC_POLISH_SCHUR
    // K s = cv of a range-space round (S.scr: entries U / uleg / utyp / Cb, W = M^-1 V in Wc; every lane alike):
    // K = Cb - V'W, rows by their three entries; L D L' without pivoting (K is quasi-definite: columns +, rows -),
    // unrolled to the round's own size (sv beyond it: 0).  Returns true (bad) when a pivot leaves its sign:
    // rank-deficient in rounding.
    auto schur_ksolve_n = [&](auto nc, const double (&cv)[LMPC_SCHUR_KMAX], double (&sv)[LMPC_SCHUR_KMAX],
                              double& kmin) -> bool {
        constexpr int KM = LMPC_SCHUR_KMAX;
        constexpr int N = decltype(nc)::value;  // = nsch: K at its own size, no padding formed
        const ldouble* U = S.scr + 48;
        const ldouble* uleg = U + 4 * KM;
        const ldouble* utyp = uleg + KM;
        const ldouble* Cb = utyp + KM;
        const ldouble* Wc = S.scr + 128;
        double Am[N][N], sg[N];
        int rb_[N];
        bool rw[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            rw[i] = utyp[i] < 0.5;
            rb_[i] = (int)uleg[i];
            sg[i] = rw[i] ? -1.0 : 1.0;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double v = Cb[KM * i + j];
                if (rw[i]) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) v = fma(-U[4 * i + q], Wc[64 * j + vidx(rb_[i], q)], v);
                } else if (rw[j]) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) v = fma(-U[4 * j + q], Wc[64 * i + vidx(rb_[j], q)], v);
                }
                Am[i][j] = v;
            }
        }
        bool bad = false;
        double dd[N];
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double d = Am[c][c];
#pragma unroll
            for (int b = 0; b < c; ++b) d = fma(-Am[c][b], Am[c][b] * dd[b], d);
            bad |= !(sg[c] * d > 1e-14 * fabs(Am[c][c]));
            kmin = fmin(kmin, fabs(d) / fabs(Am[c][c]));  // pivot over its diagonal: K's cancellation
            dd[c] = d;
            const double inv = rcp_nr(d != 0.0 ? d : 1.0);
#pragma unroll
            for (int r = c + 1; r < N; ++r) {
                double v = Am[r][c];
#pragma unroll
                for (int b = 0; b < c; ++b) v = fma(-Am[r][b], Am[c][b] * dd[b], v);
                Am[r][c] = v * inv;
            }
        }
#pragma unroll
        for (int r = 0; r < KM; ++r) sv[r] = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {  // L z = c
            double v = cv[r];
#pragma unroll
            for (int b = 0; b < r; ++b) v = fma(-Am[r][b], sv[b], v);
            sv[r] = v;
        }
#pragma unroll
        for (int r = 0; r < N; ++r) sv[r] = sv[r] * rcp_nr(dd[r] != 0.0 ? dd[r] : 1.0);
#pragma unroll
        for (int r = N - 1; r >= 0; --r) {  // L' s = D^-1 z
            double v = sv[r];
#pragma unroll
            for (int b = r + 1; b < N; ++b) v = fma(-Am[b][r], sv[b], v);
            sv[r] = v;
        }
        return bad;
    };
    // dispatch on the round's (wave-uniform) size: nsch = 1 is one reciprocal
    auto schur_ksolve = [&](const double (&cv)[LMPC_SCHUR_KMAX], double (&sv)[LMPC_SCHUR_KMAX], double& kmin) -> bool {
        static_assert(LMPC_SCHUR_KMAX == 6, "one instance per size");
        switch (nsch) {
            case 1: return schur_ksolve_n(std::integral_constant<int, 1>{}, cv, sv, kmin);
            case 2: return schur_ksolve_n(std::integral_constant<int, 2>{}, cv, sv, kmin);
            case 3: return schur_ksolve_n(std::integral_constant<int, 3>{}, cv, sv, kmin);
            case 4: return schur_ksolve_n(std::integral_constant<int, 4>{}, cv, sv, kmin);
            case 5: return schur_ksolve_n(std::integral_constant<int, 5>{}, cv, sv, kmin);
            default: return schur_ksolve_n(std::integral_constant<int, 6>{}, cv, sv, kmin);
        }
    };
    // a settled active set failed the certificate right after a range-space round: the same faces once more as a
    // factorised round before the retry ladder (the update's rounding, not the faces, may be what failed)
    bool force_fact = false, refact_done = false;
#ifdef LMPC_SCHUR_DIAG
    int sd_rounds = 0, sd_ent = 0, sd_col = 0, sd_max = 0, sd_run = 0, sd_runmax = 0, sd_mis = 0;
#endif
#endif
    for (;;) {
        if (mode == PRED) {
            if (ipm_it >= prm.dense_iter_cap) break;  // test hook: hand the QP to the Riccati kernel
            double loc = 0.0;
            if (st) ipm_gap(s, z, loc);
            DSTAMP(2);
            sz = wave_sum(loc);
            mu_c = sz * imc;
            DSTAMP(12);  // complementarity mean (wave reduction)
            if (mu_c < tol || ipm_it >= it_end) {
                act = st ? ipm_guess_active(f, s, z, fzmax) : 0;
                mode = POLISH;
                rd = 0;
                keep_tiles = 0;
                have_base = false;
            } else {
                const double rb0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // R is inside H
                double D[6];                                            // D = C'WC, packed
                ipm_barrier<false>(st, s, is, z, mu, fzmax, rb0, D, rt);
                if (st) {
                    ldouble* bk = S.blk + 9 * lane;
                    bk[0] = D[0]; bk[1] = D[1]; bk[2] = D[2];
                    bk[3] = D[1]; bk[4] = D[3]; bk[5] = D[4];
                    bk[6] = D[2]; bk[7] = D[4]; bk[8] = D[5];
                }
            }
            DSTAMP(13);  // Newton-matrix blocks D and weights
        }
        double Tn[9], upn[3];  // this polish round's leg basis (leg_basis of act)
        SchurLeg sl{0, 0, true};  // this leg-step's entries, were the round a range-space one
        if (mode == POLISH) {
            ++prounds;
            apex = false;
            double (&T)[9] = Tn;
#if LMPC_BASIS_TABLE
            if (!bt_built) {  // wave-uniform
                basis_table_build(S.bt, mu, fzmax, lane);
                bt_built = true;
                LMPC_SYNC();
            }
#endif
            if (st) apex = dense_leg_basis(S, act, mu, fzmax, T, upn);
            schur = false;
#if LMPC_POLISH_SCHUR
            if (have_base && !force_fact) {
                // Per changed leg-step: the faces it keeps (cm) span a space of nc free directions holding the
                // factorised basis's nb; the update adds kc = nc - nb of them as new columns (faces dropped) and kr
                // rows (faces added, or at a new apex the nc rows u = 0), each row removing one free direction.
                // Not at an apex with the f_max face (its particular solution is not in the kept space).
                sl = schur_leg(st && act != bact, act, bact, apex);
                const int k = sl.kc + sl.kr;
                nsch = wave_count3(k);
                ncol = wave_count3(sl.kc);
                // against a refactorisation from the first changed tile kt on (cheaper the later kt)
                const unsigned long long dif = __ballot(st && act != bact);
                const int kt = dif ? (__ffsll((long long)dif) - 1) / 5 : 4;
                schur = __all(sl.ok) && nsch > 0 && nsch + ncol <= LMPC_SCHUR_KMAX &&
                        2 * nsch + LMPC_SCHUR_SLOPE2 * kt <= LMPC_SCHUR_LIM2;
            }
            // a factorised round: tiles ahead of the first leg-step whose faces differ from the last factorised
            // round's keep their factors
            if (!schur) {
                const unsigned long long dif = __ballot(have_base && act != bact);
                keep_tiles = have_base && dif ? (__ffsll((long long)dif) - 1) / 5 : 0;
                force_fact = false;
            }
#endif
        }
        if (mode == POLISH && !schur) {
            S.vec2[lane] = 0.0;  // padding / unused variables of the up vector
            LMPC_SYNC();
            bool coupled = false;
            if (st) {
                const double (&T)[9] = Tn;
                const double (&up)[3] = upn;
#pragma unroll
                for (int p = 0; p < 3; ++p) S.lup[3 * lane + p] = up[p];
                ldouble* bk = S.blk + 9 * lane;
#pragma unroll
                for (int e = 0; e < 9; ++e) bk[e] = T[e];
#pragma unroll
                for (int e = 0; e < 9; ++e) coupled |= T[e] != 0.0;
#pragma unroll
                for (int p = 0; p < 3; ++p) S.vec2[vidx(lane, p)] = up[p];
            }
            cmask = (unsigned)__ballot(coupled);
        }
        // ---- right-hand side (and, except in the corrector, the Newton matrix) ----
        if (schur) {
        } else if (mode != POLISH) {
            if (st) {
#pragma unroll
                for (int a = 0; a < 3; ++a) S.vec[vidx(lane, a)] = -(S.gv[vidx(lane, a)] + rt[a]);
            }
            LMPC_SYNC();
        } else {
            LMPC_SYNC();
            // rhs = -T'(H up + g)
            const double hv = h_matvec(S, S.vec2, S.scr, lane) + S.gv[lane];
            LMPC_SYNC();
            S.vec2[lane] = hv;
#if LMPC_POLISH_SCHUR
            S.lhg[lane] = hv;
#endif
            LMPC_SYNC();
            if (st) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    double v = 0.0;
#pragma unroll
                    for (int p = 0; p < 3; ++p) v += S.blk[9 * lane + p * 3 + a] * S.vec2[vidx(lane, p)];
                    S.vec[vidx(lane, a)] = -v;
                }
            }
            LMPC_SYNC();
        }
        if (mode == POLISH) DSTAMP(11);  // polish set-up + right-hand side (matvec)
        else DSTAMP(2);                  // interior point: leg-step work + right-hand side
        if (mode != CORR && !schur) {
            // ---- M tiles ----
            if (mode == PRED) {
#pragma unroll
                for (int t = 0; t < 10; ++t) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) Tl[t][i] = S.Ht[t * DN_TILE + i * 64 + lane];
                }
                // + D on the diagonal leg blocks: one load per tile (lblk_reg below)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int bb = 5 * t + lblk_q;
                    const bool inb = lblk_reg >= 0 && bb < nls;
                    const double d = S.blk[inb ? 9 * bb + lblk_off : 0];
#pragma unroll
                    for (int i = 0; i < 4; ++i) Tl[tix(t, t)][i] += (inb && i == lblk_reg) ? d : 0.0;
                }
            } else {
                // polish: T^ tiles (block diagonal; identity on unused / padding slots)
                d4 Th[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int bb = 5 * t + lblk_q;
                    const bool inb = lblk_reg >= 0 && bb < nls;
                    const double tv = S.blk[inb ? 9 * bb + lblk_off : 0];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        Th[t][i] = (inb && i == lblk_reg) ? tv : (lr + 4 * i == lc ? 1.0 : 0.0);
                }
                // Tl(tr, tc) = T^_tr' H_tr,tc T^_tc  (two X'Y products per tile)
#pragma unroll
                for (int tr = 0; tr < 4; ++tr) {
#pragma unroll
                    for (int tc = tr; tc < 4; ++tc) {
                        if (tc >= NT) continue;
                        d4 Hrc;
#pragma unroll
                        for (int i = 0; i < 4; ++i) Hrc[i] = S.Ht[tix(tr, tc) * DN_TILE + i * 64 + lane];
                        const d4 zero = {0.0, 0.0, 0.0, 0.0};
                        const d4 Yt = tprod(Hrc, Th[tr], zero);  // (T_r' H_rc)'
                        Tl[tix(tr, tc)] = tprod(Yt, Th[tc], zero);
                    }
                }
                // + identity on fixed components (zero T columns) of the diagonal leg blocks: the lane's own diagonal
                // element (register ldg_reg, if it holds one) -- one test per tile
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int bb = 5 * t + lblk_q;
                    const bool dg = ldg_reg >= 0 && bb < nls;
                    const ldouble* bk = S.blk + 9 * (dg ? bb : 0);
                    const int a = lc % 3;
                    // all three loads, then bitwise ands (a short-circuit && waited on each load in turn)
                    const double b0 = bk[a], b1 = bk[3 + a], b2 = bk[6 + a];
                    const bool fixed = dg & (b0 == 0.0) & (b1 == 0.0) & (b2 == 0.0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) Tl[tix(t, t)][i] += (fixed && i == ldg_reg) ? 1.0 : 0.0;
                }
            }
            if (mode == POLISH) DSTAMP(7);  // M tiles (polish)
            else DSTAMP(3);                  // M tiles (interior point)
            // ---- tiled Cholesky M = U'U ----
            // the four tiles' coupled-block masks at once (tile_masks): from nls alone in the interior point, and with
            // the round's coupled leg-steps in the polish -- scalar work, nothing loaded between the tiles
            const unsigned tmasks = tile_masks(nls, mode == POLISH ? cmask : ~0u);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b >= NT) continue;
                DSTAMP(4);
                if (b >= keep_tiles) {
#ifndef LMPC_DIAG_TWO_TILES
                    const DiagInv di = diag_inverse_merged(S.scr, Tl[tix(b, b)], tile_mask(tmasks, b), lane);
#else  // the test-only "diag2tile" build (tests/test_gpu_dense_diag.py): T and W in tiles of their own
                    const DiagInv di = diag_inverse(S.scr, Tl[tix(b, b)], tile_mask(tmasks, b), lane);
#endif
                    Ui[b] = di.ui;
                    UiT[b] = di.uit;
                }
                DSTAMP(6);  // diagonal tiles
#pragma unroll
                for (int c = b + 1; c < 4; ++c) {
                    if (c >= NT) continue;
                    const d4 zero = {0.0, 0.0, 0.0, 0.0};
                    const d4 Mbc = Tl[tix(b, c)];
                    Tl[tix(b, c)] = tprod(Ui[b], Mbc, zero);  // U_bc = U_bb^-T M_bc
                }
#pragma unroll
                for (int c = b + 1; c < 4; ++c) {
#pragma unroll
                    for (int d = c; d < 4; ++d) {
                        if (d >= NT) continue;
                        Tl[tix(c, d)] = tprod_sub(Tl[tix(b, c)], Tl[tix(b, d)], Tl[tix(c, d)]);
                    }
                }
            }
        }
        DSTAMP(4);  // factorisation
        // ---- solve: U'y = r, U x = y (vectors replicated across the accumulator columns), S.vec in place ----
        auto solve_vec = [&]() {
            // forward: y_b = U_bb^-T (r_b - sum_{a<b} U_ab' y_a), all on the VALU (a matrix-core product would use
            // 1 of its 16 columns).  The bracket is column-indexed: lane 16g + c sums U_ab[4i+g][c] y_a[4i+g] over
            // its rows, then over the four row groups -> t[c]; y_b = UiT_b (r_b - t) row by row (the four
            // registers' row sums at once, row_sum4) comes out replicated across the columns, the layout the
            // next bracket reads.
            d4 y[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b >= NT) continue;
                double acc = S.vec[16 * b + lc];
                if (b > 0) {
                    double part = 0.0;
#pragma unroll
                    for (int a = 0; a < b; ++a) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) part = fma(Tl[tix(a, b)][i], y[a][i], part);
                    }
                    acc -= group_sum4(part);
                }
                double pp[4], rs[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) pp[i] = UiT[b][i] * acc;
                row_sum4(pp, rs);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[b][i] = rs[i];
            }
            // backward: t = y_b - sum_c U_bc x_c on the VALU (x_c column-replicated: lane l holds
            // x_c[l&15]; the four registers' row sums at once), then x_b = U_bb^-1 t = UiT_b' t also on the VALU
            // (lane 16g + c sums UiT_b[4i+g][c] t[4i+g], then over the row groups): x_b comes out
            // column-replicated, which is the layout the tiles above read -- no LDS exchange
            double xcol[4];
#pragma unroll
            for (int b = 3; b >= 0; --b) {
                if (b >= NT) continue;
                d4 acc = y[b];
                if (b + 1 < NT) {
                    double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int c = b + 1; c < 4; ++c) {
                        if (c >= NT) continue;
#pragma unroll
                        for (int i = 0; i < 4; ++i) part[i] = fma(Tl[tix(b, c)][i], xcol[c], part[i]);
                    }
                    double rs[4];
                    row_sum4(part, rs);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] -= rs[i];
                }
                double p = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) p = fma(UiT[b][i], acc[i], p);
                xcol[b] = group_sum4(p);
            }
            if (lr == 0) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (b >= NT) continue;
                    S.vec[16 * b + lc] = xcol[b];
                }
            }
            LMPC_SYNC();
        };
        double du[3] = {0.0, 0.0, 0.0};  // range-space rounds: the new columns' part of this leg-step's force
        if (!schur) {
            solve_vec();
#if LMPC_POLISH_SCHUR
            if (mode == POLISH) {  // this factorised round's solution and faces: the base of range-space rounds
#ifdef LMPC_SCHUR_DIAG
                sd_run = 0;
#endif
                S.lua[lane] = S.vec[lane];
                bact = act;
                have_base = true;
            }
#endif
        }
#if LMPC_POLISH_SCHUR
        else {
            // ---- range-space round on the factorised coordinates y (u_b = up_b + T_b y_b) ----
            // Entries e < nsch, in leg-step order, a leg-step's columns before its rows:
            //   column: a new free direction t (unit, in u-space) with coefficient w: v_e = T'H e_t (base
            //           coordinates), c_e = -t'(H up + g)_b;
            //   row:    r'u_b = beta on the base coordinates: v_e = T_b'r (on leg-step b only), c_e = beta - r'up_b.
            // With W_e = M^-1 v_e and s = [w; lambda] the round's KKT system reduces to K s = c - V'y0,
            // K = Cb - V'W (Cb: t't'H blocks between columns, r't between a row and a column of the same leg-step):
            // quasi-definite (columns +, rows -), so LDL' needs no pivoting; y = y0 - W s, u_b += sum of t w.
            constexpr int KM = LMPC_SCHUR_KMAX;
            ldouble* U = S.scr + 48;       // KM x [x0 x1 x2 c]: t (column) or T_b'r (row), and c_e
            ldouble* uleg = U + 4 * KM;    // leg-step of each entry
            ldouble* utyp = uleg + KM;     // 0: row, 1 + j: column j
            ldouble* Cb = utyp + KM;       // KM x KM
            ldouble* Wc = S.scr + 128;     // M^-1 v_e by variable, 64 doubles each
            ldouble* Vc = Wc + 64 * nsch;  // the columns' v_e by variable (nsch + ncol <= KM)
            const unsigned long long below = (1ull << lane) - 1ull;
            const int e0 = wave_prefix3(sl.kc + sl.kr, below), c0 = wave_prefix3(sl.kc, below);
            if (lane < KM * KM) Cb[lane] = 0.0;
            LMPC_SYNC();
#ifdef LMPC_SCHUR_DIAG
            {
                ++sd_rounds;
                sd_ent += nsch;
                sd_col += ncol;
                sd_max = max(sd_max, nsch);
                sd_runmax = max(sd_runmax, ++sd_run);
                // leg_free against the bases themselves: the factorised one (LDS), this round's, the kept faces'
                bool mis = false;
                if (st && act != bact) {
                    double Tk[9], uk[3];
                    (void)dense_leg_basis(S, act & bact, mu, fzmax, Tk, uk);
                    mis = ncols3(S.blk + 9 * lane) != leg_free(bact) || ncols3(Tn) != leg_free(act) ||
                          ncols3(Tk) != leg_free(act & bact);
                }
                sd_mis += __popcll(__ballot(mis));
            }
#endif
            if (sl.kc + sl.kr) {
                const ldouble* Tb = S.blk + 9 * lane;
                const ldouble* ub = S.lup + 3 * lane;
                double Tc[9], uc[3];
                (void)dense_leg_basis(S, act & bact, mu, fzmax, Tc, uc);
                // new directions: T_c's columns beyond span(T_b) (orthonormal)
                double tv[3][3];
                const int nb = ncols3(Tb);
                if (nb == 0) {
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int p = 0; p < 3; ++p) tv[j][p] = Tc[3 * p + j];
                } else {
                    double best = -1.0, rb[3] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        double r[3] = {Tc[q], Tc[3 + q], Tc[6 + q]};
#pragma unroll
                        for (int m = 0; m < 2; ++m) {  // T_b's columns (nb <= 2 where columns are added)
                            const double pr = Tb[m] * r[0] + Tb[3 + m] * r[1] + Tb[6 + m] * r[2];
#pragma unroll
                            for (int p = 0; p < 3; ++p) r[p] = fma(-pr, Tb[3 * p + m], r[p]);
                        }
                        const double n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
                        if (n2 > best) {
                            best = n2;
                            rb[0] = r[0]; rb[1] = r[1]; rb[2] = r[2];
                        }
                    }
                    const double in = rsq_nr(best > 0.0 ? best : 1.0);
#pragma unroll
                    for (int p = 0; p < 3; ++p) tv[0][p] = rb[p] * in;
                    // second (nb = 1, nc = 3): orthogonal to T_b's column and the first
                    const double b0 = Tb[0], b1 = Tb[3], b2 = Tb[6];
                    tv[1][0] = b1 * tv[0][2] - b2 * tv[0][1];
                    tv[1][1] = b2 * tv[0][0] - b0 * tv[0][2];
                    tv[1][2] = b0 * tv[0][1] - b1 * tv[0][0];
                    tv[2][0] = tv[2][1] = tv[2][2] = 0.0;
                }
                // rows: added faces, or at a new apex T_c's columns (u_b = 0)
                double rv[3][3], rbv[3];
                if (apex) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
#pragma unroll
                        for (int p = 0; p < 3; ++p) rv[j][p] = Tc[3 * p + j];
                        rbv[j] = 0.0;
                    }
                } else {
                    const ActiveRows ar = active_rows(act & ~bact);
                    cons_rowvec(ar.i0, mu, rv[0]);
                    cons_rowvec(ar.i1, mu, rv[1]);
                    cons_rowvec(ar.i2, mu, rv[2]);
                    rbv[0] = ar.i0 == 4 ? fzmax : 0.0;
                    rbv[1] = ar.i1 == 4 ? fzmax : 0.0;
                    rbv[2] = ar.i2 == 4 ? fzmax : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j >= sl.kc) continue;
                    const int e = e0 + j;
                    double c = 0.0;
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        U[4 * e + p] = tv[j][p];
                        c = fma(-tv[j][p], S.lhg[vidx(lane, p)], c);
                    }
                    U[4 * e + 3] = c;
                    uleg[e] = (double)lane;
                    utyp[e] = (double)(1 + c0 + j);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (i >= sl.kr) continue;
                    const int e = e0 + sl.kc + i;
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        U[4 * e + q] = fma(rv[i][0], Tb[q], fma(rv[i][1], Tb[3 + q], rv[i][2] * Tb[6 + q]));
                    U[4 * e + 3] = rbv[i] - fma(rv[i][0], ub[0], fma(rv[i][1], ub[1], rv[i][2] * ub[2]));
                    uleg[e] = (double)lane;
                    utyp[e] = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (j >= sl.kc) continue;
                        const double a = rv[i][0] * tv[j][0] + rv[i][1] * tv[j][1] + rv[i][2] * tv[j][2];
                        Cb[KM * e + e0 + j] = a;
                        Cb[KM * (e0 + j) + e] = a;
                    }
                }
            }
            LMPC_SYNC();
            // columns: v = T'H e_t (H e_t from three columns of H, h_col3), and the t't'H block of Cb
            if (ncol) {
                const int w16 = lane & 15, bl = 5 * (lane >> 4) + w16 / 3, al = w16 % 3;
                const bool vl = w16 < 15 && bl < nls;
                for (int e = 0; e < nsch; ++e) {  // wave-uniform
                    const double ty = utyp[e];
                    if (ty < 0.5) continue;
                    const double t3[3] = {U[4 * e], U[4 * e + 1], U[4 * e + 2]};
                    S.vec2[lane] = h_col3(S, (int)uleg[e], t3, lane);  // H e_t: three columns of H
                    LMPC_SYNC();
                    double v = 0.0;
                    if (vl) {
#pragma unroll
                        for (int p = 0; p < 3; ++p) v = fma(S.blk[9 * bl + 3 * p + al], S.vec2[vidx(bl, p)], v);
                    }
                    Vc[64 * ((int)ty - 1) + lane] = v;
                    if (lane < nsch && utyp[lane] > 0.5) {
                        const int bj = (int)uleg[lane];
                        double c = 0.0;
#pragma unroll
                        for (int p = 0; p < 3; ++p) c = fma(U[4 * lane + p], S.vec2[vidx(bj, p)], c);
                        Cb[KM * lane + e] = c;
                    }
                    LMPC_SYNC();
                }
            }
            // W_e = M^-1 v_e
            for (int e = 0; e < nsch; ++e) {  // wave-uniform
                const double ty = utyp[e];
                if (ty > 0.5) {
                    S.vec[lane] = Vc[64 * ((int)ty - 1) + lane];
                } else {
                    S.vec[lane] = 0.0;
                    LMPC_SYNC();
                    if (lane < 3) S.vec[vidx((int)uleg[e], lane)] = U[4 * e + lane];
                }
                LMPC_SYNC();
                solve_vec();
                Wc[64 * e + lane] = S.vec[lane];
            }
            LMPC_SYNC();
            // column-column products and the columns' right-hand sides (wave sums over the variables)
            if (ncol) {
                const double y0l = S.lua[lane];
                for (int e = 0; e < nsch; ++e) {  // wave-uniform
                    const double ty = utyp[e];
                    if (ty < 0.5) continue;
                    const double vl = Vc[64 * ((int)ty - 1) + lane];
                    const double cy = wave_sum(vl * y0l);
                    if (lane == 0) U[4 * e + 3] -= cy;
                    for (int f = e; f < nsch; ++f) {
                        if (utyp[f] < 0.5) continue;
                        const double g = wave_sum(vl * Wc[64 * f + lane]);
                        if (lane == 0) {
                            Cb[KM * e + f] -= g;
                            if (f != e) Cb[KM * f + e] -= g;
                        }
                    }
                }
                LMPC_SYNC();
            }
            // K's right-hand side c - V'y0 on every lane (entries beyond nsch: 0; the columns' V'y0 is in U already)
            double cv[KM], sv[KM];
#pragma unroll
            for (int i = 0; i < KM; ++i) {
                const bool iv = i < nsch;
                const bool rwi = iv && utyp[iv ? i : 0] < 0.5;
                const int rbi = iv ? (int)uleg[i] : 0;
                double c = iv ? U[4 * i + 3] : 0.0;
                if (rwi) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) c = fma(-U[4 * i + q], S.lua[vidx(rbi, q)], c);
                }
                cv[i] = c;
            }
            double kmin = 1.0;
            const bool bad = schur_ksolve(cv, sv, kmin);
            double yv = S.lua[lane];
#pragma unroll
            for (int j = 0; j < KM; ++j)
                if (j < nsch) yv = fma(-Wc[64 * j + lane], sv[j], yv);
            if (ncol && !bad && st) {
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    if (j >= nsch || utyp[j] < 0.5 || (int)uleg[j] != lane) continue;
#pragma unroll
                    for (int p = 0; p < 3; ++p) du[p] = fma(U[4 * j + p], sv[j], du[p]);
                }
            }
            if (lane == 0) {  // s of this round, for the refinement of a verified round (polish verification below)
#pragma unroll
                for (int j = 0; j < KM; ++j) S.scr[DN_SCHUR_SV + j] = sv[j];
                S.scr[DN_SCHUR_SV + KM] = kmin;
            }
            // a rank-deficient update (rounding): keep y0; the round will not verify and the next one refactorises
            // the same faces (a settled set that fails right after a range-space round, below)
            S.vec[lane] = bad ? S.lua[lane] : yv;
            if (bad) have_base = false;
            LMPC_SYNC();
            DSTAMP(14);  // range-space round
        }
#endif
        DSTAMP(5);  // solve
        // ---- leg-step solution ----
        u[0] = u[1] = u[2] = 0.0;
        if (st) {
            double y3[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) y3[a] = S.vec[vidx(lane, a)];
            if (mode == POLISH) {
                const ldouble* Tb = S.blk + 9 * lane;
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    u[p] = apex ? 0.0
                                : S.lup[3 * lane + p] + Tb[p * 3] * y3[0] + Tb[p * 3 + 1] * y3[1] + Tb[p * 3 + 2] * y3[2] +
                                      du[p];
            } else {
#pragma unroll
                for (int p = 0; p < 3; ++p) u[p] = y3[p];
            }
        }
        if (mode == PRED) {
            double amax = 1.0;
            double dsa[5], dza[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) dsa[i] = dza[i] = 0.0;
            if (st) {
#pragma unroll
                for (int m = 0; m < 3; ++m) S.lua[3 * lane + m] = u[m];
            }
            if (st) ipm_pred_leg(u, s, is, z, mu, fzmax, dsa, dza, amax);
            const double aa = wave_min(amax);
            double loc = 0.0;
            if (st) ipm_aff_gap(s, z, dsa, dza, aa, loc);
            // ratio = mu_aff / mu over the sums, not the means as in the Riccati kernels: the 1/mc factors cancel
            smu = ipm_centring(wave_sum(loc) / sz, mu_c);
            if (st) ipm_corr_rhs(s, is, z, dsa, dza, smu, mu, fzmax, rt);
            mode = CORR;
            DSTAMP(8);  // predictor step length + corrector terms
        } else if (mode == CORR) {
            double ds[5], dz[5];
            double amax = 1.0, dmax = 1.0;  // primal (s) and dual (z) distances to the boundary
#pragma unroll
            for (int i = 0; i < 5; ++i) ds[i] = dz[i] = 0.0;
            if (st) {
                double ua[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) ua[m] = S.lua[3 * lane + m];
                ipm_corr_leg(u, ua, s, is, z, smu, mu, fzmax, ds, dz, amax, dmax);
            }
            const double alpha = ipm_step_length(wave_min(amax));
            const double alpd = ipm_step_length(wave_min(dmax));
            if (st) {
#pragma unroll
                for (int m = 0; m < 3; ++m) f[m] += alpha * (u[m] - f[m]);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    s[i] += alpha * ds[i];
                    z[i] += alpd * dz[i];
                    is[i] = rcp_nr(s[i]);
                }
            }
            ++ipm_it;
            mode = PRED;
            DSTAMP(9);  // corrector step + iterate update
        } else {
            // ---- polish verification: gradient H u + g, primal feasibility, multiplier signs ----
            S.vec2[lane] = 0.0;
            LMPC_SYNC();
            if (st) {
#pragma unroll
                for (int p = 0; p < 3; ++p) S.vec2[vidx(lane, p)] = u[p];
            }
            LMPC_SYNC();
            const double gl = h_matvec(S, S.vec2, S.scr, lane) + S.gv[lane];
            LMPC_SYNC();
            S.vec2[lane] = gl;
            LMPC_SYNC();
            double g[3] = {0.0, 0.0, 0.0};
            double gloc = 1.0;
            if (st) {
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    g[p] = S.vec2[vidx(lane, p)];
                    gloc = fmax(gloc, fabs(g[p]));
                }
            }
            const double gscale = wave_max(gloc);
            int changed = 0;
            double sres = 0.0;  // stationarity residual on the leg-step's free directions (leg_certify)
            if (st) {
                const LegCert c = leg_certify(u, g, act, apex, mu, fzmax, prm.tol_p * fzmax, prm.tol_d * gscale);
                act = c.act;
                changed = c.changed ? 1 : 0;
                sres = c.res;
            }
            DSTAMP(10);  // polish verification
            const unsigned long long chg = __ballot(changed);
            if (!chg) {
                // a settled active set is the optimum's only if H u + g vanishes on every free direction; otherwise
                // this attempt cannot verify (another round would repeat it) and the retry ladder takes over
                const double sr = wave_max(sres);
#ifdef LMPC_KKT_DIAG
                if (lane == 0 && qp < LMPC_KKT_DIAG_QPS) {
                    lmpc_kkt_diag_dense[qp][0] = sr / gscale;
                    lmpc_kkt_diag_dense[qp][1] = 0.0;
                    lmpc_kkt_diag_dense[qp][2] = gscale;
                    lmpc_kkt_diag_dense[qp][3] = 1.0;
                }
#endif
#ifndef LMPC_KKT_OFF
                if (sr <= prm.tol_d * gscale)
#endif
                {
#if LMPC_POLISH_SCHUR
                    if (schur && sr > LMPC_REFINE_SR * gscale) {
                        // One step of iterative refinement of a verified range-space round.  The
                        // update solves the round's bordered system [M V; V' Cb] [y; s] = [r0; c] through K = Cb - V'W,
                        // W = M^-1 V; K's rounding, amplified by W, left config 2's forces up to ~2e-9 N from the optimum
                        // (~1e-10 N refactorised).  The residuals come from the gradient G = H u + g in hand (S.vec2):
                        //   base coordinates  rho_y = -T_b'G - (rows' a) lambda
                        //   a column entry    rho_e = -t'G - (r't) lambda;   a row entry  rho_e = c_e - a'y - (r't) w
                        // and the same factorisations give the correction: dy0 = M^-1 rho_y, K ds = rho_s - V'dy0,
                        // dy = dy0 - W ds, du_b = T_b dy_b + t dw.  The refined forces are certified again (feasibility
                        // of the free faces, stationarity / the apex cone test); if they fail, the verified ones stand.
                        constexpr int KM = LMPC_SCHUR_KMAX;
                        const ldouble* U = S.scr + 48;
                        const ldouble* uleg = U + 4 * KM;
                        const ldouble* utyp = uleg + KM;
                        const ldouble* Cb = utyp + KM;
                        const ldouble* Wc = S.scr + 128;
                        const ldouble* Vc = Wc + 64 * nsch;
                        const ldouble* svs = S.scr + DN_SCHUR_SV;
                        double re = 0.0;  // entry residual (lane e)
                        if (lane < nsch) {
                            const int b = (int)uleg[lane];
                            const bool row = utyp[lane] < 0.5;
                            if (row) {
                                re = U[4 * lane + 3];
#pragma unroll
                                for (int q = 0; q < 3; ++q) re = fma(-U[4 * lane + q], S.vec[vidx(b, q)], re);
                            } else {
#pragma unroll
                                for (int p = 0; p < 3; ++p) re = fma(-U[4 * lane + p], S.vec2[vidx(b, p)], re);
                            }
#pragma unroll
                            for (int f = 0; f < KM; ++f)
                                if (f < nsch && (utyp[f] < 0.5) != row) re = fma(-Cb[KM * lane + f], svs[f], re);
                        }
                        // rho_y, lane = variable (16 t + 3 a + q <-> leg-step 5 t + a, component q)
                        const int vw = lane & 15, vb = 5 * (lane >> 4) + vw / 3, vq = vw % 3;
                        double ry = 0.0;
                        if (vw < 15 && vb < nls) {
                            const ldouble* Tb = S.blk + 9 * vb;
#pragma unroll
                            for (int p = 0; p < 3; ++p) ry = fma(-Tb[3 * p + vq], S.vec2[vidx(vb, p)], ry);
#pragma unroll
                            for (int e = 0; e < KM; ++e)
                                if (e < nsch && utyp[e] < 0.5 && (int)uleg[e] == vb) ry = fma(-U[4 * e + vq], svs[e], ry);
                        }
                        LMPC_SYNC();  // the reads of y above come first
                        S.vec[lane] = ry;
                        LMPC_SYNC();
                        solve_vec();  // dy0 = M^-1 rho_y (the base factorisation, untouched by range-space rounds)
                        const double dyl = S.vec[lane];
                        double rc = re;
                        if (lane < nsch && utyp[lane] < 0.5) {
                            const int b = (int)uleg[lane];
#pragma unroll
                            for (int q = 0; q < 3; ++q) rc = fma(-U[4 * lane + q], S.vec[vidx(b, q)], rc);
                        }
                        double cv[KM], dsv[KM];
#pragma unroll
                        for (int e = 0; e < KM; ++e) {
                            cv[e] = 0.0;
                            if (e < nsch) {  // wave-uniform
                                double c = readlane_f64(rc, e);
                                const double ty = utyp[e];
                                if (ty > 0.5) c -= wave_sum(Vc[64 * ((int)ty - 1) + lane] * dyl);
                                cv[e] = c;
                            }
                        }
                        double kmin2 = 1.0;
                        const bool bad2 = schur_ksolve(cv, dsv, kmin2);
                        double dy = dyl;
#pragma unroll
                        for (int j = 0; j < KM; ++j)
                            if (j < nsch) dy = fma(-Wc[64 * j + lane], dsv[j], dy);
                        LMPC_SYNC();
                        S.vec[lane] = dy;
                        LMPC_SYNC();
                        double ur[3] = {u[0], u[1], u[2]};
                        if (st && !apex) {
                            const ldouble* Tb = S.blk + 9 * lane;
                            double d3[3];
#pragma unroll
                            for (int a = 0; a < 3; ++a) d3[a] = S.vec[vidx(lane, a)];
#pragma unroll
                            for (int p = 0; p < 3; ++p) ur[p] += Tb[3 * p] * d3[0] + Tb[3 * p + 1] * d3[1] + Tb[3 * p + 2] * d3[2];
#pragma unroll
                            for (int j = 0; j < KM; ++j) {
                                if (j >= nsch || utyp[j] < 0.5 || (int)uleg[j] != lane) continue;
#pragma unroll
                                for (int p = 0; p < 3; ++p) ur[p] = fma(U[4 * j + p], dsv[j], ur[p]);
                            }
                        }
                        // certify the refined forces
                        S.vec2[lane] = 0.0;
                        LMPC_SYNC();
                        if (st) {
#pragma unroll
                            for (int p = 0; p < 3; ++p) S.vec2[vidx(lane, p)] = ur[p];
                        }
                        LMPC_SYNC();
                        const double gr = h_matvec(S, S.vec2, S.scr, lane) + S.gv[lane];
                        LMPC_SYNC();
                        S.vec2[lane] = gr;
                        LMPC_SYNC();
                        double g2[3] = {0.0, 0.0, 0.0}, gl2 = 1.0;
                        if (st) {
#pragma unroll
                            for (int p = 0; p < 3; ++p) {
                                g2[p] = S.vec2[vidx(lane, p)];
                                gl2 = fmax(gl2, fabs(g2[p]));
                            }
                        }
                        const double gs2 = wave_max(gl2);
                        bool ok = !bad2;
                        if (st) {  // the certificate asks nothing of the leg-step, and its residual is within tol_d
                            const LegCert c = leg_certify(ur, g2, act, apex, mu, fzmax, prm.tol_p * fzmax, prm.tol_d * gs2);
                            ok = ok && !c.changed && c.res <= prm.tol_d * gs2;
                        }
#ifdef LMPC_REFINE_DIAG
                        {
                            double dl = 0.0;
#pragma unroll
                            for (int p = 0; p < 3; ++p) dl = fmax(dl, fabs(ur[p] - u[p]));
                            dl = wave_max(dl);
                            const bool allok = __all(ok);
                            if (lane == 0 && qp < LMPC_KKT_DIAG_QPS) {
                                lmpc_refine_diag[qp][0] = sr / gscale;
                                lmpc_refine_diag[qp][1] = S.scr[DN_SCHUR_SV + KM];
                                lmpc_refine_diag[qp][2] = dl;
                                lmpc_refine_diag[qp][3] = allok ? 1.0 : 2.0;
                            }
                        }
#endif
                        if (__all(ok)) {
#pragma unroll
                            for (int p = 0; p < 3; ++p) u[p] = ur[p];
                        }
                    }
#endif
                    done = true;
                    break;
                }
#if LMPC_POLISH_SCHUR
                if (schur && !refact_done) {
                    force_fact = true;  //  the same faces once more, factorised, before the retry ladder
                    refact_done = true;
                } else
#endif
                    rd = prm.max_rounds - 1;
            }
            keep_tiles = chg ? (__ffsll((long long)chg) - 1) / 5 : 0;  // tile of the first changed leg-step
            if (++rd >= prm.max_rounds) {
                keep_tiles = 0;
                schur = false;  // the interior point resumes: its own right-hand sides and factorisations
                if (!ipm_retry(prm, att, tol, it_end)) break;
                mode = PRED;
            }
        }
    }
#if LMPC_POLISH_SCHUR && defined(LMPC_SCHUR_DIAG)
    if (lane == 0 && qp < LMPC_SCHUR_DIAG_QPS) {
        const int sd[6] = {sd_rounds, sd_ent, sd_col, sd_max, sd_runmax, sd_mis};
#pragma unroll
        for (int i = 0; i < 6; ++i) lmpc_schur_diag[qp][i] = (double)sd[i];
    }
#endif
    if (!done) {
        qstatus = LMPC_QP_MAX_ITER;
#pragma unroll
        for (int m = 0; m < 3; ++m) u[m] = f[m];
    }
    const int bad = st && (u[0] != u[0] || u[1] != u[1] || u[2] != u[2]);
    const bool anybad = __any(bad);
    // A QP without a verified optimum (iteration caps, non-finite iterate) is left to the Riccati kernel of the
    // same launch, as lmpc_gi_kernel does: flag 0, nothing written.  Flag 1: solved here.
    if (done_out) {
        const bool keep = done && !anybad;
        if (lane == 0) done_out[qp] = keep ? 1 : 0;
        if (!keep) {
            DSTAMP_FLUSH(qp);
            return false;
        }
    }
    // ---- output: stance forces through LDS to the lane of leg-step 4k + j ----
    LMPC_SYNC();
    if (st) {
        double fo[3];
        world_force<TERRAIN>(S.tf + 9 * lj, u, fo);
#pragma unroll
        for (int p = 0; p < 3; ++p) S.vec[3 * lane + p] = fo[p];
    }
    LMPC_SYNC();
    double* gout = grf + (size_t)qp * 12 * H;
    if (lane < 4 * H) {
#pragma unroll
        for (int p = 0; p < 3; ++p) gout[3 * lane + p] = (anybad || !stl) ? 0.0 : S.vec[3 * (stl ? rank : 0) + p];
    }
    qp_store_words(status, iters, qp, lane, anybad, qstatus, ipm_it, prounds);
    DSTAMP(2);
    DSTAMP_FLUSH(qp);
    return true;
}

}  // namespace lmpc
