"""The dense path's condensation: the recursions of csrc/lmpc_dense_common.h's header comment against the closed
forms dense_condense evaluates (CPU, numpy).

Recursions (state x = [Theta p omega v], A_m = I + N_m, N_m = dt blkdiag(Rz(psi_m), I) from the velocities to the
positions, B rows 6-11 = G0):
    free response  c_{m+1} = A_m c_m - g dt e11, c_0 = x0;  e_m = Q (c_{m+1} - xref_m)
    adjoint        mu_m = e_{m-1} + A_m' mu_{m+1};  g_v = (B e_v)' mu_{k+1} for a variable of step k
    cost-to-go     P~_H = Q, P~_m = Q + A_m' P~_{m+1} A_m
    Hessian        column v: L = P~_{k+1} B e_v, then L <- A_{i+1}' L down the steps i < k;
                   H[v'][v] = (B e_v')' L for the stance variables v' of step i, + R on the diagonal blocks.
Closed forms: N_j N_k = 0, so A_{n-1} ... A_m = I + N_m + ... + N_{n-1}, and c, mu and P~[:, 6:12] are prefix /
suffix sums over the steps of terms in cos / sin psi_j.

Tolerance: 1e-12 of the largest |entry| of the compared array -- fewer than a hundred roundings of 1.1e-16 on terms
no larger than the result's scale stay under 2e-14; the bar leaves 50x.
"""
import numpy as np
import pytest

TOL = 1e-12
DT, GRAV, MASS = 0.03, 9.81, 12.5
Q = np.array([25.0, 20.0, 10.0, 2.0, 3.0, 50.0, 0.1, 0.2, 0.3, 0.25, 0.35, 0.15])
R = np.array([1e-5, 2e-5, 3e-5] * 4)


def rz(psi):
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def a_mat(psi):
    A = np.eye(12)
    A[0:3, 6:9] = DT * rz(psi)
    A[3:6, 9:12] = DT * np.eye(3)
    return A


def rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def make_g0(rng, tilted):
    """B rows 6-11: dt Iw^-1 [r_j]x over dt/m I per leg; on tilted terrain times blkdiag(R_j)."""
    iw = np.linalg.inv(np.diag([0.07, 0.26, 0.28]) + 0.01 * np.ones((3, 3)))
    g0 = np.zeros((6, 12))
    for j in range(4):
        f = rng.uniform(-0.3, 0.3, 3)
        sk = np.array([[0, -f[2], f[1]], [f[2], 0, -f[0]], [-f[1], f[0], 0]])
        blk = np.vstack([DT * iw @ sk, DT / MASS * np.eye(3)])
        g0[:, 3 * j:3 * j + 3] = blk @ rot(rng) if tilted else blk
    return g0


def contacts(H, pattern):
    c = np.zeros((H, 4), dtype=bool)
    if pattern == "trot":
        for k in range(H):
            c[k, [0, 3] if (k // 2) % 2 == 0 else [1, 2]] = True
    elif pattern == "all5":  # four legs down for five steps
        c[:min(H, 5)] = True
    elif pattern == "gap":  # a flight phase in the middle
        c[:] = True
        c[H // 3:max(H // 3 + 1, 2 * H // 3)] = False
        c[:, 1] = False
        if not c.any():
            c[0, 0] = True
    elif pattern == "last":  # one stance leg-step, at the last step
        c[H - 1, 2] = True
    return c


def problem(H, pattern, tilted, seed):
    rng = np.random.default_rng(seed)
    psi = np.cumsum(rng.uniform(-1.5, 1.5, H)) + rng.uniform(-2 * np.pi, 2 * np.pi)
    x0 = rng.standard_normal(12)
    xref = rng.standard_normal((H, 12))
    xref[:, 2] = psi
    return psi, x0, xref, make_g0(rng, tilted), contacts(H, pattern)


def variables(con):
    """stance variables in leg-step order: (step, leg, component)"""
    return [(k, j, a) for k in range(con.shape[0]) for j in range(4) if con[k, j] for a in range(3)]


# ---- the recursions ----
def recursion(psi, x0, xref, g0, con):
    H = len(psi)
    A = [a_mat(p) for p in psi]
    x = x0.copy()
    em = np.zeros((H, 12))
    for m in range(H):
        x = A[m] @ x
        x[11] -= GRAV * DT  # after p_z has used v_z
        em[m] = Q * (x - xref[m])
    mus = np.zeros((H + 2, 12))  # mu_m, m = 1..H
    for m in range(H, 0, -1):
        mus[m] = em[m - 1] + (A[m].T @ mus[m + 1] if m < H else 0.0)
    P = np.zeros((H + 1, 12, 12))
    P[H] = np.diag(Q)
    for m in range(H - 1, 0, -1):
        P[m] = np.diag(Q) + A[m].T @ P[m + 1] @ A[m]
    var = variables(con)
    N = len(var)
    g = np.zeros(N)
    Hm = np.zeros((N, N))
    row = {v: n for n, v in enumerate(var)}
    for n, (k, j, a) in enumerate(var):
        b = g0[:, 3 * j + a]
        g[n] = b @ mus[k + 1][6:12]
        L = P[k + 1][:, 6:12] @ b
        for i in range(k, -1, -1):
            if i < k:
                L = A[i + 1].T @ L
            for jp in range(4):
                if con[i, jp]:
                    for ap in range(3):
                        val = g0[:, 3 * jp + ap] @ L[6:12]
                        if (i, jp) == (k, j):
                            val += (np.diag(R[3 * j:3 * j + 3]))[ap, a]
                        Hm[row[(i, jp, ap)], n] = val
                        if i < k:
                            Hm[n, row[(i, jp, ap)]] = val
    return em, mus[1:H + 1, 6:12], g, P[1:, :, 6:12], Hm


# ---- the closed forms, as dense_condense evaluates them (lane l = step l) ----
def suffix(v):
    return np.cumsum(v[::-1], axis=0)[::-1]


def shl1(v):
    out = np.zeros_like(v)
    out[:-1] = v[1:]
    return out


def closed(psi, x0, xref, g0, con):
    H = len(psi)
    ck, sk = np.cos(psi), np.sin(psi)
    C, Sn = np.cumsum(ck), np.cumsum(sk)
    n = np.arange(1, H + 1, dtype=float)
    gd = GRAV * DT
    c = np.tile(x0, (H, 1))
    c[:, 0] = x0[0] + DT * (C * x0[6] + Sn * x0[7])
    c[:, 1] = x0[1] + DT * (C * x0[7] - Sn * x0[6])
    c[:, 2] = x0[2] + DT * (n * x0[8])
    for a in range(3):
        c[:, 3 + a] = x0[3 + a] + DT * (n * x0[9 + a])
    c[:, 5] = x0[5] + DT * (n * x0[11] - gd * (0.5 * n * (n - 1.0)))
    c[:, 11] = x0[11] - n * gd
    e = Q * (c - xref)
    # adjoint: row l = mu_{l+1}
    E = suffix(e[:, 0:6])
    t = np.zeros((H, 6))
    t[:, 0] = DT * (ck * E[:, 0] - sk * E[:, 1])
    t[:, 1] = DT * (sk * E[:, 0] + ck * E[:, 1])
    t[:, 2:6] = DT * E[:, 2:6]
    mu = suffix(e[:, 6:12] + shl1(t))
    # cost-to-go sums: row l = P~_l's (row H: zero)
    rho = H - np.arange(H, dtype=float)
    q0, q1 = Q[0], Q[1]
    uc, us = suffix(rho * ck), suffix(rho * sk)
    un, vn = shl1(uc), shl1(us)
    hc, hs = rho * ck + 2 * un, rho * sk + 2 * vn
    da = q0 * (ck * hc) + q1 * (sk * hs)
    dd = q0 * (sk * hs) + q1 * (ck * hc)
    db = (q0 - q1) * (ck * (rho * sk + vn) + sk * un)
    z = np.zeros(1)
    uc, us = np.append(uc, z), np.append(us, z)
    sa, sb, sd = (np.append(suffix(d), z) for d in (da, db, dd))
    # P~_m[:, 6:12] for m = 1..H
    Pc = np.zeros((H, 12, 6))
    for m in range(1, H + 1):
        r = H - m
        cnt, w1, w2 = r + 1.0, r * (r + 1) / 2.0, r * (r + 1) * (2 * r + 1) / 6.0
        Pm = Pc[m - 1]
        Pm[0, 0:2] = DT * q0 * np.array([uc[m], us[m]])
        Pm[1, 0:2] = DT * q1 * np.array([-us[m], uc[m]])
        Pm[6, 0:2] = [cnt * Q[6] + DT * DT * sa[m], DT * DT * sb[m]]
        Pm[7, 0:2] = [DT * DT * sb[m], cnt * Q[7] + DT * DT * sd[m]]
        Pm[2, 2] = DT * Q[2] * w1
        Pm[8, 2] = cnt * Q[8] + DT * DT * Q[2] * w2
        for a in range(3):
            Pm[3 + a, 3 + a] = DT * Q[3 + a] * w1
            Pm[9 + a, 3 + a] = cnt * Q[9 + a] + DT * DT * Q[3 + a] * w2
    # gradient and Hessian columns: L from the sums, then down the steps as in the kernel
    var = variables(con)
    N = len(var)
    row = {v: i for i, v in enumerate(var)}
    g = np.zeros(N)
    Hm = np.zeros((N, N))
    for nv, (k, j, a) in enumerate(var):
        gc = g0[:, 3 * j + a]
        g[nv] = gc @ mu[k]
        m = k + 1
        r = H - 1 - k
        cnt, w1, w2 = r + 1.0, r * (r + 1) / 2.0, r * (r + 1) * (2 * r + 1) / 6.0
        L = np.zeros(12)
        L[0] = DT * q0 * (uc[m] * gc[0] + us[m] * gc[1])
        L[1] = DT * q1 * (uc[m] * gc[1] - us[m] * gc[0])
        L[6] = cnt * Q[6] * gc[0] + DT * DT * (sa[m] * gc[0] + sb[m] * gc[1])
        L[7] = cnt * Q[7] * gc[1] + DT * DT * (sb[m] * gc[0] + sd[m] * gc[1])
        L[2] = DT * Q[2] * w1 * gc[2]
        L[8] = (cnt * Q[8] + DT * DT * Q[2] * w2) * gc[2]
        for b in range(3):
            L[3 + b] = DT * Q[3 + b] * w1 * gc[3 + b]
            L[9 + b] = (cnt * Q[9 + b] + DT * DT * Q[3 + b] * w2) * gc[3 + b]
        for i in range(k, -1, -1):
            if i < k:
                cq, sq = ck[i + 1], sk[i + 1]
                l0, l1, l2 = L[0], L[1], L[2]
                L[6] += DT * (cq * l0 - sq * l1)
                L[7] += DT * (sq * l0 + cq * l1)
                L[8] += DT * l2
                L[9:12] += DT * L[3:6]
            for jp in range(4):
                if con[i, jp]:
                    for ap in range(3):
                        val = g0[:, 3 * jp + ap] @ L[6:12]
                        Hm[row[(i, jp, ap)], nv] = val
                        if i < k:
                            Hm[nv, row[(i, jp, ap)]] = val
        for ap in range(3):  # + R on the own block, after the column
            Hm[row[(k, j, ap)], nv] += np.diag(R[3 * j:3 * j + 3])[ap, a]
    return e, mu, g, Pc, Hm


def close(a, b):
    scale = max(np.abs(b).max(), np.finfo(float).tiny)
    return np.abs(a - b).max() <= TOL * scale


@pytest.mark.parametrize("tilted", [False, True], ids=["flat", "tilted"])
@pytest.mark.parametrize("pattern", ["trot", "all5", "gap", "last"])
@pytest.mark.parametrize("H", [1, 2, 3, 10, 16])
def test_closed_forms_equal_recursions(H, pattern, tilted):
    for seed in range(3):
        psi, x0, xref, g0, con = problem(H, pattern, tilted, 1000 * H + seed)
        assert con.any()
        ref = recursion(psi, x0, xref, g0, con)
        got = closed(psi, x0, xref, g0, con)
        for name, a, b in zip(("em", "mu", "g", "P~[:, 6:12]", "H"), got, ref):
            assert close(a, b), f"{name}: H={H} {pattern} seed {seed}: {np.abs(a - b).max():.3e} of {np.abs(b).max():.3e}"


def test_yaw_sequences_wrap():
    """the random yaw sequences of the cases above do leave (-pi, pi]"""
    assert any(np.abs(problem(H, "trot", False, 1000 * H + s)[0]).max() > np.pi for H in (3, 10, 16) for s in range(3))


def test_hessian_symmetric_and_positive():
    psi, x0, xref, g0, con = problem(10, "trot", True, 7)
    Hm = closed(psi, x0, xref, g0, con)[4]
    assert np.abs(Hm - Hm.T).max() <= TOL * np.abs(Hm).max()
    assert np.linalg.eigvalsh(0.5 * (Hm + Hm.T)).min() > 0.0
