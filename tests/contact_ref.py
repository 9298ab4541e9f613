"""Independent NumPy reference for the frictional contact model of include/lmpc/lmpc_contact.h (test helper, not a
test).

K = J M^-1 J' and u_free = J v_free come from rbd_ref.terms by np.linalg.solve on the dense 18 x 18 M: no elimination
is shared with the product.  The pyramid QP  min 1/2 P' K P + P' c  is
written over the pyramids' edges (P_l = E a_l, a_l >= 0), which with K = L L' makes it a non-negative least-squares
problem, and solved by the textbook dense active-set method for that: Lawson & Hanson's NNLS (dense least squares on
the passive columns by np.linalg.lstsq).  It shares nothing with the product's Gauss-Seidel sweeps, mode bases or
block Cholesky.  The answer is classified into the header's ten modes from its slacks alone, its own KKT conditions
are checked (`solve_qp` raises if they do not hold), and the strict-complementarity margin is reported: the smallest
inactive slack, active multiplier or apex dual slack, relative to max(1, |P|inf, |c|inf), so that a test can refuse
cases that sit on a tie.
"""
from __future__ import annotations

import numpy as np

import rbd_ref as R
from sim_ref import state_from_qv

FACES = ((-1.0, 0.0), (1.0, 0.0), (0.0, -1.0), (0.0, 1.0))  # normals (nx, ny, mu) of  P_x <= mu P_z, -P_x <= ..., y
# active faces (+x, -x, +y, -y) -> mode
MODE_OF = {(0, 0, 0, 0): 0, (1, 0, 0, 0): 1, (0, 1, 0, 0): 2, (0, 0, 1, 0): 3, (0, 0, 0, 1): 4, (1, 0, 1, 0): 5,
           (1, 0, 0, 1): 6, (0, 1, 1, 0): 7, (0, 1, 0, 1): 8, (1, 1, 1, 1): 9}
KKT_TOL = 1e-10
ACTIVE_TOL = 1e-9


def face_rows(mu):
    return np.array([[nx, ny, mu] for nx, ny in FACES])


def problem(model, state, tau, dt, ground_z=0.0, use_gap=True, recover_speed=0.0, t=None):
    """The step's contact problem -> dict(K, c, u_free, v_free, gap, terms)."""
    t = t if t is not None else R.terms(model, state)
    M, J = t["M"], t["J"]
    top = M @ t["v"] + dt * (np.concatenate([np.zeros(6), np.asarray(tau, dtype=np.float64)]) - t["nle"])
    v_free = np.linalg.solve(M, top)
    K = J @ np.linalg.solve(M, J.T)
    K = 0.5 * (K + K.T)
    u_free = J @ v_free
    gap = t["foot_pos"][2::3] - ground_z
    b = np.zeros(12)
    if use_gap:
        b[2::3] = np.maximum(gap, -recover_speed * dt) / dt
    return dict(K=K, c=u_free + b, u_free=u_free, v_free=v_free, gap=gap, terms=t)


def _nnls(A, b):
    """min |A x - b|, x >= 0: Lawson & Hanson's active-set algorithm NNLS (Solving Least Squares Problems, ch. 23).  A
    column that depends on the passive ones has a zero gradient and is never taken in, so the passive columns stay
    independent although the four edges of one foot's pyramid are dependent."""
    m = A.shape[1]
    x, passive = np.zeros(m), np.zeros(m, dtype=bool)
    tol = 1e-11 * max(1.0, float(np.max(np.abs(A.T @ b))))
    for _ in range(10 * m + 50):
        grad = A.T @ (b - A @ x)
        cand = np.flatnonzero(~passive & (grad > tol))
        if cand.size == 0:
            return x
        passive[cand[np.argmax(grad[cand])]] = True
        for _ in range(10 * m + 50):
            s = np.zeros(m)
            s[passive] = np.linalg.lstsq(A[:, passive], b, rcond=None)[0]
            if s[passive].min() > 0.0:
                x = s
                break
            neg = passive & (s <= 0.0)
            alpha = float(np.min(x[neg] / (x[neg] - s[neg])))
            x = x + alpha * (s - x)
            passive &= x > 1e-14 * max(1.0, float(np.max(np.abs(x))))
            x[~passive] = 0.0
        else:
            raise RuntimeError("contact_ref: NNLS's inner loop did not terminate")
    raise RuntimeError("contact_ref: NNLS did not terminate")


def _pyramid_qp(K, c, mu):
    """min 1/2 x' K x + c' x over the product of pyramids: x_l = E a_l with the pyramid's four edges E and a_l >= 0,
    K = L L', so the objective is 1/2 |L' E a + L^-1 c|^2 up to a constant: a non-negative least-squares problem."""
    n = K.shape[0]
    E1 = np.array([[sx * mu, sy * mu, 1.0] for sx in (1, -1) for sy in (1, -1)]).T  # 3 x 4
    E = np.kron(np.eye(n // 3), E1)
    L = np.linalg.cholesky(K)
    return E @ _nnls(L.T @ E, -np.linalg.solve(L, c))


def classify(P, w, mask, mu, scale):
    """Modes from the slacks alone, the multipliers by least squares on the active normals -> (modes, margin, worst
    KKT violation), all relative to `scale`."""
    N = face_rows(mu)
    modes, margin, viol = [], np.inf, 0.0
    for l in range(4):
        if not mask[l]:
            modes.append(10)
            continue
        p, wl = P[3 * l:3 * l + 3], w[3 * l:3 * l + 3]
        slack = N @ p / scale
        act = tuple(int(s <= ACTIVE_TOL) for s in slack)
        if act not in MODE_OF:
            raise RuntimeError(f"contact_ref: foot {l} has active faces {act}")
        mode = MODE_OF[act]
        modes.append(mode)
        viol = max(viol, float(-slack.min()))
        if mode == 9:
            dual = (wl[2] - mu * (abs(wl[0]) + abs(wl[1]))) / scale
            margin, viol = min(margin, dual), max(viol, -dual)
            continue
        rows = [i for i in range(4) if act[i]]
        margin = min([margin] + [slack[i] for i in range(4) if not act[i]])
        if rows:
            lam, *_ = np.linalg.lstsq(N[rows].T, wl, rcond=None)
            fit = float(np.max(np.abs(N[rows].T @ lam - wl))) / scale
            margin, viol = min(margin, float(lam.min()) / scale), max(viol, fit, float(-lam.min()) / scale)
        else:
            viol = max(viol, float(np.max(np.abs(wl))) / scale)
    return np.array(modes, dtype=np.int32), float(margin), float(viol)


def solve_qp(K, c, mask, mu):
    """The bare problem -> dict(P, w, modes, margin).  Raises if its own KKT conditions do not hold to KKT_TOL."""
    K, c = np.asarray(K, dtype=np.float64), np.asarray(c, dtype=np.float64)
    feet = [l for l in range(4) if mask[l]]
    P = np.zeros(12)
    if feet:
        idx = [3 * l + i for l in feet for i in range(3)]
        P[idx] = _pyramid_qp(K[np.ix_(idx, idx)], c[idx], mu)
    w = K @ P + c
    for l in range(4):
        if not mask[l]:
            w[3 * l:3 * l + 3] = 0.0
    cm = np.concatenate([c[3 * l:3 * l + 3] for l in feet]) if feet else np.zeros(1)
    scale = max(1.0, float(np.max(np.abs(P))), float(np.max(np.abs(cm))))
    modes, margin, viol = classify(P, w, mask, mu, scale)
    comp = abs(float(P @ w)) / scale ** 2
    if viol > KKT_TOL or comp > KKT_TOL:
        raise RuntimeError(f"contact_ref: KKT violation {viol:.2e}, complementarity {comp:.2e}")
    return dict(P=P, w=w, modes=modes, margin=margin, scale=scale)


def step(model, state, tau, mask, dt, ground_z=0.0, mu=0.6, use_gap=True, recover_speed=0.0, touch_rule=0,
         force_threshold=50.0, t=None):
    """One plant step of the contact model -> dict(P, w, modes, margin, gap, v, q, qdd, force, next, foot_pos,
    foot_vel, held, touch, K, c, terms)."""
    pr = problem(model, state, tau, dt, ground_z, use_gap, recover_speed, t)
    t = pr["terms"]
    s = solve_qp(pr["K"], pr["c"], mask, mu)
    P = s["P"]
    vp = pr["v_free"] + np.linalg.solve(t["M"], t["J"].T @ P)
    qp = t["q"] + dt * vp
    foot_vel = t["J"] @ vp
    foot_pos = t["foot_pos"] + dt * foot_vel
    force = P / dt
    if touch_rule == 0:
        touch = (foot_pos[2::3] <= ground_z).astype(np.int32)
    else:
        touch = (np.linalg.norm(force.reshape(4, 3), axis=1) > force_threshold).astype(np.int32)
    return dict(P=P, w=s["w"], modes=s["modes"], margin=s["margin"], gap=pr["gap"], v=vp, q=qp, qdd=(vp - t["v"]) / dt,
                force=force, next=state_from_qv(qp, vp), foot_pos=foot_pos, foot_vel=foot_vel,
                held=(P[2::3] > 0.0).astype(np.int32), touch=touch, K=pr["K"], c=pr["c"], v_free=pr["v_free"], terms=t)
