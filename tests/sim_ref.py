"""Independent NumPy reference for the rigid-body plant of include/lmpc/lmpc_sim.h (test helper, not a test).

It assembles the dense KKT matrix [[M, -J_C'], [J_C, 0]] from rbd_ref.terms and solves it with np.linalg.solve (LU with
partial pivoting): it shares no elimination with the product (per-leg Cholesky + a reduced 6 x 6 base block).  It
applies the same unilateral rule and returns every pass's normal components, in newtons, so that a test can refuse
cases that sit on a tie (a normal component near zero decides the contact set).
"""
from __future__ import annotations

import numpy as np

import rbd_ref as R


def _rows(held):
    return [3 * l + i for l in range(4) if held[l] for i in range(3)]


def _kkt(t, held, rhs_top, rhs_con):
    rows = _rows(held)
    Jc = t["J"][rows]
    n = len(rows)
    K = np.block([[t["M"], -Jc.T], [Jc, np.zeros((n, n))]])
    x = np.linalg.solve(K, np.concatenate([rhs_top, rhs_con[rows]]))
    lam = np.zeros(12)
    lam[rows] = x[18:]
    return x[:18], lam


def _rule(t, contact, unilateral, solve, scale):
    """The header's rule.  solve(held) -> (x, multipliers); scale: multipliers -> newtons."""
    held = [bool(c) for c in contact]
    normals = []
    while True:
        x, lam = solve(held)
        normals.append([scale * lam[3 * l + 2] for l in range(4) if held[l]])
        release = [l for l in range(4) if held[l] and lam[3 * l + 2] < 0.0] if unilateral else []
        if not release:
            return x, lam, held, normals
        for l in release:
            held[l] = False


def forward_dynamics(model, state, tau, contact, unilateral=True, t=None):
    """M qdd - J_C' F = S' tau - h, J_C qdd = -(dJ v)_C -> dict(qdd, force, held, normals, terms)."""
    t = t if t is not None else R.terms(model, state)
    top = np.concatenate([np.zeros(6), np.asarray(tau, dtype=np.float64)]) - t["nle"]
    qdd, F, held, normals = _rule(t, contact, unilateral, lambda h: _kkt(t, h, top, -t["dJv"]), 1.0)
    return dict(qdd=qdd, force=F, held=np.array(held, dtype=np.int32), normals=normals, terms=t)


def state_from_qv(q, v):
    """(q, v) -> measured_rbd_state (36): omega = E(euler) rates."""
    return np.concatenate([q[3:6], q[0:3], q[6:18], R.euler_map(q[3:6]) @ v[3:6], v[0:3], v[6:18]])


def step(model, state, tau, contact, dt, ground_z=0.0, unilateral=True, t=None):
    """M v+ - J_C' P = M v + dt (S' tau - h), J_C v+ = 0, q+ = q + dt v+ -> dict(v, q, P, qdd, force, next, foot_pos,
    foot_vel, touch, held, normals, terms)."""
    t = t if t is not None else R.terms(model, state)
    q, v = t["q"], t["v"]
    top = t["M"] @ v + dt * (np.concatenate([np.zeros(6), np.asarray(tau, dtype=np.float64)]) - t["nle"])
    vp, P, held, normals = _rule(t, contact, unilateral, lambda h: _kkt(t, h, top, np.zeros(12)), 1.0 / dt)
    qp = q + dt * vp
    foot_vel = t["J"] @ vp
    foot_pos = t["foot_pos"] + dt * foot_vel
    return dict(v=vp, q=qp, P=P, qdd=(vp - v) / dt, force=P / dt, next=state_from_qv(qp, vp), foot_pos=foot_pos,
                foot_vel=foot_vel, touch=(foot_pos[2::3] <= ground_z).astype(np.int32),
                held=np.array(held, dtype=np.int32), normals=normals, terms=t)


def tie(normals, weight, rel=1e-6):
    """True if some pass has a normal component with |.| < rel * weight (weight = m g)."""
    return any(abs(n) < rel * weight for p in normals for n in p)
