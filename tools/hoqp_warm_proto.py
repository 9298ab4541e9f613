#!/usr/bin/env python3
"""Dev tool (CPU): numpy prototype of the warm-started hierarchical chain (lmpc_hoqp.hip, warm instantiation;
DESIGN.md 4c "Warm start"), on tools/hoqp_proto.py's functions.

Per level, with the active set the chain's previous solve left (frozen rows active, own rows violated): frozen rows
whose projection this tick dropped leave the set, the exact crossover starts from y = 0 on the true bounds, and a
verified answer ends the level; anything else is the cold level of hoqp_proto (interior point, then the crossover from
its iterate).  Either way the set the crossover verified is carried on; a level that kept its iterate carries none.

    python tools/hoqp_warm_proto.py                 the feasibility table (second solve, next tick, contact change)
    python tools/hoqp_warm_proto.py --golden-wbc    second solve of the 16 committed WBC golden chains, level by level
    python tools/hoqp_warm_proto.py --write         regenerate tests/golden/hoqp_warm_golden.npz (oracle/hoqp.py answers)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
# hoqp_proto reads its switches from the environment, XO_ROUNDS at import: the kernel's settings
os.environ.setdefault("EXACT", "1")
os.environ.setdefault("VEXACT", "1")
os.environ.setdefault("HFLOOR", "1e-10")
os.environ.setdefault("XO_ROUNDS", "12")
os.environ.setdefault("RTOL", "1e-7")
import hoqp_proto as P  # noqa: E402
from oracle import hoqp as Q  # noqa: E402

from legged_mpc_control_amd import wbc as W  # noqa: E402

XO_ROUNDS = 12
FIXTURE = os.path.join(ROOT, "tests", "golden", "hoqp_warm_golden.npz")
WBC_DIMS = np.array([42, 3, 30, 18, 12, 0, 44, 0, 0, 0], dtype=np.int32)  # n, levels, eq rows[4], ineq rows[4]


def nnls(A, b, tol):
    """Lawson-Hanson: lam >= 0 minimising |A lam - b| (the kernel's nnls_rows: multipliers of dependent active rows).
    Returns (lam, residual within tol)."""
    m = A.shape[1]
    lam = np.zeros(m)
    pas = np.zeros(m, bool)
    eps = 1e-13 * (1.0 + float(np.max(np.abs(A.T @ b))) if m else 0.0)
    for _ in range(3 * m + 3):
        w = A.T @ (b - A @ lam)
        w[pas] = -np.inf
        if not (m and np.max(w) > eps):
            break
        pas[int(np.argmax(w))] = True
        for _ in range(m + 1):
            if not pas.any():
                break
            Ap = A[:, pas]
            sp = P.chol_solve(P.chol_floor(Ap.T @ Ap), Ap.T @ b)
            sa = np.zeros(m)
            sa[pas] = sp
            if np.all(sa[pas] > 0.0):
                lam = sa
                break
            neg = pas & ~(sa > 0.0) & (lam - sa > 0.0)
            alpha = min(1.0, float(np.min(lam[neg] / (lam[neg] - sa[neg])))) if neg.any() else 1.0
            lam = np.where(pas, lam + alpha * (sa - lam), 0.0)
            pas &= lam > 0.0
            lam[~pas] = 0.0
    return lam, bool(np.max(np.abs(A @ lam - b)) <= tol) and bool(np.all(lam >= 0.0))


def xo_core(Hy, c, Pm, h, Dz, g, y_start, fa, ob, scale, rounds=XO_ROUNDS):
    """hoqp_proto.crossover with the kernel's rho = max(1, max diag Hy), started from given flags (fa: frozen rows
    active, ob: own rows violated) and a given point.  Returns (verified, y, fa, ob, repair rounds)."""
    p, s = Pm.shape[0], Dz.shape[0]
    fa, ob = fa.copy(), ob.copy()
    tol = 1e-9 * scale
    rho = max(1.0, float(np.max(np.diag(Hy))))
    for rd in range(rounds):
        RA = Pm[fa] if p else np.zeros((0, len(c)))
        na = RA.shape[0]
        if na > 64:
            return False, y_start, fa, ob, rd
        K = Hy + (Dz[ob].T @ Dz[ob] if s else 0) + rho * RA.T @ RA
        L = P.chol_floor(K)
        rhs = -c + (Dz[ob].T @ g[ob] if s else 0) + rho * RA.T @ (h[fa] if p else np.zeros(0))
        y0 = y_start + P.chol_solve(L, rhs - K @ y_start)
        y, lam = y0, np.zeros(0)
        if na:
            T = np.stack([P.chol_solve(L, RA[a]) for a in range(na)])
            Ls = P.chol_floor(RA @ T.T)
            lam = P.chol_solve(Ls, RA @ y0 - h[fa])
            y = y0 - T.T @ lam
            # dependent active rows (a floored pivot) with a negative multiplier, the point on every active row:
            # non-negative multipliers for the same point, if some exist
            if np.max(np.diag(Ls)) > 1e30 and np.min(lam) < -tol and np.max(np.abs(RA @ y - h[fa])) <= tol:
                t_own = np.where(ob, Dz @ y - g, 0.0) if s else np.zeros(0)
                ln, ok = nnls(RA.T, -(Hy @ y + c + (Dz.T @ t_own if s else 0)), tol)
                if ok:
                    lam = ln
        if not (np.all(np.isfinite(y)) and np.all(np.isfinite(lam))):
            return False, y_start, fa, ob, rd
        changed = False
        tp = Pm @ y - h if p else np.zeros(0)
        t = Dz @ y - g if s else np.zeros(0)
        fa_now = fa.copy()
        if na and np.any(lam < -tol):
            fa[np.nonzero(fa_now)[0][np.argmin(lam)]] = False
            changed = True
        bad = (~fa_now) & (tp > tol) if p else np.zeros(0, bool)
        if np.any(bad):
            fa[np.argmax(np.where(bad, tp, -np.inf))] = True
            changed = True
        flip = (ob & (t < -tol)) | ((~ob) & (t > tol)) if s else np.zeros(0, bool)
        if np.any(flip):
            ob = ob ^ flip
            changed = True
        if changed:
            continue
        if p and np.any(np.abs(tp[fa]) > tol):  # dependent active rows whose bounds disagree
            return False, y_start, fa, ob, rd
        lf = np.zeros(p)
        if na:
            lf[fa] = lam
        st = Hy @ y + c + (Pm.T @ lf if p else 0) + (Dz.T @ np.where(ob, t, 0.0) if s else 0)
        if not np.max(np.abs(st)) <= tol:
            return False, y_start, fa, ob, rd
        return True, y, fa, ob, rd
    return False, y_start, fa, ob, rounds


LAST = {}


def _crossover_recording(Hy, c, Pm, h, Dz, g, y_ipm, s1, z1, s2, z2, scale, rounds=XO_ROUNDS):
    """Stands in for hoqp_proto.crossover inside level_ipm: the same call, and the verified flags are kept."""
    p, s = Pm.shape[0], Dz.shape[0]
    fa = (z2 > s2) if p else np.zeros(0, bool)
    ob = (z1 > s1) if s else np.zeros(0, bool)
    ok, y, fa, ob, rd = xo_core(Hy, c, Pm, h, Dz, g, y_ipm, fa, ob, scale, rounds)
    LAST.update(ok=ok, fa=fa, ob=ob)
    return y if ok else y_ipm


P.crossover = _crossover_recording


def warm_chain(tasks, act=None, warm_rounds=XO_ROUNDS):
    """hoqp_proto.hoqp_device with the warm attempt.  act: per level None (no set) or (fa, ob).  Returns xs, ws, the
    new act, and per level (tried, taken, repair rounds)."""
    n = max(tasks[0].a.shape[1], tasks[0].d.shape[1])
    Z = np.eye(n)
    x = np.zeros(n)
    stk_d, stk_f, stk_w = np.zeros((0, n)), np.zeros(0), np.zeros(0)
    xs, ws, act_out, outcome = [], [], [], []
    for l, t in enumerate(tasks):
        nd = Z.shape[1]
        d = t.d if t.d.shape[1] else np.zeros((0, n))
        if t.a.shape[0]:
            G = t.a @ Z
            Hy = G.T @ G + 1e-12 * np.eye(nd)
            c = G.T @ (t.a @ x - t.b)
        else:
            Hy, c = 1e-12 * np.eye(nd), np.zeros(nd)
        Pm = stk_d @ Z
        h = stk_f - stk_d @ x + stk_w
        dead = np.zeros(Pm.shape[0], bool)
        if Pm.shape[0]:
            dead = np.max(np.abs(Pm), axis=1) <= 1e-12 * np.max(np.abs(stk_d), axis=1) * np.max(np.abs(Z))
            Pm, h = Pm.copy(), h.copy()
            Pm[dead] = 0.0
            h[dead] = 1.0
        Dz = d @ Z
        g = t.f - d @ x if d.shape[0] else np.zeros(0)
        scale = 1.0 + max(np.max(np.abs(c)) if nd else 0.0, np.max(np.abs(h)) if h.size else 0.0,
                          np.max(np.abs(g)) if g.size else 0.0)
        tried = taken = False
        rd = 0
        if act is not None and act[l] is not None and Pm.shape[0] + Dz.shape[0] > 0:
            fa, ob = act[l]
            tried = True
            taken, y, fa, ob, rd = xo_core(Hy, c, Pm, h, Dz, g, np.zeros(nd), fa & ~dead, ob, scale, warm_rounds)
            if taken:
                act_out.append((fa, ob))
        if not taken:
            LAST.clear()
            y, _, _ = P.level_ipm(Hy, c, Pm, h, Dz, g)
            act_out.append((LAST["fa"], LAST["ob"]) if LAST.get("ok") else None)
        v = np.maximum(0.0, Dz @ y - g) if d.shape[0] else np.zeros(0)
        x = x + Z @ y
        xs.append(x.copy())
        ws.append(v.copy())
        outcome.append((tried, taken, rd))
        stk_d = np.vstack([d, stk_d])
        stk_f = np.concatenate([t.f if d.shape[0] else np.zeros(0), stk_f])
        stk_w = np.concatenate([stk_w, v])
        if t.a.shape[0]:
            Z = Z @ Q.fullpivlu_kernel(t.a @ Z)
    return xs, ws, act_out, outcome


def to_oracle(tasks):
    return [Q.Task(t.a, t.b, t.d, t.f) for t in tasks]


def next_tick(s, rng, rel=0.01, new_contact=None):
    """The synthetic dynamics terms one low-level tick later: what a 1.25 ms older state changes, perturbed by `rel`
    relative (element-wise, so structural zeros stay); new_contact replaces the contact pattern."""
    out = dict(s)
    for k in ("nle", "dJv", "J", "base_accel", "swing_acc", "forces_des"):
        a = np.asarray(s[k], dtype=np.float64)
        out[k] = a * (1.0 + rel * rng.standard_normal(a.shape))
    if new_contact is not None:
        out["contact"] = new_contact
    return out


def tasks_of(s):
    return W.wbc_tasks(s["M"], s["nle"], s["J"], s["dJv"], s["contact"], s["base_accel"], s["swing_acc"], s["forces_des"])


def oracle_chain(tasks):
    lv = []
    for t in to_oracle(tasks):
        lv.append(Q.HoQp(t, lv[-1] if lv else None))
    return np.stack([h.solution() for h in lv]), lv[-1].stacked_slack


def rel_x(xa, xb):
    return float(np.max(np.abs(xa[-1] - xb[-1])) / (1.0 + np.max(np.abs(xb[-1]))))


def pair(seed, rel=0.01, change=False):
    sa = W.synth_wbc(seed)
    rng = np.random.default_rng(777_000 + seed)
    nc = None
    if change:
        nc = W.GAITS[(W.GAITS.index(tuple(sa["contact"])) + 1) % len(W.GAITS)]
    return sa, next_tick(sa, rng, rel, nc)


def table():
    def run(label, seeds, make):
        taken = total = 0
        worst_x = worst_w = 0.0
        worst_rd = 0
        for seed in seeds:
            ta, tb = make(seed)
            _, _, act, _ = warm_chain(to_oracle(ta))
            xw, ww, _, out = warm_chain(to_oracle(tb), act)
            xc, wc, _, _ = warm_chain(to_oracle(tb))
            taken += sum(o[1] for o in out)
            total += len(out)
            worst_rd = max([worst_rd] + [o[2] for o in out if o[1]])
            worst_x = max(worst_x, rel_x(xw, xc))
            worst_w = max(worst_w, float(np.max(np.abs(np.concatenate(ww) - np.concatenate(wc)))))
        print(f"{label}: {taken} of {total} levels warm, most repair rounds {worst_rd}, worst final x warm vs cold "
              f"{worst_x:.1e}, worst slack difference {worst_w:.1e}")

    run("second solve, 6 seeds", range(6), lambda s: (W.synth_wbc_tasks(s),) * 2)
    run("next tick 1 %, 8 seeds", range(8), lambda s: tuple(tasks_of(q) for q in pair(s)))
    run("1 % + contact change on odd seeds, 8 seeds", range(8),
        lambda s: tuple(tasks_of(q) for q in pair(s, change=bool(s & 1))))
    run("next tick 10 %, 6 seeds", range(6), lambda s: tuple(tasks_of(q) for q in pair(s, rel=0.1)))


def unpack(rec, dims):
    n, out, o = int(dims[0]), [], 0
    for l in range(int(dims[1])):
        m, s = int(dims[2 + l]), int(dims[6 + l])
        a = rec[o:o + m * n].reshape(m, n); o += m * n
        b = rec[o:o + m]; o += m
        d = rec[o:o + s * n].reshape(s, n); o += s * n
        f = rec[o:o + s]; o += s
        out.append(Q.Task(a, b, d, f))
    return out


def golden_wbc():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hoqp_golden.npz"), allow_pickle=False)
    rec, dims = g["wbc_rec"], g["wbc_dims"]
    bad = []
    for b in range(rec.shape[0]):
        tasks = unpack(rec[b], dims)
        _, _, act, _ = warm_chain(tasks)
        xw, _, _, out = warm_chain(tasks, act)
        print(f"chain {b}: first solve verified {[a is not None for a in act]}, second solve (tried, taken, rounds) {out}, "
              f"final x vs golden {rel_x(xw, g['wbc_x'][b]):.1e}")
        bad += [(b, l) for l, o in enumerate(out) if act[l] is not None and not o[1]]
    print("levels with a verified set not taken warm:", bad)


def write():
    from legged_mpc_control_amd import hoqp as HQ

    dims = HQ.dims_of(W.synth_wbc_tasks(0))
    recs_a, recs_b, xa, wa, xb, wb, outc, seeds, changed = [], [], [], [], [], [], [], [], []

    def add(seed, change):
        sa, sb = pair(seed, change=change)
        ta, tb = tasks_of(sa), tasks_of(sb)
        _, _, act, _ = warm_chain(to_oracle(ta))
        _, _, _, out = warm_chain(to_oracle(tb), act)
        if not change and not all(o[1] and o[2] <= 2 for o in out):
            return False
        oa, ob = oracle_chain(ta), oracle_chain(tb)
        recs_a.append(HQ.pack(ta, dims)); recs_b.append(HQ.pack(tb, dims))
        xa.append(oa[0]); wa.append(oa[1]); xb.append(ob[0]); wb.append(ob[1])
        outc.append([[int(o[0]), int(o[1]), o[2]] for o in out])
        seeds.append(seed); changed.append(int(change))
        return True

    seed = 0
    while len(seeds) < 8:
        add(seed, False)
        seed += 1
    for k in range(4):
        add(100 + k, True)
    np.savez_compressed(FIXTURE, dims=WBC_DIMS, rec_a=np.stack(recs_a), rec_b=np.stack(recs_b), x_a=np.stack(xa),
                        w_a=np.stack(wa), x_b=np.stack(xb), w_b=np.stack(wb),
                        proto=np.array(outc, dtype=np.int32),  # [pair][level] (tried, taken, repair rounds) on tick B
                        seeds=np.array(seeds, dtype=np.int32), contact_changed=np.array(changed, dtype=np.int32))
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, seeds {seeds}, changed {changed}")
    print("proto (tried, taken, rounds) per pair and level:", outc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden-wbc", action="store_true")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if args.golden_wbc:
        golden_wbc()
    elif args.write:
        write()
    else:
        table()


if __name__ == "__main__":
    main()
