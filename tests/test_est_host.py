"""CPU tests of the state estimator (include/lmpc/lmpc_est.h): the host functions against the independent NumPy
restatement of BasicKF in tests/est_ref.py (dense matrices, np.linalg.solve), the drift rule's ticks, symmetry and
definiteness of P, init, the sensor model's identities on host plant steps, convergence, the noise keys, status 1,
argument checks, and the shared header under the host compiler's sanitizers.

Streams.  Per robot (Go1, A1) and dt (1.25 ms, 2.5 ms) 400 ticks of smooth sensors: a standing pose plus sinusoids on
every joint (velocities their exact derivatives), small smooth Euler angles, gyro and accelerometer signals; the contact
pattern changes every 25 ticks and runs through all 16 patterns (all-swing and all-stance included); on every seventh
tick the flags are fractional (0.7 for a stance foot, 0.3 for a swing foot).

Tolerance.  MEASURED is the host's largest deviation from est_ref over exactly these streams, x and P of every tick,
relative to max(1, |ref|); the assertions allow ten times that.  The product applies 28 scalar updates where the
restatement solves with the 28 x 28 S (cond(S) printed by the test; up to about 1e5): cond x 28 x eps = 6e-10 is what a
different elimination order may cost, and a deviation above 1e-9 is a defect, not a tolerance (DEFECT).
"""
import ctypes
import subprocess

import numpy as np
import pytest

import est_ref as ER
import rbd_ref as R
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import est, rbd, sim
from test_rbd_host import model_json, preset

# measured on these streams (python -m pytest tests/test_est_host.py -s prints the figures of the run)
MEASURED = {"x": 3.4e-15, "P": 2.2e-14}
TOL = {k: 10.0 * v for k, v in MEASURED.items()}
DEFECT = 1e-9
ROBOTS = ("go1", "a1")
DTS = (0.00125, 0.0025)
TICKS = 400
STAND = np.array([0.0, 0.8, -1.6] * 4)
PATTERNS = [tuple(float((p >> l) & 1) for l in range(4)) for p in range(16)]


def make_stream(seed, ticks, dt, first_pattern=0):
    """`ticks` sensor dicts (see the module docstring)."""
    rng = np.random.default_rng(seed)
    amp, freq, ph = rng.uniform(0.05, 0.3, 12), rng.uniform(0.5, 3.0, 12), rng.uniform(0, 2 * np.pi, 12)
    ea, ef, ep = rng.uniform(0.02, 0.15, 3), rng.uniform(0.3, 2.0, 3), rng.uniform(0, 2 * np.pi, 3)
    wa, wf, wp = rng.uniform(0.05, 0.5, 3), rng.uniform(0.5, 4.0, 3), rng.uniform(0, 2 * np.pi, 3)
    aa, af, ap = rng.uniform(0.1, 1.0, 3), rng.uniform(0.5, 5.0, 3), rng.uniform(0, 2 * np.pi, 3)
    out = []
    for k in range(ticks):
        t = k * dt
        euler = ea * np.sin(2 * np.pi * ef * t + ep)
        c = np.array(PATTERNS[(first_pattern + k // 25) % 16])
        if k % 7 == 3:
            c = np.where(c > 0.5, 0.7, 0.3)
        out.append(dict(
            imu_acc=ER.rot(euler).T @ np.array([0.0, 0.0, 9.81]) + aa * np.sin(2 * np.pi * af * t + ap),
            imu_ang_vel=wa * np.sin(2 * np.pi * wf * t + wp), euler=euler,
            joint_pos=STAND + amp * np.sin(2 * np.pi * freq * t + ph),
            joint_vel=amp * 2 * np.pi * freq * np.cos(2 * np.pi * freq * t + ph), contact=c))
    return out


def to_struct(s) -> N.LmpcEstSensors:
    return est.sensors(**s)


def dev(a, ref):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(ref)) / np.maximum(1.0, np.abs(np.asarray(ref)))))


@pytest.fixture(scope="module")
def runs():
    """Per (robot, dt): the stream, the restatement's x, P, det and cond(S) of every tick (computed once, shared, never
    modified)."""
    out = {}
    for r, name in enumerate(ROBOTS):
        md = model_json(name)
        for d, dt in enumerate(DTS):
            stream = make_stream(900 + 10 * r + d, TICKS, dt, first_pattern=5 * r + 3 * d)
            x, P = ER.init(md, stream[0])
            xs, Ps, dets, conds = [], [], [], []
            for s in stream:
                x, P, det, cond = ER.update(md, s, x, P, dt)
                xs.append(x), Ps.append(P), dets.append(det), conds.append(cond)
            out[(name, dt)] = dict(md=md, model=preset(name), stream=stream, x=xs, P=Ps, det=np.array(dets),
                                   cond=np.array(conds))
    return out


def host_run(c, dt):
    cfg = est.cfg(dt=dt)
    f = est.init(c["model"], cfg, to_struct(c["stream"][0]))
    views = []
    for s in c["stream"]:
        _, o = est.update(c["model"], cfg, to_struct(s), f)
        assert o.status == 0
        v = est.filter_view(f)
        views.append((v["x"].copy(), v["P"].copy()))
    return views


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("dt", DTS)
def test_parity_with_restatement(runs, name, dt):
    c = runs[(name, dt)]
    seen = {tuple(s["contact"]) for s in c["stream"]}
    assert all(p in seen for p in PATTERNS) and any(0.3 in k for k in seen)
    worst = {"x": 0.0, "P": 0.0}
    for (x, P), xr, Pr in zip(host_run(c, dt), c["x"], c["P"]):
        worst["x"], worst["P"] = max(worst["x"], dev(x, xr)), max(worst["P"], dev(P, Pr))
    print(f"{name} dt {dt}: host vs est_ref over {TICKS} ticks:", {k: f"{v:.2e}" for k, v in worst.items()},
          f"cond(S) <= {c['cond'].max():.2e}")
    for k in worst:
        assert worst[k] <= DEFECT, f"{k}: {worst[k]:.2e} is a defect"
        assert worst[k] <= TOL[k], f"{k}: {worst[k]:.2e}"


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("dt", DTS)
def test_drift_rule_fires_on_the_same_ticks(runs, name, dt):
    """The restatement's determinant is at least 1e-6 (relative) from the threshold on EVERY tick of the streams, so
    the rule's decision is unambiguous; the host then takes it on exactly the same ticks, seen in P bit for bit: rows
    and columns 0, 1 are exactly zero outside their block on those ticks and on no other."""
    c = runs[(name, dt)]
    margin = np.abs(c["det"] - 1e-6) / 1e-6
    assert margin.min() > 1e-6, f"tick {margin.argmin()}: relative margin {margin.min():.1e}"
    fired_ref = c["det"] > 1e-6
    assert fired_ref.sum() >= 3 and (~fired_ref).sum() >= 100
    fired = []
    for (x, P) in host_run(c, dt):
        fired.append(bool(np.all(P[0:2, 2:] == 0.0) and np.all(P[2:, 0:2] == 0.0)))
    print(f"{name} dt {dt}: drift rule fired on {int(fired_ref.sum())} ticks, least relative margin {margin.min():.1e}")
    assert np.array_equal(np.array(fired), fired_ref)


@pytest.mark.parametrize("name", ROBOTS)
def test_P_symmetric_positive_definite(runs, name):
    c = runs[(name, DTS[0])]
    for k, (x, P) in enumerate(host_run(c, DTS[0])):
        assert np.array_equal(P, P.T), f"tick {k}: P is not symmetric bit for bit"
        assert np.linalg.eigvalsh(P).min() > 0.0, f"tick {k}"


@pytest.mark.parametrize("name", ROBOTS)
def test_init(runs, name):
    c = runs[(name, DTS[0])]
    s = c["stream"][17]
    cfg = est.cfg()
    for pos0 in (None, (0.4, -0.2, 0.31)):
        f = est.filter_view(est.init(c["model"], cfg, to_struct(s), pos0))
        xr, Pr = ER.init(c["md"], s, pos0)
        assert np.array_equal(f["x"][0:3], [0.0, 0.0, 0.09] if pos0 is None else pos0)
        assert np.array_equal(f["x"][3:6], np.zeros(3))
        assert dev(f["x"], xr) <= 1e-14
        assert np.array_equal(f["P"], 3.0 * np.eye(18)) and np.array_equal(f["P"], Pr)
        assert f["inited"] == 1 and f["ticks"] == 0
        se, o = est.report(c["model"], to_struct(s), est.init(c["model"], cfg, to_struct(s), pos0))
        state_ref, out_ref = ER.report(c["md"], s, xr)
        assert dev(np.frombuffer(bytes(se), dtype=np.float64), state_ref) <= 1e-14
        for k in ("foot_pos_rel", "foot_pos_world", "foot_vel_world"):
            assert dev(np.array(getattr(o, k)), out_ref[k]) <= 1e-13, k
        # feet = R fk + pos, the filter's own foot states
        assert np.array_equal(np.array(o.foot_pos_world), f["x"][6:18])
        assert list(o.estimated_contacts) == list(out_ref["estimated_contacts"]) and o.status == 0


def plant_cases(md, model):
    """(name, state before the step (36), candidate contacts): standing on four feet, and a trot pose on two."""
    q = np.concatenate([np.zeros(6), STAND])
    h = -R.foot_positions(md, q).reshape(4, 3)[:, 2].max()
    stand = np.concatenate([np.zeros(3), [0.0, 0.0, h], STAND, np.zeros(18)])
    jp = STAND.copy()
    jp[3:6] += (0.05, -0.25, 0.45)  # FR and RL lifted
    jp[6:9] += (-0.04, -0.3, 0.5)
    trot = np.concatenate([[0.3, 0.05, -0.04], [0.1, -0.2, h], jp, [0.2, -0.1, 0.15], [0.3, 0.05, -0.02],
                           np.linspace(-1.0, 1.0, 12)])
    return [("stand", stand, (1, 1, 1, 1)), ("trot", trot, (1, 0, 0, 1))]


@pytest.mark.parametrize("name", ROBOTS)
def test_sensor_model_identities_on_plant_steps(name):
    """Exact sensors of a host plant step.  The plant enforces J_C(q) v+ = 0 at the configuration q the step started
    from, so the identities are taken on the state (q, v+): R imu_acc - (0, 0, g) = qdd[0:3]; R fk + pos =
    lmpc_rbd_compute's foot_pos; and for every held foot R leg_v = the base's lin_vel.  All to 1e-12."""
    md, model = model_json(name), preset(name)
    cfg, scfg = est.cfg(), sim.cfg(dt=0.00125, unilateral=False)  # the candidates are held whatever tau does
    tau = np.array([0.5, 4.0, -8.0] * 4)
    for label, s0, contact in plant_cases(md, model):
        nxt, out = sim.step(model, scfg, rbd.state_from_vector(s0), tau, contact)
        assert out.status == 0
        held = list(out.held)
        assert held == list(contact), label
        vplus = np.frombuffer(bytes(nxt), dtype=np.float64)
        hybrid = np.concatenate([s0[0:18], vplus[18:36]])
        # v+ holds the Euler rates; the next state reports them as omega = E(euler+) rates+, the hybrid needs E(euler)
        hybrid[18:21] = R.euler_map(s0[0:3]) @ np.linalg.solve(R.euler_map(vplus[0:3]), vplus[18:21])
        st = rbd.state_from_vector(hybrid)
        sn = est.sensors_from_plant(model, cfg, st, out, 3, 9)
        Rm = ER.rot(hybrid[0:3])
        g = np.array([0.0, 0.0, md["gravity"]])
        assert np.max(np.abs(Rm @ np.array(sn.imu_acc) - g - np.array(out.qdd[0:3]))) <= 1e-12, label
        assert np.max(np.abs(Rm @ np.array(sn.imu_ang_vel) - hybrid[18:21])) <= 1e-12
        assert list(sn.contact) == [float(t != 0) for t in out.touch]
        ref = ER.sensors_from_plant(md, hybrid, np.array(out.qdd), np.array(out.touch))
        for k in ("imu_acc", "imu_ang_vel", "euler", "joint_pos", "joint_vel", "contact"):
            assert dev(np.array(getattr(sn, k)), ref[k]) <= 1e-13, k
        f = est.init(model, cfg, sn, hybrid[3:6])
        se, o = est.report(model, sn, f)
        terms = rbd.terms_dict(rbd.compute(model, st))
        assert np.max(np.abs(np.array(o.foot_pos_world) - terms["foot_pos"])) <= 1e-12, label
        fk = np.array(o.foot_pos_rel).reshape(4, 3)
        # J_leg qd from foot_vel_world = R (J qd) + vel + R (w x fk) with the filter's vel = 0
        for l in range(4):
            if not held[l]:
                continue
            jqd = Rm.T @ np.array(o.foot_vel_world).reshape(4, 3)[l] - np.cross(np.array(sn.imu_ang_vel), fk[l])
            leg_v = -jqd - np.cross(np.array(sn.imu_ang_vel), fk[l])
            assert np.max(np.abs(Rm @ leg_v - hybrid[21:24])) <= 1e-12, (label, l)
        assert sum(held) >= 2


def test_convergence_from_reference_height():
    """A standing robot with exact sensors, the filter initialised at the reference's 0.09 m: the first flat-ground
    update has gain ~ 3 / (3 + 1e-3), so the 0.2 m error falls to ~1e-4 m at once; 1 cm after 100 ticks leaves two
    orders of magnitude."""
    md, model = model_json("go1"), preset("go1")
    _, s0, contact = plant_cases(md, model)[0]
    cfg = est.cfg()
    sn = est.sensors(imu_acc=(0, 0, 9.81), joint_pos=STAND, contact=(1, 1, 1, 1))
    f = est.init(model, cfg, sn)
    assert abs(est.filter_view(f)["x"][2] - s0[5]) > 0.15
    for k in range(100):
        se, o = est.update(model, cfg, sn, f)
        assert o.status == 0
    err = abs(se.pos[2] - s0[5])
    print(f"height error after 100 ticks: {err:.2e} m")
    assert err < 0.01 and f.ticks == 100


def test_noise_keys():
    md, model = model_json("go1"), preset("go1")
    _, s0, contact = plant_cases(md, model)[1]
    st, out = rbd.state_from_vector(s0), N.LmpcSimOut()
    out.qdd[2] = 0.3
    noisy = dict(sigma_acc=0.1, sigma_gyro=0.01, sigma_euler=0.002, sigma_joint_pos=0.001, sigma_joint_vel=0.05)

    def draw(seed, index, tick, **sig):
        return bytes(est.sensors_from_plant(model, est.cfg(seed=seed, **sig), st, out, index, tick))

    base = draw(7, 5, 11, **noisy)
    assert draw(7, 5, 11, **noisy) == base
    assert draw(7, 5, 12, **noisy) != base and draw(7, 6, 11, **noisy) != base and draw(8, 5, 11, **noisy) != base
    exact = draw(7, 5, 11)
    assert draw(12345, 5, 11) == exact and draw(7, 9, 400) == exact and exact != base
    # every channel moves, by about its sigma; the contact flags never do
    a = np.frombuffer(base, dtype=est.SENSORS_DTYPE)[0]
    e = np.frombuffer(exact, dtype=est.SENSORS_DTYPE)[0]
    for k, sg in (("imu_acc", 0.1), ("imu_ang_vel", 0.01), ("euler", 0.002), ("joint_pos", 0.001), ("joint_vel", 0.05)):
        d = np.abs(a[k] - e[k])
        assert np.all(d > 0.0) and np.all(d < 6 * sg), k
    assert np.array_equal(a["contact"], e["contact"])
    # one channel alone draws the first numbers of the stream: the same as with every channel on
    only = np.frombuffer(draw(7, 5, 11, sigma_acc=0.1), dtype=est.SENSORS_DTYPE)[0]
    assert np.array_equal(only["imu_acc"], a["imu_acc"]) and np.array_equal(only["joint_vel"], e["joint_vel"])
    # stand: every flag set whatever touch says
    assert list(est.sensors_from_plant(model, est.cfg(), st, out, 0, 0, stand=True).contact) == [1.0] * 4


def test_status_1_leaves_the_filter(runs):
    c = runs[("go1", DTS[0])]
    cfg = est.cfg()
    f = est.init(c["model"], cfg, to_struct(c["stream"][0]))
    for s in c["stream"][:5]:
        est.update(c["model"], cfg, to_struct(s), f)
    before = bytes(f)
    bad = dict(c["stream"][5])
    bad["imu_acc"] = np.array([0.1, np.nan, 9.8])
    se, o = est.update(c["model"], cfg, to_struct(bad), f)
    assert o.status == 1 and bytes(f) == before
    assert bytes(se) == bytes(N.LmpcRbdState())
    o.status = 0
    assert bytes(o) == bytes(N.LmpcEstOut())
    # a filter that was never initialised
    g = N.LmpcEstFilter()
    se, o = est.update(c["model"], cfg, to_struct(c["stream"][5]), g)
    assert o.status == 1 and bytes(g) == bytes(N.LmpcEstFilter())
    # a negative measurement variance: a non-positive innovation variance
    neg = est.cfg(noise_zfoot=-10.0)
    se, o = est.update(c["model"], neg, to_struct(c["stream"][5]), f)
    assert o.status == 1 and bytes(f) == before
    # and the feedback of a failed update: the plant's block with zero feet and no contact
    so = N.LmpcSimOut()
    so.qdd[0], so.foot_pos[3], so.touch[1], so.held[2] = 1.5, 0.2, 1, 1
    o.status = 1
    sh = est.feedback(so, o)
    assert sh.qdd[0] == 1.5 and sh.held[2] == 1 and list(sh.foot_pos) == [0.0] * 12 and list(sh.touch) == [0] * 4


def test_struct_sizes_and_defaults():
    L = N.lib()
    assert L.lmpc_est_abi_version() == N.EST_ABI_VERSION
    assert (L.lmpc_est_sensors_size(), L.lmpc_est_cfg_size(), L.lmpc_est_filter_size(), L.lmpc_est_out_size()) == \
        (296, 144, 2744, 312)
    assert est.SENSORS_BYTES == 37 * 8
    c = est.cfg()
    assert (c.dt, c.noise_pimu, c.noise_vimu, c.noise_pfoot) == (0.00125, 0.01, 0.01, 0.01)
    assert (c.noise_pimu_rel_foot, c.noise_vimu_rel_foot, c.noise_zfoot) == (0.001, 0.1, 0.001)
    assert (c.gravity, c.drift_threshold, c.drift_divisor, c.init_P, c.assume_flat_ground) == (9.81, 1e-6, 10.0, 3.0, 1)
    assert (c.sigma_acc, c.sigma_gyro, c.sigma_euler, c.sigma_joint_pos, c.sigma_joint_vel, c.seed) == (0, 0, 0, 0, 0, 0)
    for name in N.EST_SYMBOLS:
        assert hasattr(L, name), name


def test_argument_checks():
    L, model, cfg = N.lib(), preset("go1"), est.cfg()
    sn, f, st, so, o = est.sensors(joint_pos=STAND), N.LmpcEstFilter(), N.LmpcRbdState(), N.LmpcSimOut(), N.LmpcEstOut()
    b = ctypes.byref
    ERR_ARG = L.lmpc_est_init(None, b(cfg), b(sn), None, b(f))
    assert ERR_ARG != N.LMPC_OK
    assert L.lmpc_est_init(b(model), b(cfg), b(sn), None, None) == ERR_ARG
    assert L.lmpc_est_update(b(model), b(cfg), None, b(f), b(st), b(o)) == ERR_ARG
    assert L.lmpc_est_update(b(model), b(cfg), b(sn), None, b(st), b(o)) == ERR_ARG
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert L.lmpc_est_update(b(model), b(est.cfg(dt=dt)), b(sn), b(f), b(st), b(o)) == ERR_ARG
    assert L.lmpc_est_update(b(model), b(cfg), b(sn), b(f), None, None) == N.LMPC_OK  # outputs are optional
    assert L.lmpc_est_sensors_from_plant(b(model), b(cfg), b(st), None, 0, 0, 0, b(sn)) == ERR_ARG
    assert L.lmpc_est_sensors_from_plant(b(model), b(est.cfg(sigma_acc=-1.0)), b(st), b(so), 0, 0, 0, b(sn)) == ERR_ARG
    assert L.lmpc_est_report(b(model), b(sn), None, b(st), b(o)) == ERR_ARG
    assert L.lmpc_est_feedback(b(so), None, b(so)) == ERR_ARG
    # batch 0 is fine without any buffer, a negative batch is not
    assert L.lmpc_est_update_device(b(model), b(cfg), None, 0, None, None, None, None, None, None) == N.LMPC_OK
    assert L.lmpc_est_update_device(b(model), b(cfg), None, -1, None, None, None, None, None, None) == ERR_ARG
    assert L.lmpc_est_init_device(b(model), b(cfg), None, None, 0, 0, None, None, None, None, None, None) == N.LMPC_OK
    assert L.lmpc_est_sensors_from_plant_device(b(model), b(cfg), None, None, 0, 0, 0, None, 0, None, None) == N.LMPC_OK
    assert L.lmpc_est_sensors_from_plant_device(b(model), b(cfg), None, None, -2, 0, 0, None, 0, None, None) == ERR_ARG
    with pytest.raises(TypeError):
        est.cfg(no_such_field=1.0)


def test_shared_header_under_sanitizers():
    """tests/cpp/est_host_check.cpp includes csrc/lmpc_est_common.h and runs a few filters; built by the host compiler
    with -fsanitize=address,undefined and run directly (nothing loaded into Python is instrumented)."""
    from legged_mpc_control_amd import build as B

    exe = B.build_cpp_est_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "est_host_check ok" in r.stdout and "runtime error" not in r.stderr
