"""Robot models and settings off the two presets (TEST INFRASTRUCTURE ONLY), for the rigid-body, plant, contact and
estimator kernels.

Go1 and A1 have four legs that are copies or mirror images of each other: foot[l] is one vector, the link masses and
the calf's centre of mass and inertia repeat from leg to leg, every joint_origin has one or two exact zeros, and gravity
is 9.81 everywhere.  The device kernels index the model by the lane's leg (lmpc_sim::lane_model, the estimator's
copy, lmpc_rbd_kernel), the host loops over legs: a wrong leg index on the device cannot show on these two robots.  The
models below are derived from the Go1 fixture by seeded code, in the fixtures' JSON layout (rbd.model_from_json):

  * lopsided -- everything at once: no two legs alike in any field, no zero left in joint_origin or foot, full
    inertias on all 13 bodies, gravity 9.7;
  * feet     -- only foot[l] differs per leg, x and y non-zero;
  * bodies   -- only the legs' masses, centres of mass and inertias differ;
  * origins  -- only joint_origin differs per leg, all three components non-zero.

The settings are plain dicts: the estimator's noises all different (a swap of two cannot cancel), its gravity, drift
rule and init_P off default; the contact model around ground_z = 0.37 with and without recover_speed; the plant's
ground off zero; WBC targets whose torque limits, mu and swing gains differ from robot to robot.  DEFECTS are the
mistakes the sets exist to catch, written as changes to a model or to a configuration: tests/test_models_host.py shows
that each leaves the presets' answers bit for bit as they are and moves the targeted set's.
"""
import copy
import functools

import numpy as np

import rbd_ref as R
from test_rbd_host import make_targets, model_json

LEG_FIELDS = ("foot", "mass", "com", "inertia", "joint_origin")
VARIES = {"lopsided": LEG_FIELDS, "feet": ("foot",), "bodies": ("mass", "com", "inertia"), "origins": ("joint_origin",)}
NAMES = tuple(VARIES)
SINGLE = ("feet", "bodies", "origins")

MASS_SCALE = (0.7, 1.0, 1.4, 1.9)      # a light leg and a heavy one
ORIGIN_SCALE = (0.85, 1.0, 1.15, 1.3)
FOOT_SCALE = (0.8, 1.0, 1.2, 1.35)


def _box_inertia(rng, six):
    """A random rotation of a box's moments with the trace's size kept: positive definite, and the triangle inequality
    holds."""
    I = R._inertia(six)
    Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    rng.uniform(0.6, 1.6, 3)  # a draw the measured recipe made and did not use; removing it changes every later draw
    d = rng.uniform(0.5, 1.5, 3) * np.trace(I) / 6
    I2 = Q @ np.diag([d[1] + d[2], d[0] + d[2], d[0] + d[1]]) @ Q.T
    return [I2[0, 0], I2[0, 1], I2[0, 2], I2[1, 1], I2[1, 2], I2[2, 2]]


def _write(md, **arrays):
    for k, a in arrays.items():
        md[k] = np.asarray(a).tolist()
    return md


def _lopsided(seed=7):
    md = copy.deepcopy(model_json("go1"))
    rng = np.random.default_rng(seed)
    md["name"], md["gravity"] = "lopsided", 9.7
    mass = np.array(md["mass"])
    mass[0] *= 1.3
    for l in range(4):
        mass[1 + 3 * l:4 + 3 * l] *= MASS_SCALE[l] * rng.uniform(0.9, 1.1, 3)
    com = np.array(md["com"]) + rng.uniform(-0.02, 0.02, (13, 3))
    inertia = [_box_inertia(rng, md["inertia"][b]) for b in range(13)]
    jo = np.array(md["joint_origin"])
    for l in range(4):
        jo[3 * l:3 * l + 3] *= ORIGIN_SCALE[l]
    jo += rng.uniform(-0.03, 0.03, jo.shape)
    foot = np.array(md["foot"]) * np.array(FOOT_SCALE)[:, None] + rng.uniform(-0.03, 0.03, (4, 3))
    return _write(md, mass=mass, com=com, inertia=inertia, joint_origin=jo, foot=foot)


def _feet(seed=11):
    md = copy.deepcopy(model_json("go1"))
    rng = np.random.default_rng(seed)
    md["name"] = "feet"
    foot = np.array(md["foot"]) * np.array(FOOT_SCALE)[:, None] + rng.uniform(-0.03, 0.03, (4, 3))
    return _write(md, foot=foot)


def _bodies(seed=12):
    md = copy.deepcopy(model_json("go1"))
    rng = np.random.default_rng(seed)
    md["name"] = "bodies"
    mass, com, inertia = np.array(md["mass"]), np.array(md["com"]), [list(x) for x in md["inertia"]]
    for l in range(4):
        mass[1 + 3 * l:4 + 3 * l] *= MASS_SCALE[l] * rng.uniform(0.9, 1.1, 3)
    com[1:] += rng.uniform(-0.02, 0.02, (12, 3))
    for b in range(1, 13):
        inertia[b] = _box_inertia(rng, md["inertia"][b])
    return _write(md, mass=mass, com=com, inertia=inertia)


def _origins(seed=13):
    md = copy.deepcopy(model_json("go1"))
    rng = np.random.default_rng(seed)
    md["name"] = "origins"
    jo = np.array(md["joint_origin"])
    for l in range(4):
        jo[3 * l:3 * l + 3] *= ORIGIN_SCALE[l]
    jo += rng.uniform(-0.03, 0.03, jo.shape)
    return _write(md, joint_origin=jo)


@functools.lru_cache(maxsize=None)
def _models():
    out = {"lopsided": _lopsided(), "feet": _feet(), "bodies": _bodies(), "origins": _origins()}
    for name, md in out.items():
        check(md, VARIES[name])
    return out


def model(name):
    """The model dict of a set ("go1" and "a1": the fixtures); a fresh copy, the caller may change it."""
    if name in ("go1", "a1"):
        return model_json(name)
    return copy.deepcopy(_models()[name])


def leg_rows(md, field, leg):
    """The rows of `field` that belong to `leg`, as an array."""
    a = np.asarray(md[field], dtype=np.float64)
    if field == "foot":
        return a[leg]
    if field == "joint_origin":
        return a[3 * leg:3 * leg + 3]
    return a[1 + 3 * leg:4 + 3 * leg]


def check(md, varies):
    """Masses positive; every inertia positive definite with the triangle inequality; no two legs equal -- no two
    legs share a single number -- in the fields the set says it varies; the other fields are Go1's."""
    go1 = model_json("go1")
    assert len(md["mass"]) == 13 and np.all(np.asarray(md["mass"]) > 0.0)
    for six in md["inertia"]:
        ev = np.linalg.eigvalsh(R._inertia(six))
        assert ev[0] > 0.0 and ev[0] + ev[1] >= ev[2] * (1.0 - 1e-12), f"not a rigid body's inertia: {ev}"
    for field in LEG_FIELDS:
        if field not in varies:
            assert md[field][1 if field in ("mass", "com", "inertia") else 0:] == \
                go1[field][1 if field in ("mass", "com", "inertia") else 0:], field
            continue
        for a in range(4):
            for b in range(a + 1, 4):
                assert np.all(leg_rows(md, field, a) != leg_rows(md, field, b)), (field, a, b)
        if field in ("foot", "joint_origin"):
            assert np.all(np.asarray(md[field]) != 0.0), field
    if "inertia" in varies:
        assert np.all(np.asarray(md["inertia"])[1:] != 0.0)
    return md


# ---- settings --------------------------------------------------------------------------------------------------------
# the estimator: six different noises, its own gravity, the drift rule and init_P off default
EST = dict(noise_pimu=0.02, noise_vimu=0.005, noise_pfoot=0.03, noise_pimu_rel_foot=0.002, noise_vimu_rel_foot=0.07,
           noise_zfoot=0.0004, gravity=9.7, drift_threshold=2e-6, drift_divisor=7.0, init_P=2.0)
# groups of noises that are equal by default: a swap inside a group cannot fail a test that runs on the defaults
EST_EQUAL_BY_DEFAULT = (("noise_pimu", "noise_vimu"), ("noise_pimu", "noise_pfoot"), ("noise_vimu", "noise_pfoot"),
                        ("noise_pimu_rel_foot", "noise_zfoot"))


def est_cfg(flat=1, **over):
    """The estimator's off-default settings as est_ref's dict (assume_flat_ground included)."""
    return dict(EST, assume_flat_ground=bool(flat), **over)


def est_struct(cfg, dt):
    from legged_mpc_control_amd import est

    fields = {k: v for k, v in cfg.items() if k != "assume_flat_ground"}
    return est.cfg(dt=dt, assume_flat_ground=cfg["assume_flat_ground"], **fields)


GROUND_Z = 0.37
FORCE_THRESHOLD = 5.0
# the contact model: test_gpu_contact.CFGS around a ground off zero, "gap" with the penetration recovery clipped
CONTACT = {"gap": dict(mu=0.6, use_gap=1, touch_rule=1, force_threshold=FORCE_THRESHOLD, recover_speed=0.5,
                       ground_z=GROUND_Z),
           "flat": dict(mu=0.3, use_gap=0, touch_rule=0, force_threshold=FORCE_THRESHOLD, recover_speed=0.0,
                        ground_z=GROUND_Z)}
SIM_GROUND_Z = -0.23  # the plant's ground for the device pools (the states are shifted so that feet lie on both sides)


def contact_struct(cfg, dt):
    from legged_mpc_control_amd import contact

    return contact.cfg(dt=dt, **cfg)


def wbc_targets(count, seed):
    """test_rbd_host.make_targets plus, per robot, three different torque limits, mu and the swing gains."""
    rng = np.random.default_rng(seed + 1000)
    out = make_targets(count, seed)
    for t in out:
        t.update(torque_limits=rng.uniform(15.0, 45.0, 3) * [1.0, 1.3, 1.7], mu=rng.uniform(0.2, 0.9),
                 swing_kp=rng.uniform(100.0, 400.0), swing_kd=rng.uniform(3.0, 40.0))
    return out


# ---- the defects the sets exist to catch -----------------------------------------------------------------------------
def _foot_leg0(md):
    md["foot"] = [list(md["foot"][0]) for _ in range(4)]


def _mass_leg0(md):
    md["mass"] = [md["mass"][0]] + list(md["mass"][1:4]) * 4


def _calf_leg0(md):
    for l in range(4):
        md["com"][3 + 3 * l], md["inertia"][3 + 3 * l] = list(md["com"][3]), list(md["inertia"][3])


def _calf_origin_leg0(md):
    for l in range(4):
        md["joint_origin"][3 * l + 2] = list(md["joint_origin"][2])


def _origin_zeros(md):
    """The components that are exactly zero on the presets are read as zero."""
    zero = np.asarray(model_json("go1")["joint_origin"]) == 0.0
    assert np.array_equal(zero, np.asarray(model_json("a1")["joint_origin"]) == 0.0)
    md["joint_origin"] = np.where(zero, 0.0, np.asarray(md["joint_origin"])).tolist()


def _foot_zeros(md):
    md["foot"] = [[0.0, 0.0, f[2]] for f in md["foot"]]


# name -> (change to the model dict, the single-aspect set it targets)
MODEL_DEFECTS = {"leg 0's foot in every leg": (_foot_leg0, "feet"),
                 "foot x and y read as zero": (_foot_zeros, "feet"),
                 "leg 0's masses in every leg": (_mass_leg0, "bodies"),
                 "leg 0's calf com and inertia in every leg": (_calf_leg0, "bodies"),
                 "leg 0's calf joint_origin in every leg": (_calf_origin_leg0, "origins"),
                 "the presets' zero components of joint_origin read as zero": (_origin_zeros, "origins")}


def defective(name, defect):
    md = model(name)
    MODEL_DEFECTS[defect][0](md)
    return md
