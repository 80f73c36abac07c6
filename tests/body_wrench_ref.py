"""References for the body-wrench input (ss_set_body_wrench_input, MuJoCo's xfrc_applied), shared by test_body_wrench_emu.py and
test_body_wrench_gpu.py (test infrastructure).  The oracle has no applied-force input; both references are built from what it has.

R1  J^T w from the oracle's own velocity kinematics.  With qvel = e_i the oracle's forward() gives the frame-origin velocity (linvel)
    and the angular velocity (angvel) of every body in the world frame, so  v_com,b = linvel_b + angvel_b x (xipos_b - xpos_b)  is
    column i of the centre-of-mass Jacobian and  (J^T w)_i = sum_b f_b . v_com,b + tau_b . angvel_b.  Without active constraints
    (the callers assert ncon == 0 and NEFC == 0)  qacc_ref = qacc of the oracle without the wrench + solve(M, J^T w).
R2  A gravity twin.  f_b = (0, 0, -m_b d) on every body is a model with gravity -(9.81 + d): forward_kin applies gravity per body at
    the centre of mass.  Holds with contacts and limits, for controllers that do not read the bias (pd, torque) only.

Error measures: qacc, and qvel after one mj_step / one control step:  max |x - x_ref| / max(1, max |x_ref|);  qpos: max |x - x_ref|.
The contact cases (R2) use the per-step parity tests' measures and tolerances (test_gpu_parity.py: max |dqpos| < TOL_QPOS, max |dqvel| < TOL_QVEL).
"""
import contextlib
import ctypes as C
import functools

import numpy as np

from helpers import default_qpos, model_const, pd_tables
from oracle import oracle as O
from smplsim_amd import _cabi
from smplsim_amd.mjcf_writer import default_xml_str

# Gates.  float64 emulator: a condition, not a measurement — a float64 deviation above 1e-8 from R1 / R2 is a defect of the kernel or
# of the reference helper, not noise (measured worst over the cases of test_body_wrench_emu.py: see profiles/body_wrench.txt).
# float32 emulator and GPU, cases 1 to 3: 3 x the worst sample of profiles/body_wrench.txt over the listed cases, none left out.
GATE_F64 = 1e-8
# float32 emulator, worst samples: qacc 7.036e-06 (SMPL-X, random wrench), qvel after one mj_step 5.215e-06, after the control step
# qpos 1.645e-07 and qvel 1.014e-06.
GATE_F32_EMU = dict(qacc=2.12e-05, sub_qvel=1.57e-05, step_qpos=4.94e-07, step_qvel=3.05e-06)
# GPU, worst samples: qacc 7.265e-06 (SMPL-X, random wrench), qvel after one mj_step 1.206e-05, after the control step qpos 2.018e-07
# and qvel 5.276e-07.
GATE_GPU = dict(qacc=2.18e-05, sub_qvel=3.62e-05, step_qpos=6.06e-07, step_qvel=1.59e-06)
TOL_QPOS, TOL_QVEL, TOL_OBS = 1e-5, 2e-3, 2e-3               # the project's per-step parity tolerances (test_gpu_parity.py)
EFFECT = 100.0                                                # every compared case: effect of the wrench on the compared quantity >= EFFECT x its gate
G = 9.81


def rel_err(x, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def abs_err(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64)).max())


def weight(mc):
    return float(np.sum(mc.body_mass) * G)


def airborne(mc, seed, vel=0.1):
    """Root 2 m above the floor, joint angles uniform within +-0.3 rad (inside every limit), small random velocities."""
    rs = np.random.default_rng(seed)
    q = default_qpos(mc.nq); q[2] = 2.0
    q[7:] = rs.uniform(-0.3, 0.3, mc.nq - 7)
    return q, rs.normal(size=mc.nv) * vel


def wrench_cases(mc, seed=5):
    """name -> wrench [nbody, 6] of case 1 (the weight-cancelling one is run at zero velocity and zero torque)."""
    rs = np.random.default_rng(seed)
    nb, W, names = mc.nbody, weight(mc), list(mc.body_names)
    z = lambda: np.zeros((nb, 6))
    out = {"random_all": np.concatenate([rs.uniform(-1, 1, (nb, 3)) * W / 4 / np.sqrt(3), rs.uniform(-1, 1, (nb, 3)) * 20 / np.sqrt(3)], axis=1)}
    if "R_Hand" in names:                                     # (the SMPL-X humanoid's hands are made of finger bodies)
        w = z(); w[names.index("R_Hand"), :3] = (30.0, -20.0, 40.0); out["force_R_Hand"] = w
    w = z(); w[names.index("L_Toe"), 3:] = (3.0, -2.0, 4.0); out["torque_L_Toe"] = w
    w = z(); w[0, :3] = (100.0, 50.0, -80.0); out["force_root"] = w
    w = z(); w[:, 2] = np.asarray(mc.body_mass) * G; out["weight_cancel"] = w
    return out


def no_constraints(d):
    return d.ncon == 0 and int(d.get(O.D_NEFC)[0]) == 0


def jt_wrench(om, qpos, wrench):
    """R1: J^T w [nv] at qpos."""
    d = O.OracleData(om)
    w = np.asarray(wrench, np.float64)
    out = np.zeros(om.nv)
    for i in range(om.nv):
        e = np.zeros(om.nv); e[i] = 1.0
        d.qpos = qpos; d.qvel = e; d.forward()
        ang = d.angvel
        vcom = d.linvel + np.cross(ang, d.xipos - d.xpos)
        out[i] = np.sum(w[:, :3] * vcom) + np.sum(w[:, 3:] * ang)
    return out


def qacc_ref(om, qpos, qvel, tau, wrench):
    """(qacc with the wrench, qacc without it) of one forward at (qpos, qvel) under joint torques tau [nu]; asserts no constraint is active."""
    d = O.OracleData(om)
    d.qpos = qpos; d.qvel = qvel; d.ctrl = tau; d.forward()
    assert no_constraints(d)
    a0 = d.qacc
    return a0 + np.linalg.solve(d.M, jt_wrench(om, qpos, wrench)), a0


def integrate(qpos, qvel, qacc, dt):
    """Semi-implicit Euler as mj_Euler / mj_integratePos: the free joint's quaternion turns by the LOCAL angular velocity."""
    v = qvel + dt * qacc
    q = qpos.copy()
    q[:3] += dt * v[:3]
    w = v[3:6]; n = np.linalg.norm(w)
    ax = w / n if n > 0 else np.array([1.0, 0, 0])
    h = 0.5 * dt * n
    qr = np.array([np.cos(h), *(np.sin(h) * ax)])
    a = q[3:7] / np.linalg.norm(q[3:7])
    q[3:7] = [a[0] * qr[0] - a[1:] @ qr[1:], *(a[0] * qr[1:] + qr[0] * a[1:] + np.cross(a[1:], qr[1:]))]
    q[7:] += dt * v[6:]
    return q, v


def spd_steps_ref(om, qpos, qvel, action, wrench, nsub, dt=1.0 / 450, wrong=False):
    """nsub mj_steps under uhc_pd from (qpos, qvel) after an mj_forward there, airborne (asserted at every step): per mj_step
    tau = spd_torque on the stale M and bias, forward, qacc = oracle's + solve(M, J^T w) with R1 rebuilt at this state, Euler.
    wrong=True: the reference a kernel would match that folds the wrench into the bias the SPD solve reads (bias - J^T w)."""
    d = O.OracleData(om)
    d.qpos = qpos; d.qvel = qvel; d.forward()
    jt = jt_wrench(om, qpos, wrench)
    for _ in range(nsub):
        if wrong:
            d.bias = d.bias - jt                              # (jt is of the state of the last forward, as the bias is)
        d.ctrl = d.spd_torque(action); d.forward()
        assert no_constraints(d)
        q, v = d.qpos, d.qvel
        jt = jt_wrench(om, q, wrench)
        q, v = integrate(q, v, d.qacc + np.linalg.solve(d.M, jt), dt)
        d.qpos = q; d.qvel = v
    return q, v


@contextlib.contextmanager
def _gravity(g):
    """OracleModel.__init__ fills O._Desc with gravity=-9.81: while this is open, the description it fills takes g instead."""
    O.lib()                                                   # (binds om_model_create to the real O._Desc first)
    base = O._Desc
    O._Desc = lambda **kw: base(**{**kw, "gravity": g})
    try:
        yield
    finally:
        O._Desc = base


def twin_model(name, d, control_mode="pd", self_collision=False, mc=None, xml=None, **gain_kw):
    """R2: the oracle's model with gravity -(9.81 + d)."""
    mc = mc or model_const(name)
    kp, kd, tl, sc, of = pd_tables(mc, control_mode=control_mode, **gain_kw)
    from helpers import FEET
    with _gravity(-(G + d)):
        return O.OracleModel(xml or default_xml_str(name), kp, kd, tl, sc, of, legal_bodies=FEET, self_collision=self_collision)


def twin_wrench(mc, d):
    w = np.zeros((mc.nbody, 6)); w[:, 2] = -np.asarray(mc.body_mass) * d
    return w


def twin_step(om, control_mode_id, pre, action):
    """One control step of the oracle env on model om from the recorded pre-step state; returns (qpos, qvel)."""
    e = O.OracleEnv(om, control_mode=control_mode_id)
    e.reset()
    dd = e.data
    dd.qpos = pre["qpos_prev"]; dd.qvel = pre["qvel_prev"]; dd.forward()
    dd.qpos = pre["qpos"]; dd.qvel = pre["qvel"]; dd.warm = pre["qacc_warm"]
    e.step(action)
    return dd.qpos, dd.qvel


@functools.lru_cache(maxsize=None)
def qacc_cases():
    """Case 1, computed once: (name, humanoid, qpos, qvel, tau, wrench, qacc_ref, qacc without the wrench).  smpl_humanoid under
    every wrench, smplx_humanoid under the random one; the weight-cancelling wrench at zero velocity and zero torque."""
    from helpers import oracle_model
    out = []
    for hum, names in (("smpl_humanoid", None), ("smplx_humanoid", ("random_all",))):
        mc, om = model_const(hum), oracle_model(hum)
        q, v = airborne(mc, 1)
        tau = np.random.default_rng(2).normal(size=mc.nu) * 2.0
        for name, w in wrench_cases(mc).items():
            if names and name not in names:
                continue
            vv, tt = (v * 0, tau * 0) if name == "weight_cancel" else (v, tau)
            ref, ref0 = qacc_ref(om, q, vv, tt, w)
            out.append((name, hum, q, vv, tt, w, ref, ref0))
    return out


def qacc_err(name, qacc, ref):
    """Case 1's measure; the weight-cancelling case: qacc must vanish against the scale 9.81."""
    return float(np.abs(np.asarray(qacc, np.float64)).max() / G) if name == "weight_cancel" else rel_err(qacc, ref)


SPD_WRENCH = ("R_Hand", (60.0, -40.0, 80.0))                  # cases 2 and 3: a force on the hand loads the arm's joints, which the SPD gains act on


@functools.lru_cache(maxsize=None)
def spd_cases():
    """Cases 2 and 3, computed once: dict(q, v, action, wrench, sub = (qvel after one mj_step: right, wrong, without the wrench),
    step = (qpos, qvel after 15 mj_steps; the same without the wrench))."""
    from helpers import oracle_model
    mc, om = model_const(), oracle_model()
    q, v = airborne(mc, 3)
    a = np.random.default_rng(4).uniform(-0.3, 0.3, mc.nu)
    w = np.zeros((mc.nbody, 6)); w[list(mc.body_names).index(SPD_WRENCH[0]), :3] = SPD_WRENCH[1]
    sub = tuple(spd_steps_ref(om, q, v, a, ww, 1, wrong=wr)[1] for ww, wr in ((w, False), (w, True), (0 * w, False)))
    return dict(q=q, v=v, action=a, wrench=w, sub=sub, step=spd_steps_ref(om, q, v, a, w, 15) + spd_steps_ref(om, q, v, a, 0 * w, 15))


def attach(eb, wrench):
    """Hand an emulator batch the wrench [N, nbody, 6] (kept alive on the batch, in its float type); None = off."""
    _cabi.bind_wrench(eb.L)                                   # (the emulator front end binds smplsim_hip.h and smplsim_motion.h)
    eb.xfrc = None if wrench is None else np.ascontiguousarray(wrench, eb.ft)
    eb._chk(eb.L.ss_set_body_wrench_input(eb.batch, None if wrench is None else eb.xfrc.ctypes.data_as(C.c_void_p)))
    return eb.xfrc
