"""Reference values for the per-body contact-force output (ss_set_contact_force_output), shared by test_contact_force_emu.py and
test_contact_force_gpu.py (test infrastructure).

The reference is the float64 oracle doing what the reference's loop does from the pre-step state the stepper held: 15 x (spd_torque,
ctrl, mj_step), then mjData.efc_force of the last mj_step.  Contact rows are the last 4 * ncon rows of efc_force, four per contact in
the order of make_constraints (oracle.c): n + mu t1, n - mu t1, n + mu t2, n - mu t2 with n, t1, t2 the rows of con_frame.  A contact's
force is added to con_body and, for a body-body contact (con_body1 >= 0), subtracted from con_body1.

Error measure (per env): max_b |F - F_ref|_inf / max(W, max_b |F_ref|_inf), W the model's total weight.
Gates: 3 x the worst measured sample (profiles/contact_force.txt), the float64 one capped at 1e-6.
"""
import numpy as np

from oracle import oracle as O

# 3 x the worst sample of profiles/contact_force.txt.  On the CPU: the test cases plus every env-step of two rollouts of the
# benchmark's state distributions (256 floor-only, 256 self-collision; episode ends and bad-state resets included).  float64: none
# left out, worst 1.527e-12 (the condition on this gate: <= 1e-6; a float64 deviation above that is a defect, not noise).  float32
# emulator: one env-step of the 512 left out and listed there (a state blowing up inside the step: 1.6e-1 at 95 Newton iterations),
# worst of the rest 3.292e-4.  On the GPU: over its test cases, worst 1.212e-05.
GATE_F64 = 4.6e-12
GATE_F32_EMU = 9.9e-4
GATE_GPU = 3.64e-05
PRE_FIELDS = ("qpos", "qvel", "qpos_prev", "qvel_prev", "qacc_warm")


def weight(mc):
    return float(np.sum(mc.body_mass) * abs(mc.gravity))


def oracle_contact_force(om, mu, pre, action, nsub=15):
    """pre: dict of the env's pre-step qpos, qvel, qpos_prev, qvel_prev, qacc_warm (float64).  Returns (F [nbody, 3], info) with
    info = dict(floor_sum [3], n_floor, n_self_loaded, loaded bodies, iters of the last mj_step, nwarn, qpos, qvel)."""
    d = O.OracleData(om)
    d.qpos = pre["qpos_prev"]; d.qvel = pre["qvel_prev"]; d.forward()          # stale M, C of the last mj_forward
    d.qpos = pre["qpos"]; d.qvel = pre["qvel"]; d.warm = pre["qacc_warm"]
    for _ in range(nsub):
        d.ctrl = d.spd_torque(action); d.step()
    nefc, ncon = int(d.get(O.D_NEFC)[0]), d.ncon
    ef = d.get(O.D_EFC_FORCE)[nefc - 4 * ncon:nefc].reshape(ncon, 4)
    fr, b2, b1 = d.con_frame, d.con_body, d.con_body1
    F = np.zeros((om.nbody, 3))
    floor_sum, n_self_loaded = np.zeros(3), 0
    for c in range(ncon):
        n, t1, t2 = fr[c]
        f = ef[c, 0] * (n + mu * t1) + ef[c, 1] * (n - mu * t1) + ef[c, 2] * (n + mu * t2) + ef[c, 3] * (n - mu * t2)
        F[b2[c]] += f
        if b1[c] >= 0:
            F[b1[c]] -= f
            n_self_loaded += bool(np.abs(f).max() > 0)
        else:
            floor_sum += f
    return F, dict(floor_sum=floor_sum, n_floor=int((b1 < 0).sum()), n_self_loaded=n_self_loaded, loaded=np.nonzero(np.abs(F).max(axis=1) > 0)[0],
                   iters=d.solver_iter, nwarn=d.nwarn, qpos=d.qpos, qvel=d.qvel)


def force_error(F, F_ref, W):
    return float(np.abs(np.asarray(F, np.float64) - F_ref).max() / max(W, np.abs(F_ref).max()))


def pre_of(eb, i):
    """Pre-step state of env i of an emulator batch (or any object with the five state arrays as numpy)."""
    return {k: np.asarray(getattr(eb, k)[i], np.float64).copy() for k in PRE_FIELDS}
