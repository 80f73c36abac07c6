"""The body-wrench input (ss_set_body_wrench_input, MuJoCo's xfrc_applied) on the wavefront emulator, float64 and float32 builds,
against references built from the float64 oracle (body_wrench_ref.py: R1 = J^T w from the oracle's velocity kinematics, R2 = a gravity
twin; error measures, gates; the measured samples: profiles/body_wrench.txt).  GPU twin: test_body_wrench_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import body_wrench_ref as R
from helpers import FEET, model_const, pd_tables
from smplsim_amd import _cabi
from wave_emu import emu

BOTH = pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])


def _gate(f64, key):
    return R.GATE_F64 if f64 else R.GATE_F32_EMU[key]


def _batch(n, f64, humanoid="smpl_humanoid", control_mode="uhc_pd", pdp_scale=1.0, pdd_scale=1.0, **kw):
    mc = model_const(humanoid)
    return mc, emu.EmuBatch(mc, pd_tables(mc, control_mode=control_mode, pdp_scale=pdp_scale, pdd_scale=pdd_scale), n, legal_bodies=FEET, f64=f64, control_mode=_cabi.CONTROL_MODES[control_mode], **kw)


def _check(case, f64, key, err, effect):
    print(f"body-wrench sample: {case} {'f64' if f64 else 'f32'} {key} err {err:.3e} effect {effect:.3e}")
    assert effect >= R.EFFECT * _gate(f64, key), (case, key, effect)   # a condition on the inputs: a kernel that ignores the wrench cannot pass
    assert err <= _gate(f64, key), (case, key, err)


# ---- case 1: qacc of ss_debug_forward against R1
@BOTH
def test_qacc_unconstrained(f64):
    batches = {}
    for name, hum, q, v, tau, w, ref, ref0 in R.qacc_cases():
        if hum not in batches:
            batches[hum] = _batch(1, f64, hum)[1]
        eb = batches[hum]
        eb.set_state(q[None], v[None])
        R.attach(eb, None)
        _, bias0, _ = eb.debug_forward(tau[None])
        R.attach(eb, w[None])
        _, bias, qacc = eb.debug_forward(tau[None])
        assert np.array_equal(bias, bias0), name              # qfrc_bias does not contain the wrench
        _check(f"qacc {hum} {name}", f64, "qacc", R.qacc_err(name, qacc[0], ref), R.qacc_err(name, ref0, ref) if name == "weight_cancel" else R.rel_err(ref0, ref))


# ---- case 2: one mj_step under uhc_pd — the controller does not see the wrench
@BOTH
def test_spd_controller_does_not_see_the_wrench(f64):
    c = R.spd_cases()
    right, wrong, without = c["sub"]
    mc, eb = _batch(1, f64)
    eb.set_state(c["q"][None], c["v"][None])
    R.attach(eb, c["wrench"][None])
    eb.substep(c["action"][None], 1)
    assert R.rel_err(wrong, right) >= R.EFFECT * _gate(f64, "sub_qvel")      # the two references can be told apart
    print(f"body-wrench sample: substep right-vs-wrong reference {R.rel_err(wrong, right):.3e}")
    _check("substep uhc_pd", f64, "sub_qvel", R.rel_err(eb.qvel[0], right), R.rel_err(without, right))


# ---- case 3: a whole control step under uhc_pd, airborne
@BOTH
def test_control_step_airborne(f64):
    c = R.spd_cases()
    q_ref, v_ref, q0, v0 = c["step"]
    mc, eb = _batch(1, f64)
    eb.set_state(c["q"][None], c["v"][None])
    R.attach(eb, c["wrench"][None])
    eb.step(c["action"][None])
    assert eb.nwarn[0] == 0
    _check("control step uhc_pd", f64, "step_qpos", R.abs_err(eb.qpos[0], q_ref), R.abs_err(q0, q_ref))
    _check("control step uhc_pd", f64, "step_qvel", R.rel_err(eb.qvel[0], v_ref), R.rel_err(v0, v_ref))


# ---- case 4: contacts, R2 (gravity twin), control_mode pd
# The gains: explicit PD with the Stable-PD gain table amplifies a difference ~15 x per mj_step on the armature-dominated links
# (test_gpu_parity.py::test_pd_and_torque_controllers_on_gpu), so a control step of 15 mj_steps is not comparable in float32 whatever
# the wrench — the d = 0 control misses TOL_QVEL by four orders.  With the table divided by 10 (the reference's pdp_scale / pdd_scale)
# explicit PD is stable at 450 Hz and the control passes on these states with two orders to spare (profiles/body_wrench.txt).
PD_SCALE = dict(pdp_scale=10.0, pdd_scale=10.0)
D_TWIN = (0.3 * R.G, -0.3 * R.G, 0.0)


@functools.lru_cache(maxsize=None)
def contact_states(which):
    """Pre-step state and action of the compared step of test_contact_force_emu.standing / lying (same seeds; float64 run)."""
    import test_contact_force_emu as T
    if which == "folded":                                     # its folded poses with a loaded body-body contact (not a case of the issue's list)
        mc, om, pre, acts = T.self_states(2)
        return pre, np.asarray(acts, np.float64)
    mc, eb, pre, acts = (T.standing if which == "standing" else T.lying)(True)
    return pre, np.asarray(acts, np.float64)


@functools.lru_cache(maxsize=None)
def twin_refs(which, d, self_collision=False):
    pre, acts = contact_states(which)
    om = R.twin_model("smpl_humanoid", d, self_collision=self_collision, **PD_SCALE)
    return [R.twin_step(om, _cabi.CTRL_PD, pre[i], acts[i]) for i in range(len(pre))]


def set_pre(eb, pre):
    eb.set_state(*[np.array([p[k] for p in pre]) for k in ("qpos", "qvel", "qpos_prev", "qvel_prev", "qacc_warm")])


def check_twin(case, d, qpos, qvel, touch, ref, ref0, tq, tv):
    """One case = one batch: every env within (tq, tv) of the twin; the twin's distance from the ordinary oracle, over the batch, at
    least EFFECT x the tolerances (standing: two of the three envs are between two foot contacts at the end of the step and merely
    fall d dt faster, 0.098 m/s — the env on its foot carries the case); returns the per-env errors."""
    errs, fq, fv = [], 0.0, 0.0
    for i in range(len(ref)):
        eq, ev = R.abs_err(qpos[i], ref[i][0]), R.abs_err(qvel[i], ref[i][1])
        gq, gv = R.abs_err(ref0[i][0], ref[i][0]), R.abs_err(ref0[i][1], ref[i][1])
        fq, fv = max(fq, gq), max(fv, gv)
        print(f"body-wrench sample: twin {case} d {d:+.3f} env {i} qpos err {eq:.3e} effect {gq:.3e} qvel err {ev:.3e} effect {gv:.3e} touch {int(touch[i]) & 0xFFFFFFFF:#x}")
        errs.append((eq, ev))
    assert any(int(t) != 0 for t in touch), case              # in contact with the floor
    if d:
        assert fq >= R.EFFECT * tq and fv >= R.EFFECT * tv, (case, d, fq, fv)
    for i, (eq, ev) in enumerate(errs):
        assert eq <= tq and ev <= tv, (case, d, i, eq, ev)
    return errs


@BOTH
@pytest.mark.parametrize("which", ["standing", "lying"])
@pytest.mark.parametrize("d", D_TWIN, ids=["heavier", "lighter", "control"])
def test_contacts_gravity_twin(f64, which, d):
    pre, acts = contact_states(which)
    n = len(pre)
    mc, eb = _batch(n, f64, control_mode="pd", **PD_SCALE)
    set_pre(eb, pre)
    R.attach(eb, np.tile(R.twin_wrench(mc, d), (n, 1, 1)))
    eb.step(acts)
    assert not eb.nwarn.any()
    tq, tv = (R.GATE_F64, R.GATE_F64) if f64 else (R.TOL_QPOS, R.TOL_QVEL)
    check_twin(f"{which} {'f64' if f64 else 'f32'}", d, eb.qpos, eb.qvel, eb.touch[:, 0], twin_refs(which, d), twin_refs(which, 0.0), tq, tv)


# The lying humanoid does not touch itself.  Body-body contact rows under a wrench: the folded poses of test_contact_force_emu.py with
# self_collision on, d = +0.6 x 9.81 (at 0.3 the twin moves qvel by 0.15, short of 100 x TOL_QVEL) and the d = 0 control.
D_FOLDED = (0.6 * R.G, 0.0)


@BOTH
@pytest.mark.parametrize("d", D_FOLDED, ids=["heavier", "control"])
def test_body_body_contacts_gravity_twin(f64, d):
    pre, acts = contact_states("folded")
    mc, eb = _batch(2, f64, control_mode="pd", self_collision=True, **PD_SCALE)
    set_pre(eb, pre)
    R.attach(eb, np.tile(R.twin_wrench(mc, d), (2, 1, 1)))
    eb.step(acts)
    assert not eb.nwarn.any() and (eb.self_contacts > 0).all()
    tq, tv = (R.GATE_F64, R.GATE_F64) if f64 else (R.TOL_QPOS, R.TOL_QVEL)
    check_twin(f"folded self-collision {'f64' if f64 else 'f32'}", d, eb.qpos, eb.qvel, eb.touch[:, 0], twin_refs("folded", d, True), twin_refs("folded", 0.0, True), tq, tv)


# ---- case 5: off and zero, in the kernel that the contact-force output selects
def _run3(f64, wrench_mode, n=2, **kw):
    mc, eb = _batch(n, f64, **kw)
    eb.cforce = np.full((n, mc.nbody, 3), np.nan, eb.ft)
    eb._chk(eb.L.ss_set_contact_force_output(eb.batch, eb.cforce.ctypes.data_as(C.c_void_p)))
    if wrench_mode == "zero":
        R.attach(eb, np.zeros((n, mc.nbody, 6)))
    elif wrench_mode == "detached":
        R.attach(eb, np.full((n, mc.nbody, 6), 50.0)); R.attach(eb, None)
    elif wrench_mode == "on":
        R.attach(eb, np.full((n, mc.nbody, 6), 5.0))
    rs = np.random.default_rng(8)
    eb.reset()
    rec = []
    for _ in range(3):
        obs, rew, term, trunc = eb.step(rs.uniform(-1, 1, (n, mc.nu)))
        rec += [eb.qpos.copy(), eb.qvel.copy(), obs, rew, term, trunc, eb.cforce.copy()]
    return rec


@BOTH
def test_off_and_zero_are_the_same_bits(f64):
    off = _run3(f64, None)
    for mode in ("zero", "detached"):
        for x, y in zip(off, _run3(f64, mode)):
            assert np.array_equal(x, y), mode
    on = _run3(f64, "on")
    assert not np.array_equal(off[0], on[0])                  # (and a wrench that is attached acts)


# ---- case 6: a bad-state reset inside the launch drops the wrench for that launch
@BOTH
def test_bad_state_reset_drops_the_wrench_for_the_launch(f64):
    mc = model_const()
    big = np.zeros((2, mc.nbody, 6)); big[:, :, :3] = 300.0
    rs = np.random.default_rng(9)
    a1, a2 = rs.uniform(-0.3, 0.3, (2, 2, mc.nu))
    runs = []
    for w in (big, 0 * big):
        _, eb = _batch(2, f64)
        eb.reset()
        eb.qpos[0, 0] = 1e11                                  # mj_checkPos resets env 0 in the first mj_step
        R.attach(eb, w)
        o1 = eb.step(a1)[0]
        s1 = (eb.qpos.copy(), eb.qvel.copy(), o1, eb.nwarn.copy())
        eb.step(a2)
        runs.append((s1, eb.qpos.copy(), None if eb.xfrc is None else eb.xfrc.copy()))
    (s_big, q2_big, x_big), (s_zero, q2_zero, _) = runs
    assert s_big[3][0] >= 1 and s_big[3][1] == 0
    for x, y in zip(s_big, s_zero):
        assert np.array_equal(x[0], y[0])                     # env 0: the bytes of the zero-wrench run
    assert not np.array_equal(s_big[0][1], s_zero[0][1])      # env 1 was pushed
    assert not np.array_equal(q2_big[0], q2_zero[0])          # the next launch applies it to env 0 again
    assert np.array_equal(x_big, big)                         # the kernel never writes the caller's buffer


# ---- case 7: resets do not apply it
@BOTH
def test_resets_do_not_apply_the_wrench(f64):
    """ss_reset under StateInit Fall (45 mj_steps per env), and the fused reset pass of ss_step_autoreset.  The reset pass starts its
    Newton iteration from the step's qacc_warm, so its bits follow the step's; for the byte comparison env 1's step must not depend on
    the wrench either: a bad qpos resets it in the first mj_step, which drops the wrench for the launch (the test above), and its
    episode ends by truncation.  Env 2 is truncated after an ordinary, pushed step: float64 shows that its reset pass differs by the
    warm start's rounding only."""
    mc = model_const()
    rs = np.random.default_rng(10)
    fall, fall2 = rs.uniform(size=(2, 3, 3, mc.nu))
    act = rs.uniform(-0.3, 0.3, (3, mc.nu))
    big = np.zeros((3, mc.nbody, 6)); big[:, :, :3] = 40.0
    runs = []
    for w in (big, 0 * big):
        _, eb = _batch(3, f64, state_init=_cabi.INIT_FALL, episode_length=20)
        R.attach(eb, w)
        obs = eb.reset(fall_actions=fall)
        after_reset = (obs, eb.qpos.copy(), eb.qvel.copy())
        fa = np.ascontiguousarray(fall2, eb.ft)
        eb._chk(eb.L.ss_set_fall_actions(eb.batch, fa.ctypes.data_as(C.c_void_p)))
        eb.cur_t[1:] = 20                                     # the episodes of envs 1 and 2 end in this step: the launch resets them (Fall again)
        eb.qpos[1, 0] = 1e11
        _, obs_next, _, term, trunc = eb.step_autoreset(act)
        assert (term | trunc).tolist() == [False, True, True] and eb.nwarn.tolist() == [0, 1, 0]
        runs.append((after_reset, obs_next, eb.qpos.copy(), eb.qvel.copy()))
    (r_big, o_big, q_big, v_big), (r_zero, o_zero, q_zero, v_zero) = runs
    for x, y in zip(r_big, r_zero):
        assert np.array_equal(x, y)
    assert np.array_equal(o_big[1], o_zero[1]) and np.array_equal(q_big[1], q_zero[1]) and np.array_equal(v_big[1], v_zero[1])   # the fused reset pass
    assert not np.array_equal(q_big[0], q_zero[0])            # while env 0's step was pushed
    if f64:
        assert R.abs_err(q_big[2], q_zero[2]) < 1e-10 and R.abs_err(v_big[2], v_zero[2]) < 1e-10


# ---- case 11: C ABI error paths
def test_error_paths():
    mc, eb = _batch(1, False)
    L = _cabi.bind_wrench(eb.L)
    assert _cabi.WRENCH_EXPORTS == ["ss_set_body_wrench_input"] and L.ss_set_body_wrench_input.argtypes == [C.c_void_p, C.c_void_p]
    assert "ss_set_body_wrench_input" not in _cabi.EXPORTS    # a header of its own: what bind() attaches is what it was
    assert L.ss_set_body_wrench_input(None, None) == -1 and b"null batch" in L.ss_last_error()
    buf = np.zeros((1, mc.nbody, 6), np.float32)
    assert L.ss_set_body_wrench_input(None, buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.ss_set_body_wrench_input(eb.batch, None) == 0    # off while off
