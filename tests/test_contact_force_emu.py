"""Per-body contact forces (ss_set_contact_force_output) on the wavefront emulator, float64 and float32 builds, against the float64
oracle's mjData.efc_force of the control step's last mj_step (contact_force_ref.py: reference, error measure, gates; the measured
samples behind the gates: profiles/contact_force.txt).  GPU twin: test_contact_force_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import contact_force_ref as R
from helpers import FEET, model_const, oracle_model, pd_tables
from smplsim_amd import _cabi
from wave_emu import emu

BOTH = pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])


def _gate(f64):
    return R.GATE_F64 if f64 else R.GATE_F32_EMU


def _batch(n, f64, humanoid="smpl_humanoid", **kw):
    mc = model_const(humanoid)
    eb = emu.EmuBatch(mc, pd_tables(mc), n, legal_bodies=FEET, f64=f64, **kw)
    eb.cforce = np.full((n, mc.nbody, 3), np.nan, eb.ft)        # NaN: a body the kernel does not write shows
    eb._chk(eb.L.ss_set_contact_force_output(eb.batch, eb.cforce.ctypes.data_as(C.c_void_p)))
    return mc, eb


def _compare(case, eb, mc, om, pre, acts, f64, touch_zero=True):
    """The compared step was taken: every env's forces against the oracle from its pre-step state.  Returns the oracle's infos."""
    W, infos = R.weight(mc), []
    assert np.isfinite(eb.cforce).all()                        # every body of every env was written
    for i in range(eb.N):
        Fr, info = R.oracle_contact_force(om, mc.friction, pre[i], acts[i])
        err = R.force_error(eb.cforce[i], Fr, W)
        print(f"contact-force sample: {case} {'f64' if f64 else 'f32'} env {i} err {err:.3e} loaded {len(info['loaded'])} iters {eb.solver_iters[i]}")
        assert err < _gate(f64), (case, i, err)
        if touch_zero:                                         # bodies that do not touch the floor: exact zeros (floor-only batches)
            touch = int(eb.touch[i, 0]) & 0xFFFFFFFF | (int(eb.touch[i, 1]) & 0xFFFFFFFF) << 32
            for b in range(mc.nbody):
                if not (touch >> b) & 1:
                    assert not eb.cforce[i, b].any(), (case, i, b)
            assert (eb.cforce[i, :, 2] >= 0).all(), (case, i)  # a floor can only push
        infos.append(info)
    return infos


def standing(f64):
    mc, eb = _batch(3, f64)
    rs = np.random.default_rng(21)
    eb.reset()
    for _ in range(5):
        acts = rs.uniform(-0.4, 0.4, (3, mc.nu))
        pre = [R.pre_of(eb, i) for i in range(3)]
        eb.step(acts)
    return mc, eb, pre, acts


@BOTH
def test_standing(f64):
    mc, eb, pre, acts = standing(f64)
    infos = _compare("standing", eb, mc, oracle_model(), pre, acts, f64)
    assert sum(len(i["loaded"]) for i in infos) >= 1


LYING_SEED, LYING_SETTLE = 3, 17       # picked on the CPU: every one of the three envs ends with >= 6 loaded bodies, boxes and capsules


def lying_inputs(seed=LYING_SEED):
    """(fall_actions [3, 3, nu], action of the compared step [3, nu]): the GPU test uses the three envs, this file the first two."""
    rs = np.random.default_rng(seed)
    return rs.uniform(size=(3, 3, 69)), rs.uniform(-0.02, 0.02, (3, 69))


def lying(f64, seed=LYING_SEED, settle=LYING_SETTLE, n=2):
    """StateInit.Fall, then zero actions until the humanoid lies still (the contact set stops changing after ~15 control steps),
    then the compared step under a small action."""
    mc, eb = _batch(n, f64, state_init=_cabi.INIT_FALL)
    fall, acts = lying_inputs(seed)
    eb.reset(fall_actions=fall[:n])
    for _ in range(settle):
        eb.step(np.zeros((n, mc.nu)))
    pre = [R.pre_of(eb, i) for i in range(n)]
    eb.step(acts[:n])
    return mc, eb, pre, acts[:n]


@BOTH
def test_lying_many_contacts(f64):
    mc, eb, pre, acts = lying(f64)
    infos = _compare("lying", eb, mc, oracle_model(), pre, acts, f64)
    from smplsim_amd import mjcf
    for info in infos:                                         # the oracle alone: many loaded bodies, a box and a capsule among them, in each env
        kinds = {int(mc.geom_type[b]) for b in info["loaded"]}
        assert len(info["loaded"]) >= 6 and {mjcf.GEOM_BOX, mjcf.GEOM_CAPSULE} <= kinds, (info["loaded"], kinds)


SELF_SEED = 2


def self_states(n, seed=SELF_SEED, humanoid="smpl_humanoid"):
    """Folded poses just above the floor (as test_selfcol_emu.py's), kept when the oracle's control step from them ends with a
    loaded body-body contact and a loaded floor contact."""
    from helpers import default_qpos
    mc, om = model_const(humanoid), oracle_model(humanoid, self_collision=True)
    rs = np.random.default_rng(seed)
    pres, acts = [], []
    while len(pres) < n:
        q = default_qpos(mc.nq); q[2] = 0.35; q[7:] = rs.uniform(-1.5, 1.5, mc.nq - 7)
        v, a = rs.normal(size=mc.nv) * 0.5, rs.uniform(-1, 1, mc.nu)
        pre = dict(qpos=q, qvel=v, qpos_prev=q, qvel_prev=v, qacc_warm=np.zeros(mc.nv))
        F, info = R.oracle_contact_force(om, mc.friction, pre, a)
        if info["n_self_loaded"] >= 1 and np.abs(info["floor_sum"]).max() > 0 and info["nwarn"] == 0:
            pres.append(pre); acts.append(a)
    return mc, om, pres, np.array(acts)


def body_body(f64):
    mc, om, pres, acts = self_states(2)
    _, eb = _batch(2, f64, self_collision=True)
    eb.set_state(np.array([p["qpos"] for p in pres]), np.array([p["qvel"] for p in pres]))
    eb.step(acts)
    return mc, om, eb, pres, acts


@BOTH
def test_body_body_contacts(f64):
    mc, om, eb, pres, acts = body_body(f64)
    infos = _compare("body-body", eb, mc, om, pres, acts, f64, touch_zero=False)
    W = R.weight(mc)
    for i, info in enumerate(infos):
        assert info["n_self_loaded"] >= 1
        # action = reaction: the body-body forces cancel in the sum over bodies, what is left is the floor's
        tot = eb.cforce[i].astype(np.float64).sum(axis=0)
        assert np.abs(tot - info["floor_sum"]).max() < mc.nbody * _gate(f64) * max(W, np.abs(info["floor_sum"]).max()), (i, tot, info["floor_sum"])


def smplx(f64):
    """52 bodies, 136 contact slots: a humanoid that lies still on the floor, fingers included (slots of the second pass)."""
    mc, eb = _batch(1, f64, humanoid="smplx_humanoid", state_init=_cabi.INIT_FALL)
    rs = np.random.default_rng(1)
    eb.reset(fall_actions=rs.uniform(size=(1, 3, mc.nu)))
    for _ in range(LYING_SETTLE):
        eb.step(np.zeros((1, mc.nu)))
    acts = rs.uniform(-0.02, 0.02, (1, mc.nu))
    pre = [R.pre_of(eb, 0)]
    eb.step(acts)
    return mc, eb, pre, acts


@BOTH
def test_smplx(f64):
    from smplsim_amd import mjcf
    mc, eb, pre, acts = smplx(f64)
    infos = _compare("smplx", eb, mc, oracle_model("smplx_humanoid"), pre, acts, f64)
    # first contact slot of every body: a box owns 4 slots, then 2 per capsule / sphere in body order (make_constraints)
    box = mc.geom_type == mjcf.GEOM_BOX
    slot = np.where(box, 4 * (np.cumsum(box) - 1), 4 * box.sum() + 2 * (np.cumsum(~box) - 1))
    loaded = slot[infos[0]["loaded"]]
    assert (loaded < 64).any() and (loaded >= 64).any(), loaded  # both passes over the slots carry load


@BOTH
def test_switching_off_and_same_bits(f64):
    runs = []
    for on in (True, True, False):
        mc, eb = _batch(3, f64, self_collision=True)
        if not on:
            eb._chk(eb.L.ss_set_contact_force_output(eb.batch, None))
        rs = np.random.default_rng(8)
        eb.reset()
        rec = []
        for _ in range(4):
            obs, rew, _, _ = eb.step(rs.uniform(-1, 1, (3, mc.nu)))
            rec += [eb.qpos.copy(), eb.qvel.copy(), obs, rew]
        runs.append((rec, eb.cforce.copy(), eb))
    (r0, f0, eb0), (r1, f1, _), (r2, f2, _) = runs
    assert np.isfinite(f0).all() and np.abs(f0).max() > 1.0
    assert f0.tobytes() == f1.tobytes()                         # two runs: the same bits
    assert np.isnan(f2).all()                                  # off from the start: never written
    for x, y in zip(r0, r2):                                   # the state does not depend on the output
        assert x.tobytes() == y.tobytes()
    eb0._chk(eb0.L.ss_set_contact_force_output(eb0.batch, None))   # off again: the buffer keeps its contents
    eb0.step(np.zeros((3, 69)))
    assert eb0.cforce.tobytes() == f0.tobytes()


def test_error_paths():
    mc, eb = _batch(2, False)
    L = eb.L
    buf = np.zeros((2, mc.nbody, 3), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    eb.reset(); eb.step(np.zeros((2, mc.nu)))
    assert L.ss_get_state(eb.batch, _cabi.FIELDS["contact_force"], p, None) == 0 and buf.tobytes() == eb.cforce.tobytes()
    assert L.ss_set_state(eb.batch, _cabi.FIELDS["contact_force"], p, None) == -1 and b"read-only" in L.ss_batch_last_error(eb.batch)
    eb._chk(L.ss_set_contact_force_output(eb.batch, None))
    assert L.ss_get_state(eb.batch, _cabi.FIELDS["contact_force"], p, None) == -1
    assert b"ss_set_contact_force_output" in L.ss_batch_last_error(eb.batch)
    assert L.ss_set_contact_force_output(None, None) == -1


@BOTH
def test_autoreset_keeps_the_forces_of_the_step_that_ended_the_episode(f64):
    """Fused autoreset: env 1's episode ends in the compared step (truncation) and the launch resets it; its row holds the forces
    of that step, not of the reset state — resets write nothing."""
    mc, eb = _batch(3, f64, episode_length=20)
    rs = np.random.default_rng(4)
    eb.reset()
    for _ in range(5):
        eb.step(rs.uniform(-0.4, 0.4, (3, mc.nu)))
    eb.cur_t[1] = 20
    acts = rs.uniform(-0.4, 0.4, (3, mc.nu))
    pre = [R.pre_of(eb, i) for i in range(3)]
    _, _, _, term, trunc = eb.step_autoreset(acts)
    assert (term | trunc).tolist() == [False, True, False] and eb.cur_t[1] == 0 and abs(eb.qpos[1, 2] - 0.94) < 1e-6
    infos = _compare("autoreset", eb, mc, oracle_model(), pre, acts, f64, touch_zero=False)   # (touch is the reset state's for env 1)
    assert len(infos[1]["loaded"]) >= 1
    keep = eb.cforce.copy()
    eb.reset(mask=[1, 1, 1])                                   # a reset launch leaves the buffer alone
    assert eb.cforce.tobytes() == keep.tobytes()
