"""Where an env runs is scheduling only: the persistent step launch must give every env the same bytes whichever workgroup,
wavefront and LDS slice steps it, in whichever round of the hand-out, behind whichever other env, under whichever order array.

Every case steps the 37 envs of placement_cases.py under the launch geometries and hand-out orders of placement_cases.geometries
(ss_set_launch_geometry, ss_set_order, ss_schedule_longest_first) and compares everything the launches write, byte for byte, with the
automatic launch — at 37 envs one env per single-wavefront workgroup, which the rest of the suite (and, for two cases, this file) pins
to the float64 oracle.  The geometries reach what the small GPU tests never run: the hand-out counter, a wavefront stepping a second
env in the slice the first one left behind (with NaNs in it, or after a fused reset), several slices in one workgroup, the shared
dense block of body-body-contact batches behind its lock, and the double-buffered counter across launches of different geometry.

test_one_env_cannot_move_another changes one env of a full workgroup and requires every other env to keep its bytes.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parity_tools as P  # noqa: E402
import placement_cases as PC  # noqa: E402
from smplsim_amd._lib import lib  # noqa: E402

N = PC.N
CASES = ("smpl", "generic_chain15", "getup", "smplx", "selfcol_crowded", "imitation_fused", "smplx_selfcol_crowded")
CROWDED = {"selfcol_crowded": "smpl_humanoid", "smplx_selfcol_crowded": "smplx_humanoid"}


class Rig:
    """One batch and the state it was built with: restore() puts every tensor of the env (state, outputs, draws) and its generators
    back in place, so that every geometry starts from the same bytes on the SAME batch (its work counters keep alternating)."""

    def __init__(self, env):
        self.env, self.base = env, getattr(env, "base", env)
        self.objs = [env] if self.base is env else [env, self.base]
        torch.cuda.synchronize()
        self.saved = [(o, n, t.clone()) for o in self.objs for n, t in vars(o).items() if torch.is_tensor(t)]
        self.gens = [(o.gen, o.gen.get_state()) for o in self.objs]
        self.max_epw = self.base.launch_info()["envs_per_workgroup"]
        self.keep = []                                           # order arrays: alive until the batch is closed
        self.geom = None

    def restore(self):
        torch.cuda.synchronize()
        for o, n, t in self.saved:
            getattr(o, n).copy_(t)
        for g, s in self.gens:
            g.set_state(s)
        if self.base is not self.env:                            # the imitation env's block of resampling draws: drawn again
            self.env._rand_block, self.env._rand_i = None, self.env.RAND_BLOCK

    def set_geometry(self, geom):
        name, epw, max_wgs, kind, order = geom
        self.geom = geom
        assert lib().ss_set_launch_geometry(self.base.handle, epw, max_wgs) == 0
        ptr = None
        if isinstance(order, np.ndarray):
            t = torch.tensor(order, dtype=torch.int32, device=self.base.device)
            self.keep.append(t)
            ptr = C.c_void_p(t.data_ptr())
        assert lib().ss_set_order(self.base.handle, ptr) == 0

    def step(self, actions):
        """One control step under the current geometry; the longest-first order is computed before the launch and dropped after it,
        as the env classes do above 64 envs."""
        device_order = isinstance(self.geom[4], str)
        if device_order:
            assert lib().ss_schedule_longest_first(self.base.handle, self.base._stream()) == 0
        self.env.step(actions)
        if device_order:
            assert lib().ss_set_order(self.base.handle, None) == 0
        torch.cuda.synchronize()
        return PC.snapshot(self.env)

    def where(self):
        _, epw, max_wgs, _, order = self.geom
        return PC.placement(epw, max_wgs, order)

    def close(self):
        torch.cuda.synchronize()
        lib().ss_set_order(self.base.handle, None)
        self.env.close()


def _acts(a, device):
    return torch.tensor(a, dtype=torch.float32, device=device)


def _chain15():
    from smplsim_amd.batch import ShardModel
    from smplsim_amd.mjcf import compile_mjcf
    from smplsim_amd.mjcf_writer import table_to_mjcf
    from test_synthetic_trees_emu import _chain
    xml = table_to_mjcf(_chain(14))
    mc = compile_mjcf(xml)
    tables = (np.full(mc.nu, 60.0), np.full(mc.nu, 6.0), np.full(mc.nu, 40.0), np.full(mc.nu, 2.0), np.zeros(mc.nu))
    rs = np.random.default_rng(15)
    q = np.zeros((N, mc.nq)); q[:, 2] = np.where(np.arange(N) % 4 == 3, 2.6, 2.8); q[:, 3] = 1.0   # every fourth chain starts in the floor
    q[:, 7:] = rs.uniform(-0.3, 0.3, (N, mc.nq - 7))
    s = dict(qpos=q, qvel=rs.normal(size=(N, mc.nv)) * 0.3, acts=rs.uniform(-0.3, 0.3, (PC.STEPS, N, mc.nu)))
    s["acts"][0, PC.NAN_ROW, 2] = np.nan
    return ShardModel(xml=xml, contact_bodies=tuple(mc.body_names), tables=tables), s


def build(case):
    """(Rig, inputs) of a case."""
    from smplsim_amd.batch import SMPLSimVecEnv
    if case == "smpl":                                           # the headline instantiation: fixed layout, flavour 0
        return Rig(SMPLSimVecEnv(N, task="HumanoidSpeed", episode_length=2, autoreset=True, seed=11)), PC.humanoid_states("smpl_humanoid")
    if case == "generic_chain15":                                # the runtime-layout instantiation (any model that is not a packaged fixture)
        model, s = _chain15()
        return Rig(SMPLSimVecEnv(N, model=model, task="HumanoidSpeed", episode_length=1, autoreset=True, seed=12, reach_body=0)), s
    if case == "getup":
        return Rig(SMPLSimVecEnv(N, task="HumanoidGetup", state_init="Fall", episode_length=1, recovery_steps=1, autoreset=True, seed=13)), PC.humanoid_states("smpl_humanoid")
    if case == "smplx":                                          # the two-pass kernel on the aliased layout, 7 envs per workgroup at most
        return Rig(SMPLSimVecEnv(N, humanoid="smplx_humanoid", autoreset=True, seed=14)), PC.humanoid_states("smplx_humanoid")
    if case == "selfcol_crowded":
        return Rig(SMPLSimVecEnv(N, self_collision=True, autoreset=False, state_init="External", seed=15)), PC.crowded_case_states()
    if case == "smplx_selfcol_crowded":                          # 52 bodies: a shared block of 14084 reals, two envs per workgroup
        return (Rig(SMPLSimVecEnv(N, humanoid="smplx_humanoid", self_collision=True, autoreset=False, state_init="External", seed=16)),
                PC.crowded_case_states(humanoid="smplx_humanoid"))
    assert case == "imitation_fused"
    import test_motion_lib as T
    from smplsim_amd.imitation import SMPLSimImitationVecEnv
    env = SMPLSimImitationVecEnv(N, T.make_lib(None, device=0), seed=3)
    assert env.fused
    env.offset[:, 2] = 0.05
    return Rig(env), None


def run(case, rig, geom, s, edit=None):
    """The case's launches under one geometry from the restored batch: the list of snapshots, one per launch that is compared.
    edit(state dict): the isolation test's change of one env."""
    rig.restore()
    rig.set_geometry(geom)
    env, dev = rig.env, rig.base.device
    if s is not None and edit is not None:
        s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
        edit(s)
    snaps = []
    if case in ("smpl", "generic_chain15", "smplx"):
        env.reset()                                              # Default reset: task state, cur_t
        env.set_state(s["qpos"], s["qvel"], warm=np.zeros_like(s["qvel"]))
        for t in range(3 if case == "smpl" else 2):
            snaps.append(rig.step(_acts(s["acts"][t], dev)))
    elif case == "getup":
        env.reset()                                              # the Fall reset launch: 45 mj_steps per env, MODE_RESET
        torch.cuda.synchronize()
        snaps.append(PC.snapshot(env))
        for t in range(2):                                       # episode_length 1: every env is reset from _fall_buf inside each launch
            snaps.append(rig.step(_acts(s["acts"][t], dev)))
        env.reset(torch.arange(N, device=dev) % 3 == 0)
        torch.cuda.synchronize()
        snaps.append(PC.snapshot(env))
    elif case in CROWDED:
        env.set_state(s["qpos"], s["qvel"], warm=np.zeros_like(s["qvel"]))
        snaps.append(rig.step(_acts(s["acts"][0], dev)))
        if geom[0] in ("R", "b", "c"):
            snaps.append(rig.step(_acts(s["acts"][1], dev)))
    else:
        env.reset()
        ids = env.motion_ids.clone()
        late = torch.arange(N, device=dev) % 3 == 1              # 12 envs start 2.5 control steps before the end of their clip
        t0 = torch.where(late, (env.motion_lib.get_motion_length(ids) - 2.5 * env.dt).clamp_(min=0.0), env.start_times)
        env.reset(motion_ids=ids, start_times=t0)
        torch.cuda.synchronize()
        snaps.append(PC.snapshot(env))
        for t in range(4):
            snaps.append(rig.step(env.reference_actions()))
    return snaps


def _report(ref, got, rig, skip_rows=()):
    lines = []
    for i, (a, b) in enumerate(zip(ref, got)):
        lines += ["launch %d: %s" % (i, m) for m in PC.compare(a, b, rig.where(), skip_rows)]
    return lines


def _f32(snap, field):
    return snap[field].view(np.float32).astype(np.float64)


def _i32(snap, field):
    return snap[field].view(np.int32)


def _pin_to_oracle(case, s, first):
    """The reference launch itself: its first control step against the float64 oracle at the per-control-step tolerance, over the envs
    without a bad-state reset (test_sweep_padding_gpu.py holds the same kind of state to the same tolerance)."""
    humanoid = "smpl_humanoid" if case == "smpl" else "smplx_humanoid"
    q, v = s["qpos"].astype(np.float32).astype(np.float64), s["qvel"].astype(np.float32).astype(np.float64)
    pre = dict(qpos=q, qvel=v, qpos_prev=q, qvel_prev=v, qacc_warm=np.zeros_like(v))
    a = s["acts"][0].astype(np.float32).astype(np.float64)
    if case == "smpl":
        # the fused reset replaced the state of the envs the first step terminated (the dropped ones fall over): the same kernel
        # instantiation without autoreset, under the same automatic launch, keeps every env's post-step state — and is the case's
        # own first launch bit for bit wherever that one did not reset
        from smplsim_amd.batch import SMPLSimVecEnv
        plain = SMPLSimVecEnv(N, task="HumanoidSpeed", episode_length=2, autoreset=False, seed=11)
        plain.reset()
        plain.set_state(s["qpos"], s["qvel"], warm=np.zeros_like(s["qvel"]))
        plain.step(_acts(s["acts"][0], plain.device))
        torch.cuda.synchronize()
        kept, reset_rows = PC.snapshot(plain), np.flatnonzero(first["terminated"][:, 0])
        plain.close()
        assert len(reset_rows) >= 8 and np.array_equal(kept["terminated"], first["terminated"])
        for f in ("qpos", "qvel", "qacc_warm", "touch", "solver_iters", "nwarn", "rew_buf"):
            assert np.array_equal(np.delete(kept[f], reset_rows, 0), np.delete(first[f], reset_rows, 0)), f
        assert np.array_equal(kept["obs_buf"], first["obs_final"])
        first = kept
    ok = _i32(first, "nwarn")[:, 0] == 0
    rows = np.flatnonzero(ok)
    orc = P.oracle_step({k: x[rows] for k, x in pre.items()}, a[rows], humanoid)
    err = P.rel_err(dict(qpos=_f32(first, "qpos")[rows], qvel=_f32(first, "qvel")[rows]), orc)
    print(case, "reference launch vs oracle: rows", rows.tolist(), "rel. error (qpos, qvel) max", err.max(axis=0).tolist(), "worst row", int(rows[err[:, 1].argmax()]))
    assert sorted(set(range(N)) - set(rows.tolist())) == sorted([s["nan_row"], s["diverging_row"]])
    assert (orc["nwarn"] == 0).all()
    assert P.within_tol(err, P.TOL_STEP).all(), (case, rows[~P.within_tol(err, P.TOL_STEP)].tolist(), err)


@pytest.mark.parametrize("case", CASES)
def test_results_do_not_depend_on_launch_geometry_or_hand_out(case):
    rig, s = build(case)
    try:
        geoms = PC.geometries(rig.max_epw, leading=8 if case in CROWDED else 0)
        assert rig.max_epw == {"smpl": 12, "getup": 12, "imitation_fused": 12, "smplx": 7, "selfcol_crowded": 8, "smplx_selfcol_crowded": 2}.get(case, rig.max_epw)
        if case in CROWDED:                                      # the crowded rows hold the contacts the host count saw
            rig.restore(); rig.set_geometry(geoms[0])
            rig.env.set_state(s["qpos"], s["qvel"], warm=np.zeros_like(s["qvel"]))
            rig.env.debug_forward()
            torch.cuda.synchronize()
            assert rig.env.self_contacts[:8].cpu().tolist() == s["nself"].tolist()
        ref = run(case, rig, geoms[0], s)
        again = run(case, rig, geoms[0], s)
        lines = _report(ref, again, rig)
        assert not lines, "the reference geometry is not deterministic from run to run:\n" + "\n".join(lines)
        # the case runs what it is for
        if case in ("smpl", "generic_chain15"):
            trunc = [snap["truncated"][:, 0].astype(bool) for snap in ref]
            print(case, "truncated per step", [int(t.sum()) for t in trunc], "terminated per step", [int(snap["terminated"].sum()) for snap in ref])
            # every env runs the fused reset (the second trip of the kernel's rep loop) in a reused slice: inside the last step launch by
            # truncation, unless the step of an earlier launch terminated it (the dropped envs fall over, the two bad-state envs)
            early = np.any([snap["terminated"][:, 0].astype(bool) for snap in ref[:-1]], axis=0)
            assert not any(t.any() for t in trunc[:-1]) and np.array_equal(trunc[-1], ~early) and trunc[-1].sum() >= 24
            assert (_i32(ref[-1], "cur_t")[~early] == 0).all()
        if case == "smpl":
            touching = (_i32(ref[0], "touch") != 0).any(axis=1)
            assert touching.any() and not touching.all()
        if case in ("smpl", "smplx"):
            _pin_to_oracle(case, s, ref[0])
        if case == "getup":
            print(case, "truncated per launch", [int(snap["truncated"].sum()) for snap in ref], "terminated", [int(snap["terminated"].sum()) for snap in ref])
            assert ref[2]["truncated"][:, 0].all() and (_i32(ref[2], "cur_t") == 0).all()   # episode_length 1: the second step resets every env from _fall_buf
        if case in CROWDED:
            nself = _i32(ref[0], "self_contacts")[:, 0]
            print(case, "body-body contacts after the first control step", nself.tolist(), "Newton iterations", _i32(ref[0], "solver_iters")[:, 0].tolist())
            q, v = s["qpos"].astype(np.float32).astype(np.float64), s["qvel"].astype(np.float32).astype(np.float64)
            rows = np.arange(8)
            orc = P.oracle_step(dict(qpos=q[rows], qvel=v[rows], qpos_prev=q[rows], qvel_prev=v[rows], qacc_warm=np.zeros_like(v[rows])),
                                s["acts"][0].astype(np.float32).astype(np.float64)[rows], CROWDED[case], self_collision=True)
            err = P.rel_err(dict(qpos=_f32(ref[0], "qpos")[rows], qvel=_f32(ref[0], "qvel")[rows]), orc)
            print(case, "crowded rows vs oracle (not asserted): rel. error (qpos, qvel) per row", err.tolist(), "oracle nwarn", orc["nwarn"].tolist(),
                  "device nwarn", _i32(ref[0], "nwarn")[rows, 0].tolist())
        if case == "imitation_fused":
            cur = np.stack([_i32(snap, "cur_t")[:, 0] for snap in ref])
            assert ((cur[1:] == 0).any(axis=0)).sum() >= 10      # re-initialised inside a step launch: the clip time restarted
            assert (cur[-1] > 0).any()
        failures = []
        for geom in geoms[1:]:
            got = run(case, rig, geom, s)
            assert len(got) == (len(ref) if case not in CROWDED or geom[0] in ("b", "c") else 1)   # (crowded: the second step under R, b, c only)
            lines = _report(ref, got, rig)
            if lines:
                failures.append("geometry %s (envs_per_wg %d, max_workgroups %d, order %s):\n  " % geom[:4] + "\n  ".join(lines))
        assert not failures, "results depend on where the envs ran:\n" + "\n".join(failures)
    finally:
        rig.close()


ISOLATION = [("smpl", 5, "nan_action"), ("smpl", 20, "diverging_state"),
             ("selfcol_crowded", 3, "nan_action"), ("selfcol_crowded", 5, "diverging_state"), ("selfcol_crowded", 20, "crowded_state"),
             ("smplx_selfcol_crowded", 20, "crowded_state")]


@pytest.mark.parametrize("case,j,change", ISOLATION)
def test_one_env_cannot_move_another(case, j, change):
    """One full workgroup (geometry b): env j's action becomes NaNs, or its state a diverging or a crowded one.  j is a row of the
    first round (5; 3 in the crowded case, between crowded neighbours) or one handed out later (20).  Every other env keeps its
    bytes — no slice overruns into its neighbour, nothing is read from the shared block outside the lock, and nothing env j left in
    its slice reaches the env that wavefront steps next — and env j itself does change."""
    rig, s = build(case)
    try:
        geom = PC.geometries(rig.max_epw, leading=8 if case in CROWDED else 0)[2]
        assert geom[0] == "b" and (j in PC.placement(geom[1], geom[2], geom[4])) == (j < rig.max_epw)

        def edit(st):
            if change == "nan_action":
                st["acts"][:, j] = np.nan
            elif change == "diverging_state":
                st["qvel"][j] = st["qvel"][PC.DIVERGING_ROW]
            else:
                st["qpos"][j] = PC.crowded_states(humanoid=CROWDED[case])["qpos"][0]; st["qvel"][j] = 0.0
        assert j not in (PC.NAN_ROW, PC.DIVERGING_ROW)
        one = run(case, rig, geom, s)[:1]
        two = run(case, rig, geom, s, edit)[:1]
        lines = _report(one, two, rig, skip_rows=(j,))
        assert not lines, "env %d (%s) moved other envs:\n" % (j, change) + "\n".join(lines)
        assert PC.differing_rows(one[0], two[0]) == [j]
    finally:
        rig.close()


def test_launch_geometry_contract_on_the_device():
    """ss_set_launch_geometry refuses what the batch cannot launch, says why, and leaves the geometry it had in force."""
    rig, s = build("smpl")
    try:
        h, L = rig.base.handle, lib()
        geoms = PC.geometries(rig.max_epw)
        ref = run("smpl", rig, geoms[0], s)
        rig.restore(); rig.set_geometry(geoms[4])                 # d: 2 envs per workgroup, 3 workgroups
        for bad in ((rig.max_epw + 1, 0), (-1, 0), (1, -1), (-3, -3)):
            assert L.ss_set_launch_geometry(h, *bad) == -1
            msg = L.ss_batch_last_error(h).decode()
            assert "[0, ss_launch_info's value]" in msg and "max_workgroups >= 0" in msg
        assert L.ss_set_launch_geometry(None, 1, 1) == -1
        # the refused calls changed nothing: the launches still run (as geometry d) and still equal the reference
        env, dev = rig.env, rig.base.device
        env.reset()
        env.set_state(s["qpos"], s["qvel"], warm=np.zeros_like(s["qvel"]))
        got = [rig.step(_acts(s["acts"][t], dev)) for t in range(3)]
        assert not _report(ref, got, rig)
        assert L.ss_set_launch_geometry(h, rig.max_epw, 0) == 0 and L.ss_set_launch_geometry(h, 0, 0) == 0
    finally:
        rig.close()
