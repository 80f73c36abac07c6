"""Gym-style single-env surface of the reference, backed by the batched HIP stepper.

Keeps the call surface of reference smpl_sim/envs/base_env.py:64-110 and
smpl_sim/envs/humanoid_env.py:148-184,509-512 (constructor from a cfg object, `reset(seed, options)
-> (obs, info)`, `step(action) -> (obs, reward, terminated, truncated, info)` with
`info['critic_state']`, `observation_space`, `action_space`, `actuator_names`, `np_random`,
`seed()`, `close()`, `render()`), so `Agent.sample_worker` (reference agents/agent.py:64-109) and
`examples/benchmark.py:87-116` run unchanged.  Physics, controller, observation and reward run
in one HIP launch on a 1-env batch (`SMPLSimVecEnv`); `SMPLSimGymVecEnv` exposes the same batch
with numpy in/out for `gym.vector`-style callers (`num_envs`, `step(actions=...)`).

Not provided (outside the hot path): viewers / rendering, SMPL_Robot shape
generation (needs the licensed SMPL files) — the packaged mean-body model is used, exactly the
reference's own fallback (humanoid_env.py:249-254).
"""
import os
import types

import numpy as np

from ..batch import SMPLSimVecEnv, ShardModel
from ..mjcf_writer import default_xml_str
from ..spaces import Box


def _opt(node, key, default):
    """cfg key with a default.  pdp_scale / pdd_scale: the reference reads them unconditionally (humanoid_env.py:315), but the YAML text
    of its own examples/benchmark.py:27-66 does not have them — missing means 1 here, so that harness runs."""
    if hasattr(node, "get"):
        v = node.get(key, default)
        return default if v is None else v
    return getattr(node, key, default)


class _MjDataView:
    """The few mjData fields callers of the reference env read (examples/env_humanoid_test.py:44)."""

    def __init__(self, env):
        self._e = env

    @property
    def qpos(self):
        return self._e._vec.qpos[0].cpu().numpy().astype(np.float64)

    @property
    def qvel(self):
        return self._e._vec.qvel[0].cpu().numpy().astype(np.float64)

    @property
    def ctrl(self):
        return np.zeros(self._e._vec.nu)

    @property
    def xfrc_applied(self):
        """mjData.xfrc_applied of env 0: a writable [nbody, 6] view (force at the centre of mass ; torque, world frame) of the batch's
        wrench tensor, rows in the order of body_names_orig (no world body: MuJoCo's body id - 1).  Reading or writing it turns the
        input on (SMPLSimVecEnv.enable_body_wrenches); the next step applies what it holds."""
        return _XfrcView(self._e._vec.enable_body_wrenches()[0])

    @xfrc_applied.setter
    def xfrc_applied(self, value):
        self.xfrc_applied[...] = value


class _XfrcView:
    """numpy-style indexing onto one env's [nbody, 6] rows of the device tensor: reads copy to the host, writes go to the device."""

    def __init__(self, rows):
        self._t = rows
        self.shape, self.dtype = tuple(rows.shape), np.float64

    def __array__(self, dtype=None, copy=None):
        return self._t.cpu().numpy().astype(dtype or np.float64)

    def __getitem__(self, idx):
        return np.asarray(self)[idx]

    def __setitem__(self, idx, value):
        import torch
        a = np.asarray(self)
        a[idx] = value                                       # numpy's indexing and broadcasting rules
        self._t.copy_(torch.as_tensor(a, dtype=torch.float32))

    def __repr__(self):
        return repr(np.asarray(self))


class HumanoidEnv:
    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 30}
    _TASK = "HumanoidEnv"

    def __init__(self, cfg, device=0, num_envs=1, bodies=None):
        """bodies (cfg.robot.has_shape_variation): one posed body per env — a dict with `verts` [S, V, 3], `joints` [S, J, 3],
        `skin_weights` [V, J], `joint_names`, `parents` (and optionally `joint_range`), i.e. what the reference's SMPL parser
        hands to SMPL_Robot for a betas draw (smpl_local_robot.py:1345-1368); S = 1 or num_envs.  The SMPL model files that turn
        betas into these arrays are licensed and stay with the caller; the geometry rules that follow them are in ..robot."""
        self.cfg = cfg
        e, r = cfg.env, cfg.robot
        self.clip_actions = e.clip_actions
        self.render_mode = e.get("render_mode", None) if hasattr(e, "get") else getattr(e, "render_mode", None)
        self.headless = getattr(cfg, "headless", True)
        self.sim_timestep_inv = e.sim_timestep_inv
        self.sim_timestep = 1.0 / self.sim_timestep_inv
        self.control_freq_inv = e.control_frequency_inv
        self.dt = self.sim_timestep * self.control_freq_inv
        self.control_mode = e.control_mode
        self.power_scale = e.power_scale
        self.max_episode_length = e.episode_length
        self._root_height_obs = e.root_height_obs
        self.self_obs_v = e.self_obs_v
        self.dtype = np.float32
        self.humanoid_type = r.humanoid_type
        if self.humanoid_type not in ("smpl", "smplh", "smplx"):
            raise NotImplementedError(f"humanoid_type: {self.humanoid_type}")
        if self.control_mode not in ("uhc_pd", "pd", "torque", "simple_pid", "default"):   # reference _AVAILABLE_CONTROLLERS
            raise NotImplementedError(f"control_mode {self.control_mode!r} is not supported by the HIP stepper")
        if self.self_obs_v == 2 and not r.create_vel_sensors:
            raise AssertionError("self_obs_v=2 needs robot.create_vel_sensors (reference humanoid_env.py:297)")
        self.has_shape_variation = bool(r.has_shape_variation)
        if self.has_shape_variation and bodies is None:
            raise ValueError("robot.has_shape_variation: pass bodies=dict(verts, joints, skin_weights, joint_names, parents) — the posed "
                             "SMPL mesh of every env's betas draw; this package holds the reference's geometry rules (smplsim_amd.robot), "
                             "not the licensed SMPL model files that produce the mesh")
        smpl_dir = r.get("smpl_data_dir", "data/smpl") if hasattr(r, "get") else "data/smpl"
        if os.path.exists(smpl_dir) and bodies is None:
            print("SMPL files found, but the SMPL parser is not part of this package; using the mean neutral body (pass bodies=...)")
        self.default_xml_str = default_xml_str("smpl_humanoid" if self.humanoid_type == "smpl" else "smplx_humanoid")
        shape_mcs = None
        if bodies is not None:
            from .. import robot as _robot
            from ..mjcf_writer import table_to_mjcf
            g = (lambda k, d=None: r.get(k, d)) if hasattr(r, "get") else (lambda k, d=None: getattr(r, k, d))
            flags = dict(smpl_model=self.humanoid_type, upright_start=bool(g("has_upright_start", False)), remove_toe=bool(g("remove_toe", False)),
                         big_ankle=bool(g("big_ankle", True)), box_body=bool(g("box_body", True)), freeze_hand=bool(g("freeze_hand", False)),
                         real_weight=bool(g("real_weight", True)), real_weight_porpotion_capsules=bool(g("real_weight_porpotion_capsules", True)),
                         real_weight_porpotion_boxes=bool(g("real_weight_porpotion_boxes", True)), create_vel_sensors=bool(r.create_vel_sensors))
            shape_mcs = _robot.models_from_mesh(bodies["verts"], bodies["joints"], bodies["skin_weights"], bodies["joint_names"],
                                                bodies["parents"], joint_range=bodies.get("joint_range"), **flags)
            if len(shape_mcs) not in (1, num_envs):
                raise ValueError("bodies must hold one shape, or one per env")
        self.contact_bodies = list(e.contact_bodies)
        # body-body contacts: on like in the reference's MuJoCo model (smpl_humanoid.xml:5,24,231-242) unless the cfg says otherwise
        # (`env.self_collision: False` = floor contacts and joint limits only, the faster path; not a key of the reference's yaml)
        self.self_collision = bool(e.get("self_collision", True) if hasattr(e, "get") else getattr(e, "self_collision", True))
        kw = self._task_kwargs(e)
        # Nothing touches the GPU here: the model's device tables and the batch are created on first use, in the process that uses
        # them — the reference's sampler builds the env once and forks its worker processes (agents/agent.py:121-145), and a forked
        # child cannot use its parent's HIP context.  (No GPU at that point = RuntimeError there: there is no CPU path.)
        self._model = ShardModel(xml=self.default_xml_str, mcs=shape_mcs, device=device, contact_bodies=self.contact_bodies,
                                 control_mode=self.control_mode, clip_actions=self.clip_actions,
                                 pdp_scale=_opt(e, "pdp_scale", 1), pdd_scale=_opt(e, "pdd_scale", 1), sim_timestep_inv=self.sim_timestep_inv, lazy=True)
        if shape_mcs is not None and len(shape_mcs) > 1:
            kw["shape_id"] = list(range(num_envs))
        self._num_envs = num_envs
        self._vec_kw = dict(model=self._model, task=self._TASK, state_init=e.state_init,
                            self_obs_v=self.self_obs_v, control_mode=self.control_mode,
                            episode_length=self.max_episode_length, control_freq_inv=self.control_freq_inv,
                            root_height_obs=self._root_height_obs, power_scale=float(self.power_scale),
                            autoreset=False, self_collision=self.self_collision, **kw)
        self._vec_obj, self._vec_pid = None, None
        mc = self._model.mc
        self.mj_body_names = ["world"] + list(mc.body_names)
        self.body_names_orig = list(mc.body_names)
        self.num_rigid_bodies = mc.nbody
        self.dof_names = self.body_names_orig[1:]
        self.dof_size = mc.nu
        self.actuator_names = list(mc.actuator_names)
        self.qpos_lim, self.qvel_lim = mc.nq, mc.nv
        self.jkp, self.jkd, self.torque_lim, self._pd_action_scale, self._pd_action_offset = self._model.tables
        self.mj_data = _MjDataView(self)
        self.mj_model = types.SimpleNamespace(nq=mc.nq, nv=mc.nv, nu=mc.nu, nbody=mc.nbody + 1,
                                              opt=types.SimpleNamespace(timestep=self.sim_timestep))
        n_obs, n_act = self.get_obs_size(), self.get_action_size()
        self.observation_space = Box(-np.inf * np.ones(n_obs), np.inf * np.ones(n_obs), dtype=self.dtype)
        lim = np.ones(n_act) if self.clip_actions else np.inf * np.ones(n_act)
        self.action_space = Box(-lim, lim, dtype=self.dtype)
        self.np_random = np.random.default_rng()
        self.cur_t = 0
        self.reward_info = {}
        self.viewer = self.renderer = None

    @property
    def _vec(self):
        """The GPU batch of this env object, created on first use in the calling process (see __init__)."""
        if self._vec_obj is None or self._vec_pid != os.getpid():
            self._vec_obj, self._vec_pid = SMPLSimVecEnv(self._num_envs, **self._vec_kw), os.getpid()
            # the host formulas of get_obs_size() (spaces are needed before any device exists) against the library's ss_obs_size
            assert self._vec_obj.obs_size == self.get_obs_size(), (self._vec_obj.obs_size, self.get_obs_size())
        return self._vec_obj

    # ---- sizes
    def _task_kwargs(self, e):
        return {}

    def get_action_size(self):
        return self.dof_size

    def get_obs_size(self):
        return self.get_self_obs_size() + self.get_task_obs_size()

    def get_self_obs_size(self):
        # reference humanoid_env.py:293-299 (= ss_obs_size of the library, without needing the device; checked against it when the
        # device batch is created).  With has_shape_variation the reference adds 10 to _num_self_obs (:304-305) although its
        # compute_proprioception produces no shape entries — its declared space and its observation disagree; here the space has
        # the observation's length (INTEGRATION.md "deviations")
        nb = self._model.mc.nbody
        nd = 3 * (nb - 1)
        return (1 if self._root_height_obs else 0) + nd + (6 * nb + 6 + nd if self.self_obs_v == 1 else 12 * nb)

    def get_task_obs_size(self):
        return 0

    # ---- gym API
    def seed(self, seed=None):
        self.np_random = np.random.default_rng(seed)

    def _fall_rand(self):
        """StateInit.Fall draws action = np_random.random(nu) - 0.5 three times, in init_humanoid only (humanoid_env.py:485-488):
        self.np_random advances on resets and never between them."""
        import torch
        v = self._vec
        if v.state_init != 1:
            return None
        return torch.as_tensor(self.np_random.random((v.num_envs, 3, v.nu)), dtype=torch.float32, device=v.device)

    def _task_rand(self):
        """Task targets use the global numpy RNG in the reference (humanoid_speed.py:97-103), on reset and on target changes."""
        import torch
        v = self._vec
        if v.task_id == 0:
            return None
        return torch.as_tensor(np.random.random((v.num_envs, 4)), dtype=torch.float32, device=v.device)

    def reset(self, seed=None, options=None):
        if seed is not None:
            self.seed(seed)
        obs, _ = self._vec.reset(fall_actions=self._fall_rand(), task_rand=self._task_rand())
        self.cur_t = 0
        o = obs[0].cpu().numpy().astype(self.dtype)
        return o, {"critic_state": o}

    def step(self, action):
        import torch
        v = self._vec
        a = torch.as_tensor(np.asarray(action, dtype=np.float32)[None, : v.nu], device=v.device)
        obs, rew, term, trunc, _ = v.step(a, task_rand=self._task_rand())
        self.cur_t += 1
        o = obs[0].cpu().numpy().astype(self.dtype)
        info = dict(self.reward_info)
        info["critic_state"] = o
        return o, float(rew[0].item()), bool(term[0].item()), bool(trunc[0].item()), info

    def render(self):
        return None

    def close(self):
        if self._vec_obj is not None and self._vec_pid == os.getpid():
            self._vec_obj.close()

    @property
    def curr_power_usage(self):
        """reference humanoid_env.py:443-451: one array [nv - 6] per mj_step of the last control step, |qfrc_actuator * qvel| with the
        torque applied in that mj_step and the velocity after it.  Recorded from the first access on (the step launch writes it as
        an optional by-product): empty before the next step."""
        v = self._vec
        first = getattr(v, "power_usage", None) is None
        p = v.enable_power_usage()
        if first or self.cur_t == 0:
            return []
        return [row.astype(np.float64) for row in p[0].cpu().numpy()]

    # ---- state accessors used by callers of the reference env
    def get_qpos(self):
        return self.mj_data.qpos

    def get_qvel(self):
        return self.mj_data.qvel

    def get_body_xpos(self):
        return self._vec.kinematics()[0][0].cpu().numpy().astype(np.float64)

    def get_body_contact_force(self):
        """[nbody, 3] net contact force on every body (world frame, N) at the last mj_step of the last control step
        (SMPLSimVecEnv.enable_contact_forces).  The first call turns the output on: values are valid from the next step on."""
        return self._vec.enable_contact_forces()[0].cpu().numpy().astype(np.float64)

    def get_root_pos(self):
        return self.get_qpos()[:3].copy()


class HumanoidTask(HumanoidEnv):
    pass


class HumanoidSpeed(HumanoidTask):
    _TASK = "HumanoidSpeed"

    def _task_kwargs(self, e):
        return dict(tar_speed=(e.tar_speed_min, e.tar_speed_max),
                    speed_change=(e.speed_change_steps_min, e.speed_change_steps_max))

    def get_task_obs_size(self):
        return 3


class HumanoidGetup(HumanoidTask):
    _TASK = "HumanoidGetup"

    def _task_kwargs(self, e):
        return dict(tar_height=(e.tar_height_min, e.tar_height_max),
                    height_change=(e.height_change_steps_min, e.height_change_steps_max),
                    recovery_steps=e.recovery_steps)

    def get_task_obs_size(self):
        return 1


class HumanoidReach(HumanoidTask):
    _TASK = "HumanoidReach"

    def _task_kwargs(self, e):
        return dict(tar_height=(e.tar_height_min, e.tar_height_max), tar_dist_max=e.tar_dist_max,
                    height_change=(e.tar_change_steps_min, e.tar_change_steps_max), reach_body=e.reach_body_name)

    def get_task_obs_size(self):
        return 3


class SMPLSimGymVecEnv:
    """numpy-in / numpy-out vector env with the attributes `examples/benchmark.py:97-116` touches on a
    `gym.vector` env (`num_envs`, `action_space.sample()`, `reset(seed=)`, `step(actions=)`), backed by one
    HIP launch for all envs instead of one OS process per env (reference benchmark.py:78-81)."""

    def __init__(self, cfg, num_envs, device=0, autoreset=True, bodies=None):
        import torch
        cls = {"HumanoidEnv": HumanoidEnv, "HumanoidSpeed": HumanoidSpeed, "HumanoidGetup": HumanoidGetup,
               "HumanoidReach": HumanoidReach}[cfg.env.task]
        self._single = cls(cfg, device=device, num_envs=num_envs, bodies=bodies)   # bodies: see HumanoidEnv (has_shape_variation)
        self._vec = self._single._vec
        self._vec.autoreset = autoreset
        self.num_envs = num_envs
        self.single_observation_space = self._single.observation_space
        self.single_action_space = self._single.action_space
        n_act = self._single.get_action_size()
        lim = np.ones((num_envs, n_act))
        self.action_space = Box(-lim, lim, dtype=np.float32)
        self.observation_space = Box(-np.inf * np.ones((num_envs, self._vec.obs_size)),
                                     np.inf * np.ones((num_envs, self._vec.obs_size)), dtype=np.float32)
        self._torch = torch

    def reset(self, seed=None, options=None):
        if seed is not None:
            self._single.seed(seed)
            self._vec.gen.manual_seed(int(seed))
        obs, _ = self._vec.reset()
        o = obs.cpu().numpy()
        return o, {"critic_state": o}

    def step(self, actions):
        t = self._torch
        a = t.as_tensor(np.asarray(actions, dtype=np.float32), device=self._vec.device)
        obs, rew, term, trunc, info = self._vec.step(a)
        out = {"critic_state": obs.cpu().numpy()}
        if "final_observation" in info:
            out["final_observation"] = info["final_observation"].cpu().numpy()
        return obs.cpu().numpy(), rew.cpu().numpy().astype(np.float64), term.cpu().numpy(), trunc.cpu().numpy(), out

    def close(self):
        self._vec.close()
