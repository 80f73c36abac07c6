"""ctypes bindings of the C ABI, derived from include/smplsim_hip.h, smplsim_motion.h, smplsim_mlp.h and smplsim_wrench.h when this module is imported.

The headers are the one description of the ABI: _cheader.parse reads their structs, prototypes and integer constants, and `_ctype`
below is the one mapping from a C type to ctypes.  Nothing here repeats a field list, an argument list, a function name or a
constant's value; a new entry point is declared in the header and is bound.  tests/test_cabi_cpu.py holds the result against
clang's reading of the same headers.

`bind(cdll)` attaches the prototypes of smplsim_hip.h and smplsim_motion.h to an already-loaded library, `bind_mlp(cdll)` those of
smplsim_mlp.h (product library only: the matrix-core kernels), `bind_wrench(cdll)` that of smplsim_wrench.h (the body-wrench input).  The product loads libsmplsim_hip.so through smplsim_amd/_lib.py;
tests bind the same declarations onto the wavefront-emulator build of the kernel source.
"""
import ctypes as C
import os
import re

import numpy as np

from . import _cheader

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = {n: _cheader.parse(open(os.path.join(_INCLUDE, n)).read(), n) for n in ("smplsim_hip.h", "smplsim_motion.h", "smplsim_mlp.h", "smplsim_wrench.h")}

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "uint8_t": C.c_uint8}
_PY_NAMES = {"ss_model_desc": "ModelDesc", "ss_env_cfg": "EnvCfg", "ss_state": "State", "ss_mjcf_options": "MjcfOptions", "ss_skeleton": "Skeleton",
             "ss_motion_data": "MotionData", "ss_motion_state": "MotionState", "ss_imitation_cfg": "ImitationCfg", "ss_imitation_io": "ImitationIO",
             "ss_adam_tensor": "AdamTensor", "ss_gather_tensor": "GatherTensor"}
STRUCTS = {}                     # C name -> ctypes.Structure class; the classes are module attributes under their _PY_NAMES
_OPAQUE = {o for h in HEADERS.values() for o in h.opaque}


def _ctype(ctype):
    """C type (in the spelling of _cheader) -> ctypes, for parameters, results and struct fields alike.  Data pointers and handles are
    c_void_p (it takes None, an address, byref(...) and an array); only what a caller fills in through ctypes keeps its pointee."""
    base = " ".join(w for w in re.findall(r"\w+", ctype.split("[")[0]) if w not in ("const", "struct"))
    stars, bound = ctype.count("*"), re.search(r"\[(\d+)\]$", ctype)
    if stars == 0:
        t = None if base == "void" else STRUCTS[base] if base in STRUCTS else _SCALARS[base]
        return t * int(bound.group(1)) if bound else t
    if base == "char" and stars <= 2:
        return C.c_char_p if stars == 1 else C.POINTER(C.c_char_p)
    if base in STRUCTS and stars == 1:
        return C.POINTER(STRUCTS[base])
    if base in _OPAQUE and stars == 2:
        return C.POINTER(C.c_void_p)
    return C.c_void_p


for _hname, _h in HEADERS.items():
    for _cname, _fields in _h.structs.items():
        STRUCTS[_cname] = type(_PY_NAMES[_cname], (C.Structure,), {"_fields_": [(f, _ctype(t)) for f, t in _fields],
                                                                   "__doc__": f"{_cname} of include/{_hname}"})
globals().update({c.__name__: c for c in STRUCTS.values()})

# header -> {function: (restype, argtypes)}
PROTOTYPES = {hname: {f: (_ctype(ret), [_ctype(p) for p in params]) for f, (ret, params) in h.functions.items()} for hname, h in HEADERS.items()}
EXPORTS = [f for hname in ("smplsim_hip.h", "smplsim_motion.h") for f in PROTOTYPES[hname]]
MLP_EXPORTS = list(PROTOTYPES["smplsim_mlp.h"])
WRENCH_EXPORTS = list(PROTOTYPES["smplsim_wrench.h"])


def _bind(lib, *hnames):
    for hname in hnames:
        for f, (restype, argtypes) in PROTOTYPES[hname].items():
            fn = getattr(lib, f)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind(lib):
    return _bind(lib, "smplsim_hip.h", "smplsim_motion.h")


def bind_mlp(lib):
    return _bind(lib, "smplsim_mlp.h")


def bind_wrench(lib):
    return _bind(lib, "smplsim_wrench.h")


CONSTANTS = {k: v for h in HEADERS.values() for k, v in h.constants.items()}      # every enumerator and integer define


def _family(prefix, end=None):
    """{lower-case name: value} of the constants `prefix`*, by value; `end` names the enumerator that closes the family (a count)."""
    return {k[len(prefix):].lower(): v for k, v in sorted(CONSTANTS.items(), key=lambda kv: kv[1])
            if k.startswith(prefix) and (end is None or v < CONSTANTS[end])}


TASK_BASE, TASK_SPEED, TASK_GETUP, TASK_REACH = (CONSTANTS["SS_TASK_" + n] for n in ("BASE", "SPEED", "GETUP", "REACH"))
INIT_DEFAULT, INIT_FALL, INIT_EXTERNAL = (CONSTANTS["SS_INIT_" + n] for n in ("DEFAULT", "FALL", "EXTERNAL"))
CTRL_UHC_PD, CTRL_PD, CTRL_TORQUE, CTRL_SIMPLE_PID, CTRL_DEFAULT = (CONSTANTS["SS_CTRL_" + n] for n in ("UHC_PD", "PD", "TORQUE", "SIMPLE_PID", "DEFAULT"))
# the names only Python knows: the reference's env classes, control_mode strings and StateInit members
TASKS = {"HumanoidEnv": TASK_BASE, "HumanoidSpeed": TASK_SPEED, "HumanoidGetup": TASK_GETUP, "HumanoidReach": TASK_REACH}
CONTROL_MODES = {"uhc_pd": CTRL_UHC_PD, "pd": CTRL_PD, "torque": CTRL_TORQUE, "simple_pid": CTRL_SIMPLE_PID,
                 "default": CTRL_DEFAULT}
STATE_INITS = {"Default": INIT_DEFAULT, "Fall": INIT_FALL, "External": INIT_EXTERNAL}
SS_MAX_SELF_CONTACTS = CONSTANTS["SS_MAX_SELF_CONTACTS"]           # one body-body contact per lane of the env's wavefront
FIELDS = _family("SS_FIELD_")                                      # ss_get_state / ss_set_state
ACTIVATIONS = _family("SS_ACT_")
NORM_BLOCK_ROWS = CONSTANTS["SS_NORM_BLOCK_ROWS"]                  # rows per (mean, M2) pair in the workspace of ss_running_norm_update
EPISODE_MAX_PARTS = CONSTANTS["SS_EPISODE_MAX_PARTS"]              # reward terms of one ss_episode_stats call
EPISODE_STATS = tuple(_family("SS_EP_", "SS_EP_PARTS"))            # the fixed statistics of ss_episode_stats, in the order of `stats`; the P part sums follow
CLIP_COLUMNS = tuple(_family("SS_CLIP_", "SS_CLIP_COLUMNS"))       # the columns of the [M, 3] int64 counters of ss_clip_outcomes
MOTION_DATA_ARRAYS = tuple(f for f, t in HEADERS["smplsim_motion.h"].structs["ss_motion_data"] if "*" in t)
MOTION_STATE_FIELDS = tuple(f for f, _ in HEADERS["smplsim_motion.h"].structs["ss_motion_state"])
# These two limits have no macro in a public header (smplsim_mlp.h states them in prose, csrc/ holds the numbers): Python constants.
ADAM_MAX_TENSORS = 32            # tensors of one ss_adam_step call (the table travels in the kernel arguments)
GATHER_MAX_TENSORS = 8           # tensors of one ss_gather_rows call


def make_model_desc(mc, kp, kd, torque_lim, act_scale, act_offset, legal_bodies=(), timestep=1.0 / 450):
    """ModelConst (smplsim_amd.mjcf) + actuator tables -> (ModelDesc, keepalive list)."""
    keep = []

    def arr(x, dt):
        a = np.ascontiguousarray(x, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    d = ModelDesc()
    d.nbody = mc.nbody
    d.body_parent = arr(mc.body_parent, np.int32)
    for name in ("body_pos", "body_mass", "body_ipos", "body_iquat", "body_inertia", "geom_size", "geom_pos",
                 "geom_quat", "dof_armature", "jnt_range", "body_invweight0", "dof_invweight0", "qpos0"):
        setattr(d, name, arr(getattr(mc, name), np.float64))
    d.geom_type = arr(mc.geom_type, np.int32)
    d.jnt_limited = arr(mc.jnt_limited, np.uint8)
    d.nu = mc.nu
    d.actuator_dof = arr(mc.actuator_dof, np.int32)
    d.kp, d.kd, d.torque_lim = arr(kp, np.float64), arr(kd, np.float64), arr(torque_lim, np.float64)
    d.act_scale, d.act_offset = arr(act_scale, np.float64), arr(act_offset, np.float64)
    d.legal_contact = arr([int(n in legal_bodies) for n in mc.body_names], np.uint8)
    d.timestep, d.gravity = timestep, mc.gravity
    d.solref = (C.c_double * 2)(*mc.solref)
    d.solimp = (C.c_double * 5)(*mc.solimp)
    d.margin, d.friction, d.impratio = mc.geom_margin, mc.friction, mc.impratio
    d.geom_contype = arr(mc.geom_contype, np.int32)
    d.geom_conaffinity = arr(mc.geom_conaffinity, np.int32)
    ex = [(mc.body_names.index(a), mc.body_names.index(b)) for a, b in mc.excludes]
    d.nexclude = len(ex)
    d.exclude = arr(np.array(ex, dtype=np.int32).reshape(-1, 2), np.int32) if ex else None
    d.meaninertia = mc.meaninertia
    return d, keep


def make_env_cfg(task=TASK_BASE, state_init=INIT_DEFAULT, self_obs_v=1, control_mode=CTRL_UHC_PD,
                 episode_length=300, control_freq_inv=15, root_height_obs=True, power_scale=1.0,
                 tar_speed=(0.0, 5.0), speed_change=(100, 200), tar_height=(0.5, 1.2), height_change=(100, 200),
                 recovery_steps=60, newton_iters=0, tar_dist_max=1.0, reach_body=0, self_collision=False, solver_tolerance=0.0):
    """newton_iters / solver_tolerance: mjOption.iterations / tolerance; 0 = MuJoCo's defaults (100, 1e-8)."""
    return EnvCfg(task=task, state_init=state_init, self_obs_v=self_obs_v, control_mode=control_mode, episode_length=episode_length,
                  control_freq_inv=control_freq_inv, root_height_obs=int(root_height_obs), power_scale=power_scale,
                  tar_speed_min=tar_speed[0], tar_speed_max=tar_speed[1], speed_change_min=speed_change[0], speed_change_max=speed_change[1],
                  tar_height_min=tar_height[0], tar_height_max=tar_height[1], height_change_min=height_change[0],
                  height_change_max=height_change[1], recovery_steps=recovery_steps, newton_iters=newton_iters, tar_dist_max=tar_dist_max,
                  reach_body=reach_body, self_collision=int(bool(self_collision)), solver_tolerance=solver_tolerance)
