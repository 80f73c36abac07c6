"""The motion-library kernels (ss_motion.h) at their clip, tile and blend edges: builders of two small edge libraries and the
check_* functions that test_motion_edges_emu.py runs on the CPU emulator and test_motion_edges_gpu.py on the device.

Every check takes the library handle (the emulator's or the product's) and builds its own small library; the device is the
library's.  The float64 reference is oracle/motion_oracle.py throughout.  Tolerances are test_motion_lib.py's (TOL,
check_blended, check_imitation); the two derived ones are stated where they are used.  Each check prints its figures before it
asserts and its docstring records the largest ones seen.

The 24-body library (F = 70 frames: neither a multiple of the 16-frame velocity tile nor of the 8 frames of an FK block):

  a 14 frames  30 fps     smooth; makes every later clip straddle a 16-frame tile
  b  2 frames  60 fps     every filter tap is an edge sample
  c  5 frames  30 fps     one pose held: consecutive quaternions equal (slerp's c >= 1 branch), zero velocities
  d  6 frames 120 fps     2e-4 rad per joint and frame (slerp's sn < 1e-3 branch)
  e  7 frames  30 fps     every joint turns 2.6 rad per frame about its own axis: sign flips in slerp and in raw_velocity's
                          dq.w < 0, and fix_continous_dof fires
  f  3 frames  29.97 fps  a frame time that is no float32 reciprocal of an integer
  g 33 frames  30 fps     sinusoidal; spans three velocity tiles

The 52-body library (clips of 2, 19 and 5 frames, F = 26) takes the 64-lane forward-kinematics and imitation layouts and the
one-wave velocity workgroup.
"""
import ctypes as C

import numpy as np
import torch

import test_motion_lib as T
from oracle import motion_oracle as mo

SENT = -7.75e7                 # sentinel of pre-filled outputs and guard rows (exact in float32)
GUARD = 3                      # guard rows behind every output of a lookup / resample / imitation launch
CLIP_NAMES = "abcdefg"
OBS_DT = np.float32(1.0 / 30)


# ------------------------------------------------------------------------------------------------ builders
def skeleton(J):
    from smplsim_amd.motion_lib import Skeleton
    from smplsim_amd.mjcf import compile_mjcf
    from smplsim_amd.mjcf_writer import default_xml_str
    if J == 24:
        return Skeleton.from_model_const(compile_mjcf(default_xml_str("smpl_humanoid")))
    mc = compile_mjcf(default_xml_str("smplx_humanoid"))       # as test_motion_lib.smplx_lib: a scrambled "SMPL" joint order
    rs = np.random.default_rng(52)
    perm = rs.permutation(52)
    perm[list(perm).index(0)], perm[0] = perm[0], 0
    return Skeleton(mc.body_names, mc.body_parent, mc.body_pos, smpl_order_names=[mc.body_names[i] for i in perm])


def _smooth(rs, nf, fps, J):
    t = np.arange(nf)[:, None, None] / fps
    pose = rs.normal(size=(1, J, 3)) * 0.4 + 0.5 * np.sin(2 * np.pi * rs.uniform(0.5, 2, size=(1, J, 3)) * t)
    t = t[:, 0, 0]
    return pose, np.stack([0.5 * t, 0.1 * np.sin(3 * t), 0.95 + 0.02 * np.cos(5 * t)], -1)


def _unit(rs, shape):
    v = rs.normal(size=shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def edge_clips(J):
    rs = np.random.default_rng(7024 + J)
    if J != 24:
        spec = [("x0", 2, 30.0, "smooth"), ("x1", 19, 30.0, "smooth"), ("x2", 5, 30.0, "smooth")]
    else:
        spec = [("a", 14, 30.0, "smooth"), ("b", 2, 60.0, "smooth"), ("c", 5, 30.0, "held"), ("d", 6, 120.0, "tiny"), ("e", 7, 30.0, "spin"),
                ("f", 3, 29.97, "smooth"), ("g", 33, 30.0, "smooth")]
    clips = {}
    for name, nf, fps, kind in spec:
        pose, trans = _smooth(rs, nf, fps, J)
        k = np.arange(nf)[:, None, None]
        if kind == "held":
            pose, trans = np.repeat(pose[:1], nf, 0), np.repeat(trans[:1], nf, 0)
        elif kind == "tiny":
            pose = pose[:1] + k * 2e-4 * _unit(rs, (1, J, 3))
            trans = trans[:1] + k[:, 0] * 1e-4 * _unit(rs, (1, 3))
        elif kind == "spin":                                     # the angle kept in (-pi, pi], as clip files have it
            ph, axis = rs.uniform(0, 2 * np.pi, size=(1, J, 1)), _unit(rs, (1, J, 3))
            # three joints about their y axis from 0.2 rad: frame 1 is at 2.8 rad, whose XYZ Euler angles come out as
            # (pi, pi - 2.8, pi) and are put back to (0, 2.8, 0) by fix_continous_dof (a general axis turns too far for its flip to help)
            ph[0, [5, 12, 20]], axis[0, [5, 12, 20]] = 0.2, (0.0, 1.0, 0.0)
            pose = axis * ((ph + 2.6 * k + np.pi) % (2 * np.pi) - np.pi)
        clips[name] = dict(pose_aa=pose.reshape(nf, 3 * J).astype(np.float32), trans=trans.astype(np.float32), fps=fps)
    return clips


def build_lib(J, filter_vel=True):
    """(library, clips) on the backend the package is bound to: the emulator under the emu_backend fixture, else cuda:0."""
    from smplsim_amd.motion_lib import MotionLibSMPL
    clips = edge_clips(J)
    lib = MotionLibSMPL(clips, skeleton(J), device=0, filter_vel=filter_vel)
    lib.load_motions(random_sample=False)
    assert int(lib._motion_num_frames.sum()) == (70 if J == 24 else 26)
    return lib, clips


def _sync(device):
    if torch.device(device).type != "cpu":
        torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(lib, a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(lib.device)


def _rot_err(got, want):
    """per quaternion: distance up to sign"""
    return np.minimum(np.abs(got - want).max(-1), np.abs(got + want).max(-1))


def oracle_cook(lib, clips, filt):
    sk = lib.skeleton
    J = sk.num_joints
    return [mo.cook(c["pose_aa"].reshape(-1, J, 3), c["trans"], sk.offsets, sk.parents, sk.smpl_2_mujoco, float(lib._motion_dt[m]), filt)
            for m, c in enumerate(clips.values())]


# ------------------------------------------------------------------------------------------------ 2. cook
def cook_guarded(lib, clib, filt):
    """ss_motion_cook of the library's clips into arrays of its own, each with one more frame of sentinel behind it."""
    from smplsim_amd import _cabi
    F, J, M = int(lib._motion_num_frames.sum()), lib.skeleton.num_joints, lib.num_current_motions()
    row = dict(gts=(J, 3), grs=(J, 4), lrs=(J, 4), gvs=(J, 3), gavs=(J, 3), dof_pos=(J - 1, 3), dvs=(J - 1, 3), qpos=(7 + 3 * (J - 1),),
               qvel=(6 + 3 * (J - 1),))
    buf = {k: torch.full((F + 1,) + s, SENT, dtype=torch.float32, device=lib.device) for k, s in row.items()}
    data = _cabi.MotionData(M, F, J, *[_ptr(buf[k] if k in buf else lib._d[k]) for k in _cabi.MOTION_DATA_ARRAYS])
    skel = _cabi.Skeleton(J, lib._sk_keep[0].ctypes.data_as(C.c_void_p), lib._sk_keep[1].ctypes.data_as(C.c_void_p))
    assert clib.ss_motion_cook(C.byref(skel), C.byref(data), int(filt), lib._stream()) == 0, clib.ss_last_error()
    _sync(lib.device)
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    for k, v in out.items():
        assert (v[F] == np.float32(SENT)).all(), ("guard frame written", k)
        assert np.array_equal(v[:F], getattr(lib, k).cpu().numpy()), ("two cooks of the same clips differ", k)
    return {k: v[:F] for k, v in out.items()}


def check_cook(clib, J, filt):
    """Every cooked array of every clip against mo.cook, within test_motion_lib.TOL; the angular-velocity arrays (gavs, qvel)
    within TOL * max(1, fps / 30), the scaling of that module's docstring (acos noise per frame, times fps).  The frame behind
    each array stays untouched.

    Largest error / bound seen, emulator | MI355X, over both skeletons and filter on and off (worst clip):
      gts 3.3e-7 | 3.7e-7 / 2e-5; grs 2.8e-7 | 3.0e-7 / 2e-5; lrs 1.1e-7 | 1.1e-7 / 2e-5; dof_pos, qpos 1.9e-6 | 2.0e-6 / 2e-5 (f)
      gvs 4.1e-5 | 3.8e-5 / 2e-3 (d); dvs 6.6e-5 | 6.2e-5 / 2e-3 (f)
      gavs at 30, 29.97 and 60 fps 3.1e-4 | 1.0e-4 / 5e-2; qvel there 1.2e-4 | 1.2e-4 / 5e-2
      gavs of clip d (120 fps) 7.2e-2 | 7.2e-2 unfiltered, 7.1e-2 | 7.1e-2 filtered / 2e-1; its qvel 2.2e-2 | 2.2e-2 / 2e-1
    """
    lib, clips = build_lib(J, filt)
    got = cook_guarded(lib, clib, filt)
    want = oracle_cook(lib, clips, filt)
    if J == 24:     # from the oracle alone: the reference's Euler-angle fix changes clip e
        e = list(clips).index("e")
        c = clips["e"]
        raw = mo.matrix_to_euler_xyz(mo.quaternion_to_matrix(mo.axis_angle_to_quaternion(c["pose_aa"].reshape(-1, J, 3).astype(np.float64)))
                                     [:, lib.skeleton.smpl_2_mujoco])[:, 1:]
        assert (np.abs(raw - want[e]["dof_pos"]) > 1e-3).any()
    worst = {}
    for m, name in enumerate(clips):
        s, nf, fps = int(lib.length_starts[m]), int(lib._motion_num_frames[m]), float(lib._motion_fps[m])
        for k, attr in T.NAMES.items():
            g = got[attr][s:s + nf]
            ref = want[m][k].reshape(g.shape)
            err = _rot_err(g, ref).max() if k.endswith("rotation") else np.abs(g - ref).max()
            tol = T.TOL[k] * (max(1.0, fps / 30.0) if attr in ("gavs", "qvel") else 1.0)
            print(f"cook J={J} filter={int(filt)} clip {name} {attr}: {err:.3g} / {tol:.3g}")
            if err / tol > worst.get(attr, (0, 0, 0))[0]:
                worst[attr] = (err / tol, err, name)
            assert err < tol, (name, k, err, tol)
    return worst


# ------------------------------------------------------------------------------------------------ 3. blended lookup
def edge_queries(lib):
    """(ids, float32 times): every frame boundary float32(k dt) of every clip and its two float32 neighbours, and per clip
    -1, length, length + 3, 0.37 length, 0.25 dt, 0.5 dt, (nf - 1.5) dt."""
    ids, times = [], []
    for m in range(lib.num_current_motions()):
        nf, dt, L = int(lib._motion_num_frames[m]), np.float32(lib._motion_dt[m]), np.float32(lib._motion_lengths[m])
        t = []
        for k in range(nf):
            b = np.float32(k) * dt
            t += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
        t += [-1.0, L, L + np.float32(3), np.float32(0.37) * L, np.float32(0.25) * dt, np.float32(0.5) * dt, np.float32(nf - 1.5) * dt]
        ids += [m] * len(t)
        times += t
    return np.array(ids, np.int32), np.array(times, np.float32)


def slerp_census(arr, ids, times):
    """Which branch of the three-branch slerp each (query, body) pair takes, by the float64 oracle on the cooked arrays; and
    the allowance of the pairs near its branch points."""
    i0, i1, _ = mo.calc_frame_blend(times.astype(np.float64), arr["lengths"][ids], arr["num_frames"][ids], arr["dt"][ids])
    q0, q1 = arr["grs"][i0 + arr["length_starts"][ids]], arr["grs"][i1 + arr["length_starts"][ids]]
    c = (q0 * q1).sum(-1)
    neg = c < 0
    q1 = np.where(neg[..., None], -q1, q1)
    c = np.abs(c)
    sn = np.sqrt(np.maximum(1 - c * c, 0))
    ge1 = c >= 1
    small = ~ge1 & (sn < 1e-3)
    # c >= 1 returns q0 and sn < 1e-3 returns the midpoint: around those two points the function jumps by up to half the
    # distance of the two quaternions, and float32 and float64 may be on different sides of them
    allow = np.where(sn < 2e-3, 0.5 * np.abs(q1 - q0).max(-1), 0.0)
    return dict(neg=neg, ge1=ge1, small=small, general=~ge1 & ~small, f0=i0 + arr["length_starts"][ids], f1=i1 + arr["length_starts"][ids]), allow


def check_blended_edges(clib, J):
    """ss_motion_state_at (blended) at every frame boundary +- one float32 spacing, at and beyond both clip ends, against
    mo.motion_state on the library's own cooked arrays, at check_blended's tolerances: 1e-4 positions and dofs, 5e-3
    velocities, 2e-4 rotations up to sign.  One derived allowance: a (query, body) pair whose float64 sn is below 2e-3 may add
    0.5 max|q1 - q0| (sign-flipped), the size of the slerp's own jump at its two branch points.  Quaternion norms within 1e-4
    of 1.  The branch census comes from the oracle, not from the kernel.

    Largest error / bound seen, emulator | MI355X:
      24 bodies: 6216 pairs, c < 0 602 | 602, c >= 1 1007 | 1010, sn < 1e-3 601 | 598, general 4608 | 4608 (the cooked arrays differ
        in their last bits); 259 | 256 of the c >= 1 pairs have q0 != q1
        rotations minus allowance 3.0e-5 | 3.0e-5 / 2e-4; positions 4.4e-7 | 3.8e-7 / 1e-4; dofs 7.2e-7 | 4.5e-7 / 1e-4;
        velocities 3.3e-5 | 2.3e-5 / 5e-3; |norm - 1| 1.2e-5 | 1.2e-5 / 1e-4; qvel[3:6] 7.5e-6 | 6.2e-6 / 5e-3
      52 bodies: rotations 1.9e-5 | 1.9e-5; positions 4.4e-7 | 4.4e-7; dofs 6.5e-7 | 6.5e-7; velocities 8.1e-6 | 8.1e-6;
        |norm - 1| 2.3e-5 | 2.3e-5
    """
    lib, _ = build_lib(J)
    rs = np.random.default_rng(31)
    ids, times = edge_queries(lib)
    n = len(ids)
    off = rs.normal(size=(n, 3)).astype(np.float32)
    arr = T.lib_arrays(lib)
    census, allow = slerp_census(arr, ids, times)
    counts = {k: int(census[k].sum()) for k in ("neg", "ge1", "small", "general")}
    print(f"lookup J={J}: {n} queries, {n * J} pairs, branches {counts}")
    if J == 24:
        assert n * J == 6216
        assert counts["neg"] >= 1 and counts["ge1"] >= 1 and counts["small"] >= 1 and counts["general"] > n * J // 2, counts
    got = {k: v.cpu().numpy() for k, v in lib.get_motion_state(ids, times, offset=off, with_qpos=True).items()}
    want = mo.motion_state(arr, ids, times.astype(np.float64), off.astype(np.float64))
    worst = {}
    for k, v in want.items():
        g = got[k]
        if k.endswith("rot"):
            err, tol = (_rot_err(g, v) - (allow[:, 0] if k == "root_rot" else allow)).max(), 2e-4
            assert np.abs(np.linalg.norm(g, axis=-1) - 1).max() < 1e-4, k
        else:
            err, tol = np.abs(g - v.reshape(g.shape)).max(), 5e-3 if "vel" in k else 1e-4
        print(f"lookup J={J} {k}: {err:.3g} / {tol:.3g}")
        worst[k] = err
        assert err < tol, (k, err)
    # Where the float64 c is >= 1 the kernel has no arithmetic to do.  Its float32 dot product of two unit quaternions is off by
    # less than 4e-7 (seven roundings of at most 3e-8), so it is in its c >= 1 branch, which hands back q0 as loaded, or, from
    # c >= 1 - 4e-7 and sqrt(1 - c^2) <= 9e-4, in its sn < 1e-3 branch, whose 0.5 q0 + 0.5 q1 rounds once, contracted or
    # not: bit for bit one of the two.  (q1 instead of q0 stays inside the allowance above, which is half their distance.)
    grs = lib.grs.cpu().numpy()
    q0, q1 = grs[census["f0"]], grs[census["f1"]]
    q1 = np.where(census["neg"][..., None], -q1, q1)
    mid = np.float32(0.5) * q0 + np.float32(0.5) * q1
    plain = (got["rb_rot"] == q0).all(-1) | (got["rb_rot"] == mid).all(-1)
    moving = census["ge1"] & (q0 != q1).any(-1)
    print(f"lookup J={J}: {int(moving.sum())} pairs with c >= 1 and q0 != q1, {int((~plain & census['ge1']).sum())} of the c >= 1 pairs neither q0 nor the midpoint")
    assert plain[census["ge1"]].all()
    if J == 24:
        assert moving.sum() >= 1
    # qpos / qvel of the blended state: root pose + Euler dofs, body-frame root angular velocity
    qp, qv = got["qpos"], got["qvel"]
    R = mo.quaternion_to_matrix(want["root_rot"])
    extra = dict(qpos_root=np.abs(qp[:, :3] - want["root_pos"]).max(), qpos_dofs=np.abs(qp[:, 7:] - want["dof_pos"]).max(),
                 qpos_quat=(_rot_err(qp[:, 3:7], want["root_rot"]) - allow[:, 0]).max(), qpos_norm=np.abs(np.linalg.norm(qp[:, 3:7], axis=-1) - 1).max(),
                 qvel_lin=np.abs(qv[:, :3] - want["root_vel"]).max(), qvel_ang=np.abs(qv[:, 3:6] - np.einsum("nba,nb->na", R, want["root_ang_vel"])).max(),
                 qvel_dofs=np.abs(qv[:, 6:] - want["dof_vel"]).max())
    print(f"lookup J={J} qpos/qvel:", {k: float(f"{v:.3g}") for k, v in extra.items()})
    assert extra["qpos_root"] < 1e-4 and extra["qpos_dofs"] < 1e-4 and extra["qpos_quat"] < 2e-4 and extra["qpos_norm"] < 1e-4, extra
    assert extra["qvel_lin"] < 5e-3 and extra["qvel_ang"] < 5e-3 and extra["qvel_dofs"] < 5e-3, extra
    worst.update(extra)
    return worst, counts


# ------------------------------------------------------------------------------------------------ 4. intervaled lookup
def check_intervaled_edges(clib, J):
    """ss_motion_state_at (intervaled) at (k + 0.25) dt and (k + 0.75) dt of every frame, at -1 and at length + 3: clear of the
    integer knife edges, where the compiler's contraction may decide the frame.  A gather: every output equals, bit for bit,
    the library's own arrays at mo.intervaled_frame's frame, which is also the frame the times were built for (emulator and
    MI355X: identical).
    And at (nf - 1 + j / 16) dt, j = 1 .. 15, past the end of every clip: the last frame.  The reference's (1 - b) i0 + b i1
    with i0 = i1 = nf - 1 is that integer only in exact arithmetic; rounded in float32 it came out as 12.999999 for the
    14-frame clip, at j = 3 on the emulator and at j = 4 (the (k + 0.25) dt query of the last frame) on the MI355X, and the
    kernel returned the frame before the last until frame_intervaled was rewritten as i0 + b (i1 - i0)."""
    lib, _ = build_lib(J)
    ids, times = [], []
    for m in range(lib.num_current_motions()):
        nf, dt, L = int(lib._motion_num_frames[m]), np.float32(lib._motion_dt[m]), np.float32(lib._motion_lengths[m])
        t = [np.float32(k + f) * dt for k in range(nf) for f in (0.25, 0.75)] + [-1.0, L + np.float32(3)]
        t += [np.float32(nf - 1 + j / 16) * dt for j in range(1, 16)]      # past the end: the last frame, whatever the blend weight
        ids += [m] * len(t)
        times += t
    ids, times = np.array(ids, np.int32), np.array(times, np.float32)
    n = len(ids)
    off = np.random.default_rng(32).normal(size=(n, 3)).astype(np.float32)
    st = {k: v.cpu().numpy() for k, v in lib.get_motion_state_intervaled(ids, times, offset=off).items()}
    fl = mo.intervaled_frame(times, lib._motion_lengths[ids], lib._motion_num_frames[ids], lib._motion_dt[ids]) + lib.length_starts[ids]
    # the frames asked for, from the construction of the times
    want_fl = np.concatenate([np.r_[np.repeat(np.arange(nf), 2), 0, nf - 1, [nf - 1] * 15] + s for nf, s in zip(lib._motion_num_frames, lib.length_starts)])
    assert np.array_equal(fl, want_fl)
    a = {k: getattr(lib, k).cpu().numpy() for k in ("gts", "grs", "gvs", "gavs", "dof_pos", "dvs", "qpos", "qvel")}
    pairs = dict(xpos=a["gts"][fl] + off[:, None], xquat=a["grs"][fl], body_vel=a["gvs"][fl], body_ang_vel=a["gavs"][fl], dof_pos=a["dof_pos"][fl],
                 dof_vel=a["dvs"][fl].reshape(n, -1), qpos=a["qpos"][fl], qvel=a["qvel"][fl], root_pos=a["gts"][fl][:, 0] + off,
                 root_rot=a["grs"][fl][:, 0], root_vel=a["gvs"][fl][:, 0], root_ang_vel=a["gavs"][fl][:, 0])
    for k, v in pairs.items():
        assert np.array_equal(st[k], v), k
    return n


# ------------------------------------------------------------------------------------------------ 5. NULL outputs, mask, strides
def _state_rows(J):
    return dict(root_pos=3, root_rot=4, dof_pos=3 * (J - 1), root_vel=3, root_ang_vel=3, dof_vel=3 * (J - 1), rg_pos=3 * J, rb_rot=4 * J,
                body_vel=3 * J, body_ang_vel=3 * J, qpos=7 + 3 * (J - 1), qvel=6 + 3 * (J - 1))


def check_masked_lookup(clib, J=24, n=257):
    """ss_motion_state_at with a mask of period 3 at N = 257 (N J is no multiple of the 256-thread block), every output
    pre-filled with a sentinel and followed by 3 guard rows: once with every output, once with qpos and qvel only (the
    reference-state write into the simulator), once with rb_rot only; blended and intervaled.  Masked-out rows and guard rows
    keep their bits, and the rows of a subset call equal those of the full call bit for bit (emulator and MI355X: exact)."""
    from smplsim_amd import _cabi
    lib, _ = build_lib(J)
    rs = np.random.default_rng(33)
    eid, et = edge_queries(lib)
    pick = rs.permutation(len(eid))[:n // 2]
    ids = np.concatenate([eid[pick], rs.integers(0, lib.num_current_motions(), size=n - len(pick))]).astype(np.int32)
    times = np.concatenate([et[pick], rs.uniform(-0.1, 1.1, size=n - len(pick)) * lib._motion_lengths[ids[len(pick):]]]).astype(np.float32)
    mask = np.arange(n) % 3 == 1
    d_ids, d_times, d_off, d_mask = _dev(lib, ids, torch.int32), _dev(lib, times), _dev(lib, rs.normal(size=(n, 3))), _dev(lib, mask, torch.uint8)
    rows = _state_rows(J)
    for intervaled in (0, 1):
        res = []
        for fields in (tuple(rows), ("qpos", "qvel"), ("rb_rot",)):
            out = {k: torch.full((n + GUARD, rows[k]), SENT, dtype=torch.float32, device=lib.device) for k in fields}
            st = _cabi.MotionState(**{k: _ptr(v).value for k, v in out.items()})
            assert clib.ss_motion_state_at(C.byref(lib.data), _ptr(d_ids), _ptr(d_times), _ptr(d_off), _ptr(d_mask), n, intervaled, C.byref(st),
                                           lib._stream()) == 0, clib.ss_last_error()
            _sync(lib.device)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            for k, v in out.items():
                assert (v[n:] == np.float32(SENT)).all() and (v[:n][~mask] == np.float32(SENT)).all(), (intervaled, fields, k)
                assert (v[:n][mask] != np.float32(SENT)).all(), (intervaled, fields, k)
                if res:
                    assert np.array_equal(v, res[0][k]), (intervaled, fields, k)
            res.append(out)
        # and the full masked call writes what the unmasked library call returns
        want = lib._lookup(ids, times, d_off, bool(intervaled), list(rows))[0]
        for k in rows:
            assert np.array_equal(res[0][k][:n][mask], want[k].cpu().numpy().reshape(n, -1)[mask]), (intervaled, k)


# ------------------------------------------------------------------------------------------------ 6. resample
RESAMPLE_WEIGHTS = ([1, 0, 3, 0, 2, 0, 0], [0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0])
TOP = np.float32(1 - 2.0 ** -24)                               # the largest float32 below 1


def resample_draws(rs, cdf, n, mask):
    """[n,2] draws: random, and on the first selected rows u0 = each CDF entry, the float32 just below it, 0 and 1 - 2^-24, each
    with u1 = 0, 1 - 2^-24 and a random one."""
    rand = rs.random(size=(n, 2), dtype=np.float32)
    u0 = np.concatenate([cdf, np.nextafter(cdf, np.float32(-np.inf)), [np.float32(0), TOP]]).astype(np.float32)
    special = [(a, b) for a in u0 for b in (np.float32(0), TOP, np.float32(rs.random()))]
    sel = np.flatnonzero(mask)
    k = min(len(sel), len(special))
    order = rs.permutation(len(special))[:k]                       # fewer rows than special draws: a random subset of them
    rand[sel[:k]] = np.array(special, np.float32)[order]
    return rand


def check_resample(clib, J=24):
    """ss_motion_resample against mo.resample, the NumPy float32 restatement: clip ids and start times exact (emulator and
    MI355X: identical), masked rows and 3 guard rows untouched.  Four sets of sampling weights through
    set_termination_history; N = 515 with a mask of period 5, N = 256 and N = 1; truncate_time 0 and 0.15 s (longer than clips
    b, c, d and f: start time 0).
    No clip of zero probability is drawn by any draw inside [0, 1), the range of a uniform draw.  (The draws u0 = a CDF entry
    include 1.0 and 1 + 1e-6, and the one just below a CDF entry of 0 is negative: for those the oracle's own answer, the first
    or the last clip whatever its weight, is what is asserted.)"""
    lib, _ = build_lib(J)
    rs = np.random.default_rng(34)
    M = lib.num_current_motions()
    zero_start = 0
    for w in RESAMPLE_WEIGHTS:
        lib.set_termination_history({"termination_history": np.array(w, np.float64), "failed_keys": []})
        lib.load_motions(random_sample=False)
        cdf, prob = lib.sampling_cdf.cpu().numpy(), lib._sampling_batch_prob
        assert cdf.dtype == np.float32 and len(cdf) == M and np.array_equal(prob > 0, np.array(w) > 0)
        for n, period, truncate in ((515, 5, 0.0), (515, 5, 0.15), (256, 5, 0.15), (1, 0, 0.15), (1, 0, 0.0)):
            mask = np.arange(n) % period != 0 if period else np.ones(n, bool)
            rand = resample_draws(rs, cdf, n, mask)
            if n == 1:
                rand[0] = (TOP, TOP) if truncate else (cdf[rs.integers(0, M)], np.float32(0.5))
            ids = torch.full((n + GUARD,), -5, dtype=torch.int32, device=lib.device)
            t0 = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=lib.device)
            d_rand, d_mask = _dev(lib, rand), (_dev(lib, mask, torch.uint8) if period else None)
            assert clib.ss_motion_resample(C.byref(lib.data), _ptr(d_mask), _ptr(d_rand), _ptr(lib.sampling_cdf), float(truncate), n, _ptr(ids),
                                           _ptr(t0), lib._stream()) == 0, clib.ss_last_error()
            _sync(lib.device)
            ids, t0 = ids.cpu().numpy(), t0.cpu().numpy()
            assert (ids[n:] == -5).all() and (t0[n:] == np.float32(SENT)).all() and (ids[:n][~mask] == -5).all() and (t0[:n][~mask] == np.float32(SENT)).all()
            want_ids, want_t0 = mo.resample(rand, cdf, lib._motion_lengths, truncate)
            assert np.array_equal(ids[:n][mask], want_ids[mask]), (w, n, truncate)
            assert np.array_equal(t0[:n][mask].view(np.uint32), want_t0[mask].view(np.uint32)), (w, n, truncate)
            legit = mask & (rand[:, 0] >= 0) & (rand[:, 0] < 1)
            assert (prob[ids[:n][legit]] > 0).all(), (w, n, truncate)
            if n > 1:
                assert set(np.unique(ids[:n][legit])) == set(np.flatnonzero(np.array(w) > 0)), (w, n)        # every weighted clip is drawn
            short = mask & (lib._motion_lengths[np.where(mask, ids[:n], 0)] < np.float32(truncate))
            assert (t0[:n][short] == 0).all() and (t0[:n][mask] >= 0).all()
            zero_start += int(short.sum())
    assert zero_start > 50                                          # clips shorter than truncate_time were drawn
    return zero_start


# ------------------------------------------------------------------------------------------------ 7. imitation step
def imitation_specs(lib, J):
    """One row per env: (clip, cur_t, spacings of `time + obs_dt` from the clip length or None, exact, distance factor or None)."""
    if J != 24:
        return [(1, 0, None, False, 0.8), (0, 1, None, True, None), (2, 2, None, False, 1.25), (1, 3, -4, True, None), (1, 2, 64, False, None)]
    c = {n: i for i, n in enumerate(CLIP_NAMES)}
    return [(c["b"], 0, None, False, None), (c["c"], 1, None, False, 1.25), (c["d"], 2, None, True, None), (c["e"], 3, -4, True, None),
            (c["g"], 0, 4, False, None), (c["a"], 1, -64, False, 0.8), (c["e"], 2, 64, False, 1.25), (c["g"], 3, None, True, None),
            (c["f"], 1, None, False, 0.8)]


def imitation_case(lib, specs):
    """Start times of the specs.  The kernel forms time = start + cur_t * obs_dt and truncates when time + obs_dt >= length, in
    float32; whether the product and the sum are contracted is the compiler's choice, and the start time, the product and the
    two sums each round once, so the value compared can be 2 float32 spacings from the intended one.  The boundary is
    therefore placed 4 and 64 spacings away, and nothing closer is tested."""
    ids = np.array([s[0] for s in specs], np.int32)
    cur_t = np.array([s[1] for s in specs], np.int32)
    L = lib._motion_lengths[ids]
    times = np.empty(len(specs), np.float32)
    for i, (m, ct, ulps, _, _) in enumerate(specs):
        if ulps is None:
            times[i] = np.float32(0.3) * L[i]
        else:
            target = np.float64(L[i]) + ulps * np.float64(np.spacing(L[i]))
            times[i] = np.float32(target - np.float64(OBS_DT) - ct * np.float64(OBS_DT))
        assert times[i] >= 0
    # the expected flag, in float32 as the kernel states it; and in float64, at least 3 spacings clear of the boundary
    end32 = (times + cur_t.astype(np.float32) * OBS_DT).astype(np.float32) + OBS_DT
    end64 = times.astype(np.float64) + cur_t * np.float64(OBS_DT) + np.float64(OBS_DT)
    assert (np.abs(end64 - L) > 3 * np.spacing(L)).all()
    want_trunc = end32 >= L
    assert np.array_equal(want_trunc, end64 >= L)
    for i, s in enumerate(specs):
        if s[2] is not None:
            assert want_trunc[i] == (s[2] > 0)
    exact = np.array([s[3] for s in specs])
    dist = np.array([np.nan if s[4] is None else s[4] * 0.25 for s in specs])
    return cur_t, dict(ids=ids, times=times, exact=exact, dist=dist), want_trunc


def check_imitation_edges(clib, J, n):
    """ss_imitation_step with a non-NULL cur_t (0 to 3) through test_motion_lib.check_imitation (observation 2e-4, reward and
    parts 2e-5, masked launch with a row stride), on envs placed by construction: on clips b, c, d, e and g; carrying the clip's
    own state (every reward part within 1e-5 of 1, not terminated: the zero-angle end of the atan2 form); with `time + obs_dt`
    4 and 64 float32 spacings either side of the clip length (flags exact); with every body at 0.8 and 1.25 times the
    termination distance (flags exact, no env excluded).  reward, reward_parts, terminated and truncated passed as NULL in turn
    leave the bits of the others, behind each output 3 guard rows stay untouched.  N below the number of specs: they are run in
    consecutive groups of N.

    Largest error / bound seen, emulator | MI355X:
      24 bodies, N in {1, 2, 9}: observation 1.1e-5 | 1.1e-5 / 2e-4; reward parts 1.5e-7 | 7.3e-8 / 2e-5; reward 1.4e-7 | 6.1e-8 / 2e-5
      52 bodies, N in {1, 5}:    observation 9.1e-5 | 9.1e-5 / 2e-4; reward parts 6.5e-8 | 4.3e-8 / 2e-5; reward 3.7e-8 | 4.5e-8 / 2e-5
      identity |part - 1|: 0 | 0 / 1e-5 (every part is 1.0f)
    """
    lib, _ = build_lib(J)
    device = "cpu" if lib.device.type == "cpu" else "cuda"
    specs = imitation_specs(lib, J)
    worst = dict(obs=0.0, parts=0.0, reward=0.0, identity=0.0)
    seen = set()
    for w0 in range(0, len(specs), n):
        win = [specs[(w0 + i) % len(specs)] for i in range(n)]
        cur_t, case, want_trunc = imitation_case(lib, win)
        r = T.check_imitation(lib, clib, np.random.default_rng(40 + w0), n=n, device=device, stream=lib._stream(), cur_t=cur_t, case=case)
        seen |= set(win)
        parts, term, trunc = r["parts"].cpu().numpy(), r["terminated"].cpu().numpy(), r["truncated"].cpu().numpy()
        assert np.array_equal(trunc.astype(bool), want_trunc)
        for i, (_, _, _, exact, fac) in enumerate(win):
            if exact:
                worst["identity"] = max(worst["identity"], np.abs(parts[i] - 1).max())
                assert np.abs(parts[i] - 1).max() < 1e-5 and term[i] == 0, (win[i], parts[i], term[i])
            elif fac is not None:
                assert term[i] == (1 if fac > 1 else 0), (win[i], term[i])
            else:
                assert term[i] == 0, win[i]
        for k in ("obs", "parts", "reward"):
            worst[k] = max(worst[k], r["err"][k])
        # optional outputs NULL in turn; sentinel-filled outputs with guard rows
        names = ("reward", "parts", "terminated", "truncated")
        full = {k: r[k].cpu().numpy() for k in names + ("obs",)}
        for skip in names:
            out = dict(obs=torch.full((n + GUARD, 24 * J), SENT, device=lib.device), reward=torch.full((n + GUARD,), SENT, device=lib.device),
                       parts=torch.full((n + GUARD, 4), SENT, device=lib.device), terminated=torch.full((n + GUARD,), 77, dtype=torch.uint8, device=lib.device),
                       truncated=torch.full((n + GUARD,), 77, dtype=torch.uint8, device=lib.device))
            arg = {k: (None if k == skip else out[k]) for k in names}
            r["launch"](_ptr(out["obs"]), 24 * J, arg["reward"], arg["parts"], arg["terminated"], arg["truncated"])
            for k, v in out.items():
                v = v.cpu().numpy()
                fill = 77 if v.dtype == np.uint8 else np.float32(SENT)
                assert (v[n:] == fill).all(), (skip, k)
                if k == skip:
                    assert (v == fill).all(), (skip, k)
                else:
                    assert np.array_equal(v[:n], full[k]), (skip, k)
    assert seen == set(specs)
    print(f"imitation J={J} N={n}:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    return worst
