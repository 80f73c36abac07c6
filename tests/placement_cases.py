"""Inputs of the placement-invariance tests: where an env runs — which workgroup, which wavefront, which LDS slice, in which round of
the hand-out, behind which other env — is scheduling only and must not move a bit of any result.  test_placement_gpu.py steps the
same 37 envs under every launch geometry and hand-out order below and compares bytes with the automatic one-env-per-workgroup
launch; test_placement_cpu.py checks that these inputs are what the GPU test needs (so that it cannot pass vacuously).

N = 37 = 3·12 + 1 = 4·8 + 5 = 5·7 + 2: with one full workgroup of 12 (SMPL), 8 (body-body contacts) or 7 (SMPL-X) wavefronts every
wavefront steps at least three envs in a row in the same slice and the last round is ragged.

Everything here is seeded and built on the CPU; torch is imported inside the functions that need it.
"""
import functools
import math

import numpy as np

from helpers import default_qpos, model_const, oracle_model

N = 37
STEPS = 3
STANDING = (0.94, 0.93, 0.92)
DROPPED_Z = 0.60                 # root height of the dropped envs: floor contacts and joint limits, many Newton iterations
NAN_ROW, DIVERGING_ROW = 13, 22  # rows of the non-finite action and of the diverging start state (both handed out in a later round)
MIN_COUPLED, MAX_NSELF = 16, 40  # crowded poses: bodies in the coupled set (a solve whose ACTIVE contacts couple 16 bodies or more takes the
                                 # shared block: dense_floats(3 nc + 7) > hloc = 1856 reals; profiles/placement_invariance.txt), contacts at most
SMPL_TREE_ROOT = 10              # Spine: root of SMPL's elimination tree (ss_model_elimination_tree; checked in test_placement_cpu.py)


# ------------------------------------------------------------------------------------------------ launch geometries
def geometries(max_epw, leading=0, seed=5):
    """[(name, envs_per_wg, max_workgroups, order_kind, order)]: `order` is an int32 permutation of 0..N-1, None (natural order) or
    the string "device" (ss_schedule_longest_first writes it).  leading: rows 0..leading-1 stay in the first `leading` places of
    every explicit order, permuted among themselves (the crowded rows, which must all start in the first round)."""
    def order(kind):
        head, tail = np.arange(leading), np.arange(leading, N)
        if kind == "reversed":
            head, tail = head[::-1], tail[::-1]
        else:
            rs = np.random.default_rng(seed)
            head, tail = rs.permutation(head), rs.permutation(tail)
        return np.ascontiguousarray(np.concatenate([head, tail]), dtype=np.int32)
    return [("R", 0, 0, "none", None),                              # the reference: automatic = one env per workgroup, no loop
            ("a", 1, 1, "none", None),                              # one wavefront walks all envs through the counter
            ("b", max_epw, 1, "none", None),                        # one full workgroup, every wavefront loops
            ("c", max_epw, 1, "reversed", order("reversed")),       # the same through k.order
            ("d", 2, 3, "random", order("random")),                 # six wavefronts in three workgroups on the counter
            ("e", max_epw, 0, "longest_first", "device"),           # what production runs above 64 envs (here: a wavefront per env, full workgroups)
            ("e2", max_epw, 2, "longest_first", "device"),          # the same order through the counter: two workgroups, every wavefront loops
            ("f", 0, 0, "none", None)]                              # after a..e2 on the same batch: the automatic launch again


def launch_shape(epw, max_wgs, n=N):
    """(workgroups, wavefronts per workgroup) of a launch with a fixed envs_per_wg (HipBackend::launch)."""
    wgs = math.ceil(n / epw)
    if max_wgs > 0:
        wgs = min(wgs, max_wgs)
    return wgs, epw


def placement(epw, max_wgs, order, n=N):
    """{row: (workgroup, wavefront)} of the first round of a launch — static: the wavefront `w` of workgroup `g` starts with
    hand-out position w * workgroups + g; every later position comes from the device counter."""
    if epw == 0:
        return {r: (r, 0) for r in range(n)}                       # automatic launch of a small batch: one env per workgroup
    if isinstance(order, str):
        return {}
    wgs, waves = launch_shape(epw, max_wgs, n)
    out = {}
    for w in range(waves):
        for g in range(wgs):
            p = w * wgs + g
            if p < n:
                out[int(p if order is None else order[p])] = (g, w)
    return out


# ------------------------------------------------------------------------------------------------ states
def humanoid_states(humanoid="smpl_humanoid", seed=31):
    """N pre-step states and STEPS actions: mixed root heights (every fourth env dropped to DROPPED_Z), one env with a NaN in its
    first action, one env whose start state diverges inside the first control step (MuJoCo's bad-state reset: NaNs in its slice)."""
    mc = model_const(humanoid)
    rs = np.random.default_rng(seed)
    acts = rs.uniform(-0.5, 0.5, (STEPS, N, mc.nu))
    q = np.tile(default_qpos(mc.nq), (N, 1))                      # the Default reset's pose
    dropped = np.arange(N) % 4 == 3
    q[:, 2] = np.where(dropped, DROPPED_Z, np.asarray(STANDING)[np.arange(N) % 3])
    q[:, 7:] += rs.uniform(-0.1, 0.1, (N, mc.nq - 7))
    v = rs.normal(size=(N, mc.nv)) * 0.2
    v[DIVERGING_ROW, [3, 8, 20, 40]] *= 1e4
    acts[0, NAN_ROW, 5] = np.nan
    return dict(qpos=q, qvel=v, acts=acts, dropped=np.flatnonzero(dropped), nan_row=NAN_ROW, diverging_row=DIVERGING_ROW)


def elimination_parent(body_parent, root):
    """Neighbour towards `root` of every body of the body tree re-rooted at `root` (root: -1)."""
    nb = len(body_parent)
    adj = [[] for _ in range(nb)]
    for b in range(1, nb):
        adj[b].append(int(body_parent[b])); adj[int(body_parent[b])].append(b)
    up, todo = {root: -1}, [root]
    while todo:
        b = todo.pop()
        for c in adj[b]:
            if c not in up:
                up[c] = b; todo.append(c)
    return [up[b] for b in range(nb)]


def tree_centre(body_parent):
    """Centre of the body tree (the body with the smallest eccentricity; SMPL's is unique)."""
    nb = len(body_parent)
    ecc = []
    for r in range(nb):
        up = elimination_parent(body_parent, r)
        depth = lambda b: 0 if up[b] < 0 else 1 + depth(up[b])
        ecc.append(max(depth(b) for b in range(nb)))
    best = [r for r in range(nb) if ecc[r] == min(ecc)]
    assert len(best) == 1
    return best[0]


def coupled_bodies(d, up):
    """Bodies of the coupled set of the oracle state `d` after forward(): the union, over penetrating body-body contacts, of the
    bodies on the way from both contact bodies to the elimination tree's root (the root excluded)."""
    b1, b2, dist = d.con_body1, d.con_body, d.con_dist
    out = set()
    for i in range(d.ncon):
        if b1[i] >= 0 and dist[i] < 0:
            for b in (int(b1[i]), int(b2[i])):
                while up[b] >= 0:
                    out.add(b); b = up[b]
    return out


# crowded poses per humanoid: root of the elimination tree, range of the joint angles, fewest bodies in the coupled set.  SMPL-X: a solve
# is pooled from 24 coupled bodies on (dense_floats(3 nc + 7) > hloc = 3676 reals); 28 leaves room for contacts whose row is not active
CROWDED = {"smpl_humanoid": (SMPL_TREE_ROOT, 2.2, MIN_COUPLED), "smplx_humanoid": (11, 1.5, 28)}


@functools.lru_cache(maxsize=None)
def crowded_states(n_crowded=8, seed=9, max_tries=400, humanoid="smpl_humanoid"):
    """Folded poses whose coupled set is too large for an env's own dense region, so that the solve takes the workgroup's shared
    block and its lock.  Returns dict(qpos [n, nq], coupled [n], nself [n], tries)."""
    from oracle import oracle as O
    mc = model_const(humanoid)
    root, spread, min_coupled = CROWDED[humanoid]
    up = elimination_parent(mc.body_parent, root)
    d = O.OracleData(oracle_model(humanoid, self_collision=True))
    rs = np.random.default_rng(seed)
    Q, coupled, nself, tries = [], [], [], 0
    while len(Q) < n_crowded and tries < max_tries:
        tries += 1
        q = default_qpos(mc.nq); q[2] = 5.0; q[7:] = rs.uniform(-spread, spread, mc.nq - 7)
        d.qpos = q; d.qvel = np.zeros(mc.nv); d.ctrl = np.zeros(mc.nu); d.warm = np.zeros(mc.nv); d.forward()
        c = len(coupled_bodies(d, up))
        if c >= min_coupled and d.nself <= MAX_NSELF:
            Q.append(q); coupled.append(c); nself.append(d.nself)
    return dict(qpos=np.array(Q), coupled=np.array(coupled), nself=np.array(nself), tries=tries)


def crowded_case_states(n_crowded=8, seed=31, humanoid="smpl_humanoid"):
    """The crowded cases: rows 0..n_crowded-1 are crowded poses at rest, the others humanoid_states rows."""
    s = humanoid_states(humanoid, seed)
    cr = crowded_states(n_crowded, humanoid=humanoid)
    q, v = s["qpos"].copy(), s["qvel"].copy()
    q[:n_crowded] = cr["qpos"]; v[:n_crowded] = 0.0
    return dict(s, qpos=q, qvel=v, crowded=np.arange(n_crowded), nself=cr["nself"])


# ------------------------------------------------------------------------------------------------ comparison
STATE_FIELDS = ("qpos", "qvel", "qpos_prev", "qvel_prev", "qacc_warm", "body_vel", "touch", "cur_t", "task_state", "nwarn", "solver_iters",
                "self_contacts")
OUTPUT_FIELDS = ("obs_buf", "obs_final", "rew_buf", "terminated", "truncated")
IMITATION_FIELDS = ("times", "motion_ids", "start_times", "xpos", "xmat", "reward_parts")


def snapshot(env):
    """{field: [N, bytes per row] uint8 array} of everything a launch writes (the caller synchronises first).  An imitation env's
    snapshot holds the simulator state of its base batch, its own outputs and its clip bookkeeping."""
    base = getattr(env, "base", env)
    src = [(f, getattr(base, f)) for f in STATE_FIELDS] + [(f, getattr(env, f)) for f in OUTPUT_FIELDS]
    if base is not env:
        src += [(f, getattr(env, f)) for f in IMITATION_FIELDS]
    out = {}
    for name, t in src:
        a = t.detach().cpu().contiguous().numpy()
        out[name] = np.ascontiguousarray(a.reshape(a.shape[0], -1)).view(np.uint8).copy()
    return out


def compare(a, b, where=None, skip_rows=()):
    """Byte comparison of two snapshots (NaN equals NaN with the same payload).  Returns a list of mismatch reports, one line per
    field: the field, the rows that differ and, for each, where it ran — where[row] = (workgroup, wavefront) of the rows handed out
    statically (the first round, placement()); every other row came from the counter in a later round."""
    lines = []
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].shape == b[f].shape, f
        rows = [int(r) for r in np.flatnonzero((a[f] != b[f]).any(axis=1)) if int(r) not in skip_rows]
        if rows:
            def at(r):
                if where is None:
                    return "?"
                return "workgroup %d wave %d, first round" % where[r] if r in where else "later round"
            lines.append("%s: rows %s" % (f, ", ".join("%d (%s)" % (r, at(r)) for r in rows)))
    return lines


def differing_rows(a, b):
    """Rows in which any field of the two snapshots differs."""
    rows = set()
    for f in a:
        rows.update(int(r) for r in np.flatnonzero((a[f] != b[f]).any(axis=1)))
    return sorted(rows)
