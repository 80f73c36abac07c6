"""Cases of the dense-solve tests: states whose body-body contacts couple a chosen number of bodies, so that every path of
dense_solve (smplsim_amd/csrc/ss_kernel.h) that the size of the system selects is taken by a state whose float64 answer is known.

With nc coupled bodies the system has N = 3 nc + 6 unknowns and Np = N + 1 rows in 16 x 16 tiles (ss_hdr.h dense_floats):

    tile rows          Nt = ceil(Np / 16): 1 (nc <= 3), 2 (<= 8), 3 (<= 13), 4 (<= 19), 5 (<= 24), ... 10 (SMPL-X, nc = 51)
    full last tile row Np = 16, 64, 112 (nc = 3, 19, 35): the only systems in which no lane of the last tile row lies behind row N
    shared block       dense_floats(Np) > hloc: SMPL (hloc 1856) from nc = 16 on, SMPL-X (hloc 3676) from nc = 24 on
    staging area       what the system leaves of the env's region, free = hloc - dense_floats(Np), when that holds four records of 36
                       reals; else the gc fallback of 6 nb / 36 records.  SMPL: nc = 14 leaves 256 reals (7 records), nc = 15 leaves 64:
                       the fallback, 4 records, is taken at nc = 15 only.  SMPL-X: nc = 23 leaves 156 reals = 4 records (still no
                       fallback) and nc = 24 is pooled: NO size reaches the fallback of 8 records; the own-region solve with the
                       fewest records is nc = 23, where more than 4 active contacts go in rounds.
    tree part          two lanes per body with nb <= 32 (SMPL), one otherwise (SMPL-X)

The bins below put states on both sides of every one of these edges.  `size` is the HOST's coupled-set size, taken from the oracle:
the bodies between the body-body contacts with a pushing row AT THE SOLUTION and the root of the elimination tree (the walk of
placement_cases.coupled_bodies), in states where every listed body-body contact, active or not, lies inside that set.  The kernel's own
set follows the contacts with an ACTIVE row in each Newton iteration: started on the solution it is the host's, started from zero it
can be smaller in some iterations and never larger; tests/test_dense_solve_cpu.py reads the kernel's counters to show which paths
the cases really take.

The search is seeded and uses the oracle only; tests/golden/make_dense_solve_cases.py writes its result to
tests/golden/dense_solve_cases.npz, which is all the GPU test reads.  Every stored qpos / qvel / ctrl is a float32 value held in
float64, so that the float32 kernel and the float64 oracle see the same state."""
import functools
import io
import os
import zipfile

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_solve_cases.npz")
HUMANOIDS = {"smpl": "smpl_humanoid", "smplx": "smplx_humanoid"}
TREE_ROOT = {"smpl": 10, "smplx": 11}          # root of the elimination tree (placement_cases.SMPL_TREE_ROOT, placement_cases.CROWDED)
HLOC = {"smpl": 1856, "smplx": 3676}           # reals of an env's own dense region (ss_hdr.h make_layout_sc; checked in test_dense_solve_cpu.py)
NBODY = {"smpl": 24, "smplx": 52}
MARGIN, BORDERLINE = 0.001, 1e-4                 # contact margin of the models; distances this close to the margin or to zero are left out
MAX_NSELF = 60                                   # the kernel keeps 64 body-body contacts per env
SPREADS, HEIGHTS = (0.5, 0.9, 1.5, 2.2), (5.0, 0.35)
K_REC = 36                                       # reals per staged contact record (ss_kernel.h dense_solve kRec)

# (name, smallest size, largest size, states with the root at 5 m, states with the root at 0.35 m)
BINS = {
    "smpl": [("2", 2, 2, 3, 2), ("3", 3, 3, 3, 2), ("4", 4, 4, 3, 2), ("8", 8, 8, 3, 2), ("9", 9, 9, 3, 2), ("13", 13, 13, 3, 2),
             ("14", 14, 14, 3, 2), ("15", 15, 15, 3, 2), ("16", 16, 16, 3, 2), ("19", 19, 19, 3, 2), ("20+", 20, 23, 3, 2)],
    "smplx": [("4", 4, 4, 2, 1), ("12", 12, 12, 2, 1), ("23", 23, 23, 2, 1), ("24", 24, 24, 2, 1), ("28+", 28, 34, 2, 1),
              ("35", 35, 35, 3, 2), ("40+", 40, 51, 2, 1)],
}
# SMPL states of size 15 (the own region's largest system: the gc staging fallback of 4 records) with at least this many
# body-body contacts active at the solution, on top of bin "15": more active contacts than records, staged in rounds
STAGING_MIN_CONTACTS, STAGING_STATES = 7, 3
SEED = {"smpl": 20261, "smplx": 20262}
MAX_TRIES = {"smpl": 60000, "smplx": 12000}
FIELDS = ("qpos", "qvel", "ctrl", "size", "nself", "nfloor", "nactive", "qacc", "warm")


def dense_floats(np_):
    """ss_hdr.h dense_floats: reals of a system of np_ matrix rows."""
    t = (np_ - 1) // 16
    return 256 * (t * (t + 1) // 2) + 16 * (t + 1) * (np_ - 16 * t)


def paths(which, nc):
    """What a solve over nc coupled bodies selects: dict(N, Np, tile_rows, pooled, records) — records = capacity of the staging area."""
    N = 3 * nc + 6
    hf, hloc = dense_floats(N + 1), HLOC[which]
    pooled = hf > hloc
    free = hloc if pooled else hloc - hf
    return dict(N=N, Np=N + 1, tile_rows=(N + 16) // 16, pooled=pooled, records=free // K_REC if free >= 4 * K_REC else (6 * NBODY[which]) // K_REC,
                fallback=free < 4 * K_REC)


def bin_of(which, size):
    for name, lo, hi, _, _ in BINS[which]:
        if lo <= size <= hi:
            return name
    return None


def coupled_set(d, up, which_contacts):
    """placement_cases.coupled_bodies over the contacts picked by the boolean array: the bodies between them and the tree's root."""
    b1, b2 = d.con_body1, d.con_body
    out = set()
    for i in np.flatnonzero(which_contacts):
        for b in (int(b1[i]), int(b2[i])):
            while up[b] >= 0:
                out.add(b); b = up[b]
    return out


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def search(which):
    """The seeded search: {field: array over the cases} of one humanoid, in bin order.  Oracle and placement_cases only."""
    import placement_cases as PC
    from helpers import default_qpos, model_const, oracle_model
    from oracle import oracle as O
    humanoid = HUMANOIDS[which]
    mc = model_const(humanoid)
    up = PC.elimination_parent(mc.body_parent, TREE_ROOT[which])
    d = O.OracleData(oracle_model(humanoid, self_collision=True))
    dc = O.OracleData(oracle_model(humanoid, self_collision=True, solver="converged"))
    rs = np.random.default_rng(SEED[which])
    want = {(name, z): n for name, _, _, hi_n, lo_n in BINS[which] for z, n in zip(HEIGHTS, (hi_n, lo_n))}
    if which == "smpl":
        want[("15 staging", None)] = STAGING_STATES
    found = {k: [] for k in want}
    zero = np.zeros(mc.nv)
    tries = 0
    while tries < MAX_TRIES[which] and any(len(found[k]) < want[k] for k in want):
        tries += 1
        spread, z = float(rs.choice(SPREADS)), float(rs.choice(HEIGHTS))
        q = default_qpos(mc.nq); q[2] = z; q[7:] = rs.uniform(-spread, spread, mc.nq - 7)
        q, v, t = f32(q), f32(rs.normal(size=mc.nv) * 0.5), f32(rs.normal(size=mc.nu) * 5)
        w0 = d.nwarn
        d.qpos = q; d.qvel = v; d.ctrl = t; d.warm = zero; d.forward()
        if not 1 <= d.nself <= MAX_NSELF:
            continue
        dist, self_ = d.con_dist, d.con_body1 >= 0
        if z == HEIGHTS[1] and self_.all():                                        # a state near the floor is kept for its floor contacts
            continue
        # the coupled set at the solution: the contacts with a pushing pyramid row (the rows behind the joint limits' are four per
        # contact, in contact order).  It has to be the set of ALL listed body-body contacts too, so that no Newton iteration,
        # whichever rows it finds active, can couple a body outside it
        force = d.get(O.D_EFC_FORCE)
        force = force[len(force) - 4 * d.ncon:].reshape(d.ncon, 4)
        active = self_ & (force > 0).any(axis=1)
        coupled = coupled_set(d, up, active)
        if coupled != coupled_set(d, up, self_):
            continue
        name = bin_of(which, len(coupled))
        if name is None:
            continue
        nactive = int(active.sum())
        key = (name, z)
        if len(found[key]) >= want[key]:
            key = ("15 staging", None)
            if which != "smpl" or name != "15" or nactive < STAGING_MIN_CONTACTS or len(found[key]) >= want[key]:
                continue
        if min(np.abs(dist).min(), np.abs(dist - MARGIN).min()) < BORDERLINE:      # float32 may count or activate otherwise
            continue
        qacc = d.qacc
        if d.nwarn != w0 or d.solver_iter >= 100 or not np.isfinite(qacc).all():   # the oracle's solver warnings
            continue
        w1 = dc.nwarn
        dc.qpos = q; dc.qvel = v; dc.ctrl = t; dc.warm = zero; dc.forward()
        warm = dc.qacc
        if dc.nwarn != w1 or not np.isfinite(warm).all():
            continue
        found[key].append(dict(qpos=q, qvel=v, ctrl=t, size=len(coupled), nself=d.nself, nfloor=d.ncon - d.nself, nactive=nactive, qacc=qacc, warm=warm))
    cases = [c for k in want for c in found[k]]
    out = {f: np.array([c[f] for c in cases], dtype=np.float64 if np.ndim(cases[0][f]) else np.int32) for f in FIELDS}
    out["tries"] = np.array([tries], np.int32)
    return out


def build_all():
    """{humanoid_field: array} of both humanoids: the fixture's content."""
    return {f"{which}_{f}": a for which in HUMANOIDS for f, a in search(which).items()}


def to_bytes(arrays):
    """An .npz file of `arrays` with nothing in it that depends on when or where it was written (stored, fixed time stamps)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue())
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def load(which):
    """The committed cases of one humanoid: {field: array}, plus `bin` (name per case)."""
    with np.load(FIXTURE) as f:
        out = {k[len(which) + 1:]: f[k] for k in f.files if k.startswith(which + "_")}
    out["bin"] = np.array([bin_of(which, s) for s in out["size"]])
    return out


def rel_err(qacc, ref):
    """Per case: max |qacc - ref| / max |ref|."""
    return np.abs(np.asarray(qacc, np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)
