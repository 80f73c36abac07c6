"""The cases of tests/dense_solve_cases.py take the paths of dense_solve (smplsim_amd/csrc/ss_kernel.h) they were chosen for — shown by
the kernel's own counters, not by the host's count of coupled bodies: the float64 wavefront emulator built with -DSS_PROFILE
(tests/wave_emu/Makefile libss_emu64_prof.so) runs every case alone through ss_debug_forward and ss_debug_prof returns, per case, the
solves (PF_N_DENSE), the solves in the shared block (PF_N_POOLED), the solves by tile rows (PF_N_T1 .. PF_N_T5, the last one = five or
more), the active contacts (PF_N_CONTACTS) and the unknowns (PF_N_UNKNOWNS), each summed over the Newton iterations.

Two runs per case.  Started on the oracle's converged acceleration, every iteration sees the active set of the solution: the kernel's
system must then be the host's, 3 size + 6 unknowns in every solve of every case.  Started from zero the early iterations may find fewer
active rows and couple fewer bodies, never more.

The fixture itself is checked here too: the seeded search reproduces the committed file byte for byte, and every stored case respects
the conditions under which the search keeps a state.  GPU twin: test_dense_solve_gpu.py; accuracy on the emulators: test_dense_solve_emu.py."""
import functools
import os
import re

import numpy as np
import pytest

import dense_solve_cases as DC
from helpers import FEET, model_const, pd_tables
from wave_emu import emu

KERNEL_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smplsim_amd", "csrc", "ss_kernel.h")
COUNTERS = ("PF_N_DENSE", "PF_N_POOLED", "PF_N_T1", "PF_N_T2", "PF_N_T3", "PF_N_T4", "PF_N_T5", "PF_N_CONTACTS", "PF_N_UNKNOWNS")


@functools.lru_cache(maxsize=None)
def counter_index():
    """{enumerator: index} of the kernel's counters (the enum of ss_kernel.h; it is not part of the public headers)."""
    with open(KERNEL_H) as f:
        body = re.search(r"enum \{ (PF_FWD = 0.*?PF_COUNT) \};", f.read(), re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",")]
    assert all(c in names for c in COUNTERS)
    return {n: i for i, n in enumerate(names)}


@functools.lru_cache(maxsize=None)
def counters(which, warm):
    """{counter: [cases] int array}: every case alone through ss_debug_forward on the profile build."""
    c, mc = DC.load(which), model_const(DC.HUMANOIDS[which])
    idx = counter_index()
    eb = emu.EmuBatch(mc, pd_tables(mc), 1, legal_bodies=FEET, f64=True, prof=True, self_collision=True)
    rows, prev = [], eb.prof()
    for i in range(len(c["size"])):
        eb.set_state(c["qpos"][i:i + 1], c["qvel"][i:i + 1], warm=c["warm"][i:i + 1] if warm else np.zeros((1, mc.nv)))
        qacc = eb.debug_forward(c["ctrl"][i:i + 1])[2]
        assert DC.rel_err(qacc, c["qacc"][i:i + 1])[0] < 1e-10 and eb.self_contacts[0] == c["nself"][i], (which, i)   # (the counters change no result)
        cur = eb.prof()
        rows.append((cur - prev).astype(np.int64)); prev = cur
    rows = np.array(rows)
    return {n: rows[:, idx[n]] for n in COUNTERS}


def test_path_arithmetic_of_the_cases_module():
    """dense_solve_cases.paths restates ss_hdr.h / dense_solve: where the shared block begins, which own-region size takes the staging
    fallback, the constants it rests on.  (hloc itself is not exported by the library: the counter tests below show its edge on real
    states — size 15 / 23 in the own region, 16 / 24 in the shared block, each with exactly the host's unknowns.)"""
    for which, humanoid in DC.HUMANOIDS.items():
        nb = model_const(humanoid).nbody
        assert nb == DC.NBODY[which]
        p = {nc: DC.paths(which, nc) for nc in range(1, nb)}
        assert min(nc for nc in p if p[nc]["pooled"]) == {"smpl": 16, "smplx": 24}[which]
        assert [nc for nc in p if p[nc]["fallback"] and not p[nc]["pooled"]] == {"smpl": [15], "smplx": []}[which]
        assert [nc for nc in p if p[nc]["Np"] % 16 == 0] == {"smpl": [3, 19], "smplx": [3, 19, 35, 51]}[which]
    with open(KERNEL_H) as f:
        assert "constexpr int kRec = %d;" % DC.K_REC in f.read()
    with open(os.path.join(os.path.dirname(KERNEL_H), "ss_hdr.h")) as f:
        hdr = f.read()
    assert "constexpr int kDenseExtra = 256;" in hdr and "constexpr int kDenseTile = 16;" in hdr


def test_the_generator_reproduces_the_committed_fixture():
    with open(DC.FIXTURE, "rb") as f:
        committed = f.read()
    assert len(committed) < 1 << 20
    assert DC.to_bytes(DC.build_all()) == committed


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
def test_stored_cases_respect_the_exclusions_and_fill_the_bins(which):
    """From the oracle again, per stored case: contacts between bodies (1 .. 60), no distance within 1e-4 of the margin or of zero, no
    solver warning, the stored counts, size and answers; float32-representable inputs; the bins' numbers and root heights."""
    import placement_cases as PC
    from helpers import oracle_model
    from oracle import oracle as O
    c, mc = DC.load(which), model_const(DC.HUMANOIDS[which])
    up = PC.elimination_parent(mc.body_parent, DC.TREE_ROOT[which])
    assert DC.TREE_ROOT[which] == PC.CROWDED[DC.HUMANOIDS[which]][0]
    d = O.OracleData(oracle_model(DC.HUMANOIDS[which], self_collision=True))
    n = len(c["size"])
    for f in ("qpos", "qvel", "ctrl"):
        assert c[f].dtype == np.float64 and np.array_equal(c[f], DC.f32(c[f]))
    for i in range(n):
        w0 = d.nwarn
        d.qpos = c["qpos"][i]; d.qvel = c["qvel"][i]; d.ctrl = c["ctrl"][i]; d.warm = np.zeros(mc.nv); d.forward()
        dist, self_ = d.con_dist, d.con_body1 >= 0
        assert 1 <= d.nself <= DC.MAX_NSELF and d.nself == c["nself"][i] and d.ncon - d.nself == c["nfloor"][i]
        assert np.abs(dist).min() >= DC.BORDERLINE and np.abs(dist - DC.MARGIN).min() >= DC.BORDERLINE
        assert d.nwarn == w0 and d.solver_iter < 100
        assert np.array_equal(d.qacc, c["qacc"][i])
        assert len(DC.coupled_set(d, up, self_)) == c["size"][i]                  # no contact outside the set, active or not
        assert len(PC.coupled_bodies(d, up)) <= c["size"][i]                      # (the penetrating ones: placement_cases' count)
        # the warm start is the same solution, converged further
        assert DC.rel_err(c["warm"][i:i + 1], c["qacc"][i:i + 1])[0] < 1e-6
    low = c["qpos"][:, 2] < 1.0
    assert 3 * low.sum() >= n and (c["nfloor"][low] > 0).all() and (c["nfloor"][~low] == 0).all()
    for name, lo, hi, n_hi, n_lo in DC.BINS[which]:
        got = c["bin"] == name
        assert ((c["size"][got] >= lo) & (c["size"][got] <= hi)).all()
        assert (got & ~low).sum() >= n_hi and (got & low).sum() >= n_lo and got.sum() >= (3 if which == "smpl" else 2), name
    assert (c["bin"] != None).all()                                               # noqa: E711  (every case belongs to a bin)


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
def test_started_on_the_solution_every_solve_has_the_hosts_size(which):
    """The run that begins on the final active set: the kernel's coupled set is the host's in every solve of every case, so the tile
    rows, the shared block and the staging capacity are those dense_solve_cases.paths derives from the size."""
    c, k = DC.load(which), counters(which, True)
    n = len(c["size"])
    assert (k["PF_N_DENSE"] >= 1).all()
    seen_rows = set()
    for i in range(n):
        p = DC.paths(which, int(c["size"][i]))
        dense = k["PF_N_DENSE"][i]
        assert k["PF_N_UNKNOWNS"][i] == p["N"] * dense, (i, c["bin"][i])
        assert k["PF_N_POOLED"][i] == (dense if p["pooled"] else 0), (i, c["bin"][i])
        assert k["PF_N_T%d" % min(p["tile_rows"], 5)][i] == dense, (i, c["bin"][i])
        assert k["PF_N_CONTACTS"][i] == c["nactive"][i] * dense, (i, c["bin"][i])
        seen_rows.add(min(p["tile_rows"], 5))
    assert seen_rows == ({1, 2, 3, 4, 5} if which == "smpl" else {2, 3, 5})
    # the full last tile row: N = 15 and 63 (SMPL), 111 (SMPL-X), in every solve of every case of those bins
    for name, N in {"smpl": (("3", 15), ("19", 63)), "smplx": (("35", 111),)}[which]:
        got = c["bin"] == name
        assert got.sum() >= (3 if which == "smpl" else 2) and (k["PF_N_UNKNOWNS"][got] == N * k["PF_N_DENSE"][got]).all()


@pytest.mark.parametrize("which", list(DC.HUMANOIDS))
def test_started_from_zero_the_bins_take_their_paths(which):
    """The run the product makes after a reset (zero warm start), several Newton iterations per case: no solve couples more bodies
    than the host counts; the shared block is taken in the bins meant to be pooled and in no other; every tile-row count is taken;
    enough tile-full states solve the full size in EVERY iteration; the staging fallback sees more contacts than it has records."""
    c, k = DC.load(which), counters(which, False)
    need = 3 if which == "smpl" else 2
    N = np.array([DC.paths(which, int(s))["N"] for s in c["size"]])
    pooled_bin = np.array([DC.paths(which, int(s))["pooled"] for s in c["size"]])
    assert (k["PF_N_DENSE"] >= 1).all() and (k["PF_N_UNKNOWNS"] <= N * k["PF_N_DENSE"]).all()
    assert (k["PF_N_POOLED"][~pooled_bin] == 0).all()                             # size 15 (SMPL) / 23 (SMPL-X) and below: the own region, always
    for name in sorted(set(c["bin"][pooled_bin])):
        got = c["bin"] == name
        assert (k["PF_N_POOLED"][got] > 0).all(), name                            # every state of a pooled bin takes the shared block
    for t in range(1, 6):
        if which == "smpl" or t in (2, 3, 5):
            assert (k["PF_N_T%d" % t] > 0).sum() >= need, t
    every = k["PF_N_UNKNOWNS"] == N * k["PF_N_DENSE"]                             # the host's size in every solve
    for name in {"smpl": ("3", "19"), "smplx": ("35",)}[which]:
        assert (every & (c["bin"] == name)).sum() >= need, name
    if which == "smpl":
        # size 15: the system leaves 64 reals of the own region, the records go to the gc fallback, 4 at a time
        p = DC.paths("smpl", 15)
        assert p["fallback"] and not p["pooled"] and p["records"] == 4
        rounds = every & (c["size"] == 15) & (k["PF_N_CONTACTS"] > 4 * k["PF_N_DENSE"])
        assert rounds.sum() >= 3
    else:
        # no SMPL-X size reaches the fallback of 8 records (dense_solve_cases); the own-region solve with the fewest records is
        # size 23: 4 records in what the system leaves, more contacts than that in rounds
        p = DC.paths("smplx", 23)
        assert not p["fallback"] and not p["pooled"] and p["records"] == 4
        rounds = every & (c["size"] == 23) & (k["PF_N_CONTACTS"] > 4 * k["PF_N_DENSE"])
        assert rounds.sum() >= 2
