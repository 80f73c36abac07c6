"""The inputs of test_placement_gpu.py (placement_cases.py) are what that test needs: crowded poses whose coupled set takes the
workgroup's shared dense block, humanoid rows with floor contacts, one non-finite action and one diverging env, launch geometries
that really put several envs on one wavefront, and a comparison that sees one flipped bit.  Runs on the CPU: the oracle and the
wavefront emulator."""
import ctypes as C
import math

import numpy as np
import pytest

import placement_cases as PC
from helpers import FEET, model_const, oracle_model, pd_tables
from oracle import oracle as O
from wave_emu import emu


@pytest.mark.parametrize("humanoid,min_coupled", [("smpl_humanoid", 16), ("smplx_humanoid", 28)])
def test_crowded_poses_need_the_shared_block(humanoid, min_coupled):
    cr = PC.crowded_states(humanoid=humanoid)
    mc = model_const(humanoid)
    print(humanoid, "coupled bodies", cr["coupled"].tolist(), "body-body contacts", cr["nself"].tolist(), "tries", cr["tries"])
    assert len(cr["qpos"]) == 8 and cr["tries"] <= 400
    assert (cr["coupled"] >= min_coupled).all() and (cr["nself"] >= 9).all() and (cr["nself"] <= 40).all()
    # the oracle's first control step from each pose raises no solver warning
    d = O.OracleData(oracle_model(humanoid, self_collision=True))
    for q in cr["qpos"]:
        d.qpos = q; d.qvel = np.zeros(mc.nv); d.warm = np.zeros(mc.nv); d.forward()
        for _ in range(15):
            d.ctrl = d.spd_torque(np.zeros(mc.nu)); d.step()
        assert d.nwarn == 0


@pytest.mark.parametrize("humanoid", ["smpl_humanoid", "smplx_humanoid"])
def test_host_count_of_the_crowded_poses_is_the_kernels(humanoid):
    """The elimination tree's root the host count walks to is the library's, and the float64 kernel on the emulator counts the
    oracle's body-body contacts in every crowded pose."""
    mc = model_const(humanoid)
    cr = PC.crowded_states(humanoid=humanoid)
    want = PC.CROWDED[humanoid][0]
    assert PC.tree_centre(mc.body_parent) == want and mc.body_names[want] == {"smpl_humanoid": "Spine", "smplx_humanoid": "Chest"}[humanoid]
    eb = emu.EmuBatch(mc, pd_tables(mc), len(cr["qpos"]), legal_bodies=FEET, f64=True, self_collision=True)
    root = C.c_int32(-1)
    eb._chk(eb.L.ss_model_elimination_tree(eb.model, C.byref(root), None, None, None, None))
    assert root.value == want
    eb.set_state(cr["qpos"], np.zeros((len(cr["qpos"]), mc.nv)))
    eb.debug_forward(np.zeros((len(cr["qpos"]), mc.nu)))
    assert eb.self_contacts.tolist() == cr["nself"].tolist()


@pytest.mark.parametrize("humanoid,rows", [("smpl_humanoid", PC.N), ("smplx_humanoid", PC.N)])
def test_humanoid_states_cover_contacts_and_the_bad_state_reset(humanoid, rows):
    s = PC.humanoid_states(humanoid)
    mc = model_const(humanoid)
    assert s["qpos"].shape == (PC.N, mc.nq) and s["qvel"].shape == (PC.N, mc.nv) and s["acts"].shape == (PC.STEPS, PC.N, mc.nu)
    assert len(s["dropped"]) >= 8 and np.allclose(s["qpos"][s["dropped"], 2], PC.DROPPED_Z)
    bad = ~np.isfinite(s["acts"])
    assert bad.sum() == 1 and bad[0, s["nan_row"]].sum() == 1
    assert np.abs(s["qvel"][s["diverging_row"]]).max() > 100 * np.abs(np.delete(s["qvel"], s["diverging_row"], 0)).max()
    assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
    again = PC.humanoid_states(humanoid)
    assert all(np.array_equal(s[k], again[k], equal_nan=True) for k in ("qpos", "qvel", "acts"))
    # one control step on the emulator: the two special envs hit the bad-state reset, the others (almost all) do not
    eb = emu.EmuBatch(mc, pd_tables(mc), rows, legal_bodies=FEET)
    eb.set_state(s["qpos"][:rows], s["qvel"][:rows])
    eb.step(s["acts"][0, :rows])
    special = [s["nan_row"], s["diverging_row"]]
    print(humanoid, "nwarn", eb.nwarn.tolist(), "Newton iterations", eb.solver_iters.tolist())
    assert (eb.nwarn[special] > 0).all()
    assert (np.delete(eb.nwarn, special) == 0).sum() >= 30
    assert (eb.touch != 0).any(axis=1).any() and not (eb.touch != 0).any(axis=1).all()


@pytest.mark.parametrize("max_epw", [2, 7, 8, 12])
def test_geometries_are_valid_and_share_wavefronts(max_epw):
    names = []
    for leading in (0, 8):
        for name, epw, max_wgs, kind, order in PC.geometries(max_epw, leading):
            names.append(name)
            assert 0 <= epw <= max_epw and max_wgs >= 0
            if isinstance(order, np.ndarray):
                assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(PC.N))
                assert sorted(order[:leading].tolist()) == list(range(leading))
                assert order.tolist() != list(range(PC.N))
            else:
                assert order is None or (order == "device" and kind == "longest_first")
            if name in ("R", "f"):
                assert (epw, max_wgs, order) == (0, 0, None)
                continue
            waves = min(math.ceil(PC.N / epw), max_wgs or math.inf) * epw
            assert PC.launch_shape(epw, max_wgs) == (waves // epw, epw)
            if name == "e":                                        # (max, 0) as production sets it: full workgroups, a wavefront per env, the last workgroup ragged
                assert (epw, max_wgs) == (max_epw, 0) and PC.N <= waves < PC.N + epw and PC.N % epw != 0
                continue
            assert waves < PC.N                                    # every other entry makes wavefronts step several envs in a row
            first = PC.placement(epw, max_wgs, order)
            if order is None or isinstance(order, np.ndarray):
                assert len(first) == waves and len(set(first.values())) == waves
                if leading and waves >= leading:                   # the crowded rows all start in the first round
                    assert all(r in first for r in range(leading))
    assert names == ["R", "a", "b", "c", "d", "e", "e2", "f"] * 2
    b = PC.placement(max_epw, 1, None)
    assert b == {w: (0, w) for w in range(max_epw)}               # one workgroup: wavefront w starts with env w
    d = PC.placement(2, 3, None)
    assert d == {0: (0, 0), 1: (1, 0), 2: (2, 0), 3: (0, 1), 4: (1, 1), 5: (2, 1)}


def test_compare_sees_one_bit_and_names_the_row():
    rs = np.random.default_rng(0)
    a = {"qpos": rs.normal(size=(PC.N, 76)).astype(np.float32).view(np.uint8).copy(), "touch": rs.integers(0, 9, (PC.N, 2)).astype(np.int32).view(np.uint8).copy(),
         "rew_buf": np.full((PC.N, 1), np.nan, np.float32).view(np.uint8).copy()}
    b = {k: v.copy() for k, v in a.items()}
    assert PC.compare(a, b) == [] and PC.differing_rows(a, b) == []
    b["qpos"][20, 17] ^= 1                                         # one mantissa bit of one number of row 20
    where = PC.placement(12, 1, None)
    msg = PC.compare(a, b, where)
    assert msg == ["qpos: rows 20 (later round)"] and PC.differing_rows(a, b) == [20]
    b["rew_buf"][5, 0] ^= 1                                        # another NaN payload
    msg = PC.compare(a, b, where)
    assert msg == ["qpos: rows 20 (later round)", "rew_buf: rows 5 (workgroup 0 wave 5, first round)"]
    assert PC.compare(a, b, where, skip_rows=(5, 20)) == []
