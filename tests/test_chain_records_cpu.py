"""The packed chain records of the forward pass (smplsim_amd/csrc/ss_tables.h chain_records, layout in ss_hdr.h): per node its depth
and, per level of the node tree, the node on its chain from the root, one byte each — entry for entry what the chainnode / ndepth tables hold,
the node itself behind its own depth, whole 16-byte units per node.  tests/chain_records_check.cpp prints both for the body trees
handed to it: the two humanoids, the trees of tests/test_synthetic_trees_emu.py (chains of 1, 2, 3 and 14 bodies, combs of 9 and 17
branches), a star (every body a child of the root) and a chain of 19 bodies (20 levels: two 16-byte units).  And the records'
LDS must not cost a resident env: 12 SMPL envs per CU, 7 SMPL-X, 8 SMPL with body-body contacts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import FEET, model_const, pd_tables
from smplsim_amd.mjcf import compile_mjcf
from smplsim_amd.mjcf_writer import table_to_mjcf
from test_synthetic_trees_emu import _chain, _comb

HERE = os.path.dirname(os.path.abspath(__file__))
TREES = {"smpl": lambda: model_const("smpl_humanoid").body_parent, "smplx": lambda: model_const("smplx_humanoid").body_parent,
         "chain1": lambda: compile_mjcf(table_to_mjcf(_chain(1))).body_parent, "chain2": lambda: compile_mjcf(table_to_mjcf(_chain(2))).body_parent,
         "chain3": lambda: compile_mjcf(table_to_mjcf(_chain(3))).body_parent, "chain14": lambda: compile_mjcf(table_to_mjcf(_chain(14))).body_parent,
         "comb9": lambda: compile_mjcf(table_to_mjcf(_comb(9))).body_parent, "comb17": lambda: compile_mjcf(table_to_mjcf(_comb(17))).body_parent,
         "star10": lambda: [-1] + [0] * 9, "chain19": lambda: list(range(-1, 18))}
UNITS = {"smpl": 1, "smplx": 1, "chain1": 1, "chain2": 1, "chain3": 1, "chain14": 1, "comb9": 1, "comb17": 1, "star10": 1, "chain19": 2}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_records") / "chain_records_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "chain_records_check.cpp")])
    parents = {name: [int(p) for p in f()] for name, f in TREES.items()}
    lines = subprocess.check_output([exe] + [",".join(map(str, p)) for p in parents.values()], text=True).splitlines()
    out = {}
    for (name, par), line in zip(parents.items(), lines):
        nlev, ndepth, chainnode, rec = (np.array(x.split(), dtype=np.int64) for x in line.split("|"))
        out[name] = (par, int(nlev[0]), ndepth, chainnode, rec.astype(np.uint32))
    return out


@pytest.mark.parametrize("name", sorted(TREES))
def test_records_hold_the_chain_tables_entry_for_entry(name, tables):
    par, nlev, ndepth, chainnode, rec = tables[name]
    nn = len(par) + 1
    assert len(ndepth) == nn and len(chainnode) == nn * nlev and nlev == 1 + ndepth.max()
    byte = rec.view(np.uint8).reshape(nn, -1)                  # lowest byte first
    assert byte.shape[1] % 16 == 0 and byte.shape[1] // 16 == UNITS[name] and byte.shape[1] - 16 < 1 + nlev <= byte.shape[1]
    # the chain tables themselves, from the parents: node 0, node 1, then the bodies from the root down
    for n in range(nn):
        chain, b = [], n - 1
        while b >= 0:
            chain.append(b + 1); b = par[b]
        chain = ([0] + chain[::-1]) if n else [0]
        assert ndepth[n] == len(chain) - 1 and list(chainnode[n * nlev:n * nlev + len(chain)]) == chain
        assert byte[n, 0] == ndepth[n]
        for k in range(byte.shape[1] - 1):
            assert byte[n, 1 + k] == (chainnode[n * nlev + k] if k <= ndepth[n] else n), (name, n, k)


def test_the_trees_are_the_shapes_they_are_there_for(tables):
    assert tables["chain19"][1] == 20 and set(tables["chain19"][2]) == set(range(20))          # a single chain
    assert tables["star10"][1] == 3 and list(tables["star10"][2]) == [0, 1] + [2] * 9          # a star
    assert tables["smpl"][1] == 10 and tables["smplx"][1] == 12                                # ss_hdr.h fixed_chain_levels


@pytest.mark.parametrize("humanoid,self_collision,envs", [("smpl_humanoid", False, 12), ("smplx_humanoid", False, 7), ("smpl_humanoid", True, 8)])
def test_resident_envs_per_cu_are_what_they_were(humanoid, self_collision, envs):
    from wave_emu import emu
    mc = model_const(humanoid)
    eb = emu.EmuBatch(mc, pd_tables(mc), 1, legal_bodies=FEET, self_collision=self_collision)
    epw, lds, regs = C.c_int32(), C.c_int32(), C.c_int32()
    eb._chk(eb.L.ss_launch_info(eb.batch, C.byref(epw), C.byref(lds), C.byref(regs)))
    print(humanoid, "self_collision", self_collision, "envs per workgroup", epw.value, "LDS bytes", lds.value)
    assert lds.value <= 160 * 1024
    # the emulator's backend has no launch bound (16 waves): what fits the CU's 160 KiB.  The device's bounds are 12 / 7 / 8 waves
    # (ss_env_kernel.h), so the LDS must hold at least that many env slices
    assert epw.value >= envs and (epw.value == envs or not self_collision)
