"""The grid of a step launch (ss::launch_geometry in ss_hdr.h, what HipBackend::launch calls) through the emulator library's test
hook: it agrees with placement_cases.launch_shape, the arithmetic test_placement_gpu.py reasons with, on every launch geometry of
that test, and its three other branches — automatic spreading of a small batch, the cap at one resident set of workgroups, the
caller's max_workgroups on top of that cap — give the values written out below."""
import ctypes as C

import pytest

import placement_cases as PC
from wave_emu import emu

CUS, LDS = 256, 160 * 1024
FIXED, PER_ENV = 4096, 12288         # bytes of LDS per workgroup and per env: 12 envs fit a CU (4096 + 12 * 12288 = 151552 <= 163840), as SMPL's do


def geometry(nenv, cus, envs_per_wg, fixed_epw, max_wgs, lds=LDS, fixed=FIXED, per_env=PER_ENV):
    f = emu.lib().ss_emu_launch_geometry
    f.restype, f.argtypes = None, [C.c_int] * 5 + [C.c_long] * 3 + [C.POINTER(C.c_long)]
    out = (C.c_long * 3)()
    f(nenv, cus, envs_per_wg, fixed_epw, max_wgs, lds, fixed, per_env, out)
    return tuple(out)


@pytest.mark.parametrize("max_epw", [2, 7, 8, 12])
def test_hook_agrees_with_launch_shape_on_every_placement_geometry(max_epw):
    for leading in (0, 8):
        for name, epw, max_wgs, _, _ in PC.geometries(max_epw, leading):
            wgs, waves, lds = geometry(PC.N, CUS, max_epw, epw, max_wgs)
            if epw == 0:                                           # automatic launch of a small batch: placement() says one env per workgroup
                where = PC.placement(0, max_wgs, None)
                assert (wgs, waves) == (len({g for g, _ in where.values()}), 1 + max(w for _, w in where.values())) == (PC.N, 1), name
            else:
                assert (wgs, waves) == PC.launch_shape(epw, max_wgs), name
            assert lds == FIXED + waves * PER_ENV, name


def test_small_batches_are_spread_over_all_cus():
    # ceil(n / cus) < envs_per_wg: that many envs per workgroup instead, and the LDS bytes of that many
    assert geometry(1024, CUS, 12, 0, 0) == (256, 4, 4096 + 4 * 12288)
    assert geometry(100, CUS, 12, 0, 0) == (100, 1, 4096 + 12288)
    assert geometry(1, CUS, 12, 0, 0) == (1, 1, 4096 + 12288)
    assert geometry(2817, CUS, 12, 0, 0) == (235, 12, 151552)      # ceil(2817 / 256) = 12: not spread
    assert geometry(2816, CUS, 12, 0, 0) == (256, 11, 4096 + 11 * 12288)
    assert geometry(1024, CUS, 12, 12, 0) == (86, 12, 151552)      # a fixed envs_per_wg turns the spreading off


def test_workgroups_are_capped_at_one_resident_set():
    assert geometry(4096, CUS, 12, 0, 0) == (256, 12, 151552)      # ceil(4096 / 12) = 342 workgroups wanted, one of 151552 bytes fits a CU
    assert geometry(4096, 8, 12, 2, 0) == (40, 2, 28672)           # 163840 // 28672 = 5 workgroups per CU, 8 CUs
    assert geometry(100, 8, 1, 0, 0, per_env=200000) == (8, 1, 204096)   # more LDS than a CU has: counted as one per CU


def test_max_workgroups_applies_on_top_of_the_resident_cap():
    assert geometry(4096, 8, 12, 2, 64) == (40, 2, 28672)          # the cap is the smaller one
    assert geometry(4096, 8, 12, 2, 16) == (16, 2, 28672)
    assert geometry(4096, CUS, 12, 0, 100) == (100, 12, 151552)
