"""What model creation makes (smplsim_amd/csrc/ss_tables.h and the creation entries of ss_api.h), byte for byte: the emulator library's
ss_emu_model_digests hook gives one 64-bit FNV-1a digest per uploaded table (read back through the backend), per header (field by
field) and for illegal_mask, meaninertia and the self_collision_unavailable text.  tests/golden/host_tables.json holds the digests the
commit named in it gave for the models below; that file is a record of that commit and is never rewritten from a later tree.  The
refusals at the end: one description per message, each failing one check, with the return code and the text."""
import contextlib
import ctypes as C
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

from helpers import FEET, GOLDEN, model_const, pd_tables
from smplsim_amd import _cabi
from smplsim_amd.mjcf import GEOM_SPHERE, compile_mjcf
from smplsim_amd.mjcf_writer import scaled_xml_str, table_to_mjcf
from test_synthetic_trees_emu import _body, _chain, _comb, _table
from wave_emu import emu

ITEMS = ("shared", "bodyc", "candc", "candb", "pairs_sctab", "geomc", "h", "h_sc", "hc", "sc", "illegal_mask", "meaninertia",
         "self_collision_unavailable")
SS_OK, SS_ERR_INVALID = 0, -1


@functools.lru_cache(maxsize=None)
def _synthetic(name):
    kind, n = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind == "fork":                                            # 4 bodies: B0 - B1 - B2 and B3 below B0
        bodies = [_body("B0", None, (0, 0, 0), box=True), _body("B1", "B0", (0.0, 0.02, -0.19)), _body("B2", "B1", (0.0, 0.02, -0.19)),
                  _body("B3", "B0", (0.1, 0.02, -0.19))]
        return compile_mjcf(table_to_mjcf(_table(bodies)))
    return compile_mjcf(table_to_mjcf(_chain(n) if kind == "chain" else _comb(n)))


def _flat_tables(mc):
    return (np.full(mc.nu, 60.0), np.full(mc.nu, 6.0), np.full(mc.nu, 40.0), np.full(mc.nu, 2.0), np.zeros(mc.nu))


def _synthetic_case(name, change=None):
    mc = _synthetic(name)
    if change:
        mc = change(mc)
    return [(mc, _flat_tables(mc), tuple(mc.body_names))]


def _humanoid_case(name):
    mc = model_const(name)
    return [(mc, pd_tables(mc), FEET)]


@functools.lru_cache(maxsize=None)
def _smpl_shapes():
    # geom sizes and body offsets scaled per shape (the three of test_edge_cases_emu's per-env body shapes)
    return tuple(compile_mjcf(x) for x in (scaled_xml_str("smpl_humanoid", 1.0), scaled_xml_str("smpl_humanoid", 0.9, {"L_Knee": 1.1, "R_Knee": 1.1}),
                                           scaled_xml_str("smpl_humanoid", 1.08, {"Chest": 0.9, "L_Elbow": 1.2})))


def _shapes_case():
    mcs = _smpl_shapes()
    return [(m, pd_tables(mcs[0]), FEET) for m in mcs]


def _sphere(mc):
    t = mc.geom_type.copy(); t[1] = GEOM_SPHERE
    return dataclasses.replace(mc, geom_type=t)


# name -> (shapes: a list of (ModelConst, actuator tables, legal bodies), environment of the creation call)
CASES = {
    "smpl": (lambda: _humanoid_case("smpl_humanoid"), {}),
    "smplx": (lambda: _humanoid_case("smplx_humanoid"), {}),                          # aliased LDS layout, lean tables
    "smplx_no_alias": (lambda: _humanoid_case("smplx_humanoid"), {"SS_NO_ALIAS_LAYOUT": "1"}),
    "chain15": (lambda: _synthetic_case("chain14"), {}),                              # the names of test_synthetic_trees_emu.py
    "comb9": (lambda: _synthetic_case("comb9"), {}),
    "comb17": (lambda: _synthetic_case("comb17"), {}),
    "tree1": (lambda: _synthetic_case("chain1"), {}),
    "tree2": (lambda: _synthetic_case("chain2"), {}),
    "tree3": (lambda: _synthetic_case("chain3"), {}),
    "sphere": (lambda: _synthetic_case("chain3", _sphere), {}),
    "chain19_deep": (lambda: _synthetic_case("chain19"), {}),                         # elimination tree of 9 levels: no body-body contacts
    "smpl_3_shapes": (_shapes_case, {}),
}


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def create(shapes, env=None):
    """ss_model_create for one shape, ss_model_create_shapes for several -> (return code, message, model handle or None)"""
    L = emu.lib()
    descs, keep = (_cabi.ModelDesc * len(shapes))(), []
    for i, (mc, tables, legal) in enumerate(shapes):
        descs[i], k = _cabi.make_model_desc(mc, *tables, legal_bodies=legal)
        keep.append(k)
    model = C.c_void_p()
    with _environment(env or {}):
        if len(shapes) == 1:
            rc = L.ss_model_create(C.byref(descs[0]), 0, C.byref(model))
        else:
            rc = L.ss_model_create_shapes(descs, len(shapes), 0, C.byref(model))
    return rc, L.ss_last_error().decode(), (model if rc == SS_OK else None)


def digests(name):
    shapes, env = CASES[name]
    rc, msg, model = create(shapes(), env)
    assert rc == SS_OK, msg
    L = emu.lib()
    L.ss_emu_model_digests.restype, L.ss_emu_model_digests.argtypes = None, [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * len(ITEMS))()
    L.ss_emu_model_digests(model, out)
    L.ss_model_destroy(model)
    return ["%016x" % x for x in out]


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(GOLDEN, "host_tables.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_tables_and_headers_are_the_recorded_ones(name):
    rec = _recorded()
    assert tuple(rec["items"]) == ITEMS and len(rec["commit"]) == 40
    got = dict(zip(ITEMS, digests(name)))
    assert got == dict(zip(ITEMS, rec["cases"][name]))


def test_the_cases_reach_the_branches_they_are_there_for():
    """The recorded digests tell the variants apart: the switch moves SMPL-X's layout and blob, the three reasons a model has no body-body
    contacts are three texts (and SMPL has none), a model of several shapes has its shape-dependent blob regions zeroed."""
    c = {n: dict(zip(ITEMS, d)) for n, d in _recorded()["cases"].items()}
    assert c["smplx"]["h"] != c["smplx_no_alias"]["h"] and c["smplx"]["shared"] != c["smplx_no_alias"]["shared"]
    assert c["smplx"]["h_sc"] != c["smplx"]["h"] and c["smplx_no_alias"]["h_sc"] == c["smplx_no_alias"]["h"]
    assert c["smplx"]["hc"] == c["smplx_no_alias"]["hc"]
    empty = c["smpl"]["self_collision_unavailable"]
    assert empty == "%016x" % 14695981039346656037 == c["comb9"]["self_collision_unavailable"]
    assert len({empty, c["tree1"]["self_collision_unavailable"], c["chain15"]["self_collision_unavailable"], c["chain19_deep"]["self_collision_unavailable"]}) == 4
    assert c["smpl_3_shapes"]["shared"] != c["smpl"]["shared"] and c["smpl_3_shapes"]["candb"] == c["smpl"]["candb"]
    assert c["sphere"]["candc"] != c["tree3"]["candc"] and c["sphere"]["candb"] == c["tree3"]["candb"]


def _with(**changes):
    """chain3 (the fork for body_parent: four bodies) with array entries or scalars changed: {field: {index: value} or value}"""
    def change(mc):
        out = {}
        for field, v in changes.items():
            if isinstance(v, dict):
                a = np.array(getattr(mc, field)).copy()
                for i, x in v.items():
                    a[i] = x
                v = a
            out[field] = v
        return dataclasses.replace(mc, **out)
    return change


REFUSALS = {
    "nbody_range": (lambda: _synthetic_case("chain3", _with(nbody=0)), "nbody must be in [1,63]"),
    "root": (lambda: _synthetic_case("chain3", _with(body_parent={0: 0})), "body 0 must be the root"),
    "parents_precede_children": (lambda: _synthetic_case("chain3", _with(body_parent={1: 1})), "parents must precede children"),
    "depth_first_order": (lambda: _synthetic_case("fork4", _with(body_parent={2: 0, 3: 1})), "bodies must be in depth-first order"),
    "free_joint_armature": (lambda: _synthetic_case("chain3", _with(dof_armature={4: 0.01})), "armature on the free joint is not supported"),
    "actuator_dof": (lambda: _synthetic_case("chain3", _with(actuator_dof={2: 5})), "bad actuator_dof"),
    "geom_type": (lambda: _synthetic_case("chain3", _with(geom_type={1: 5})), "unknown geom type"),
    "level_of_17_nodes": (lambda: _synthetic_case("comb18"), "more than 16 nodes in one tree level"),
    "impratio": (lambda: _synthetic_case("chain3", _with(impratio=2.0)), "impratio != 1 is not supported"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_has_its_code_and_its_message(name):
    shapes, text = REFUSALS[name]
    rc, msg, model = create(shapes())
    assert (rc, msg, model) == (SS_ERR_INVALID, text, None)


def _smpl_with_gain(factor):
    mcs = _smpl_shapes()
    tabs = pd_tables(mcs[0])
    t2 = [np.array(t, dtype=np.float64).copy() for t in tabs]
    t2[0][3] *= factor
    return [(mcs[0], tabs, FEET), (mcs[1], t2, FEET)]


def test_a_shape_that_differs_in_a_gain_is_refused():
    rc, msg, model = create(_smpl_with_gain(2.0))
    assert (rc, msg, model) == (SS_ERR_INVALID, "shape 1 differs from shape 0 in more than its geometry", None)
    rc, msg, model = create([(model_const("smpl_humanoid"), pd_tables(model_const("smpl_humanoid")), FEET), _synthetic_case("chain3")[0]])
    assert (rc, msg, model) == (SS_ERR_INVALID, "shape 1 differs from shape 0 in more than its geometry", None)
    rc, msg, model = create([_synthetic_case("chain3")[0], _synthetic_case("chain3", _with(impratio=2.0))[0]])
    assert (rc, msg, model) == (SS_ERR_INVALID, "shape 1: impratio != 1 is not supported", None)


def test_a_shape_that_differs_below_float_precision_is_accepted():
    # the shapes are compared as the float tables the device gets: 1 + 1e-12 rounds away
    rc, msg, model = create(_smpl_with_gain(1.0 + 1e-12))
    assert rc == SS_OK, msg
    emu.lib().ss_model_destroy(model)
