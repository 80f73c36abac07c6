"""The Python bindings (smplsim_amd/_cabi.py, derived from the public headers by smplsim_amd/_cheader.py) held against a real C
front end: the clang that ships next to hipcc parses each header (-ast-dump=json) and the host C compiler builds a program that
prints every sizeof, offsetof and constant.  A missing compiler fails these tests; it does not skip them."""
import ctypes as C
import json
import os
import struct
import subprocess

import pytest

from smplsim_amd import _cabi, _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("smplsim_hip.h", "smplsim_motion.h", "smplsim_mlp.h")
CLANG = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "amdclang")
STRUCT_NAMES = {"ss_model_desc": "ModelDesc", "ss_env_cfg": "EnvCfg", "ss_state": "State", "ss_skeleton": "Skeleton", "ss_motion_data": "MotionData",
                "ss_motion_state": "MotionState", "ss_imitation_cfg": "ImitationCfg", "ss_imitation_io": "ImitationIO", "ss_mjcf_options": "MjcfOptions",
                "ss_adam_tensor": "AdamTensor", "ss_gather_tensor": "GatherTensor"}


def _walk(node):
    yield node
    for child in node.get("inner", []):
        yield from _walk(child)


class Clang:
    """What clang's AST says about the three headers: functions per header, records, typedefs, enumerators."""

    def __init__(self):
        self.functions, self.records, self.typedefs, self.enumerators = {}, {}, {}, set()
        for h in HEADERS:
            out = subprocess.run([CLANG, "-x", "c", "-fsyntax-only", "-Xclang", "-ast-dump=json", os.path.join(INCLUDE, h)], check=True,
                                 capture_output=True, text=True).stdout
            top = json.loads(out)["inner"]
            by_id = {n["id"]: n for n in top}
            self.functions[h] = {}
            for n in top:
                if n["kind"] == "FunctionDecl" and n["name"].startswith("ss_"):
                    ret = n["type"]["qualType"].split("(")[0].strip()
                    self.functions[h][n["name"]] = (ret, [p["type"]["qualType"] for p in n.get("inner", []) if p["kind"] == "ParmVarDecl"])
                elif n["kind"] == "TypedefDecl":
                    self.typedefs[n["name"]] = n["type"].get("desugaredQualType", n["type"]["qualType"])
                    rec = next((by_id.get(t["decl"]["id"]) for t in _walk(n) if "decl" in t), None)
                    if n["name"].startswith("ss_") and rec is not None and rec["kind"] == "RecordDecl" and rec.get("completeDefinition"):
                        assert rec.get("tagUsed") == "struct", n["name"]
                        self.records[n["name"]] = [(f["name"], f["type"]["qualType"]) for f in rec["inner"] if f["kind"] == "FieldDecl"]
                        assert not any(f.get("isBitfield") for f in rec["inner"]), n["name"]
            self.enumerators |= {n["name"] for n in _walk({"inner": top}) if n.get("kind") == "EnumConstantDecl"}

    def canonical(self, qual_type):
        """`const int32_t` -> `int`, `ss_state` -> `ss_state` (a record), `const float *` -> `const float *` (pointers: see pointee)."""
        t = qual_type.strip()
        if t.endswith("*"):
            return t
        t = " ".join(w for w in t.split() if w not in ("const", "struct"))
        while t in self.typedefs and t not in self.records:
            u = " ".join(w for w in self.typedefs[t].split() if w not in ("const", "struct"))
            if u == t:                                      # typedef struct ss_model ss_model: a handle
                break
            t = u
        return t

    @staticmethod
    def pointee(qual_type):
        t = qual_type.strip()[:-1].strip()
        return t[:-len("const")].strip() if t.endswith("const") and t[:-len("const")].strip().endswith("*") else t


@pytest.fixture(scope="module")
def clang():
    return Clang()


@pytest.fixture(scope="module")
def measured(clang, tmp_path_factory):
    """{key: int} printed by a C program built from the derived bindings: `sizeof S`, `offsetof S f`, `const NAME` and `typesize <C type>` for every
    type that occurs in a prototype or a field."""
    types = sorted({t for h in HEADERS for ret, ps in clang.functions[h].values() for t in [ret] + ps if t != "void"} |
                   {t.split("[")[0] for fields in clang.records.values() for _, t in fields})
    types = sorted(set(types) | {clang.pointee(t) for t in types if t.endswith("*") and clang.pointee(t).endswith("*")})
    lines =["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in HEADERS] + ["int main(void) {"]
    for cname, cls in _cabi.STRUCTS.items():
        lines.append(f'  printf("sizeof {cname}=%zu\\n", sizeof({cname}));')
        lines += [f'  printf("offsetof {cname} {f}=%zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'  printf("const {k}=%lld\\n", (long long)({k}));' for k in _cabi.CONSTANTS]
    lines += [f'  printf("typesize {t}=%zu\\n", sizeof({t}));' for t in types]
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("cabi")
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, str(d / "layout.c"), "-o", str(d / "layout")], check=True)
    out = subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.rsplit("=", 1) for line in out.splitlines())}


_INTEGERS = (C.c_int8, C.c_int16, C.c_int32, C.c_int64, C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64)    # c_int, c_long, c_size_t are aliases of these


def _agrees(clang, measured, qual_type, ct, where):
    """One C type against one ctypes class: same size, same integer / float / pointer category and signedness, c_char_p exactly for char
    pointers, POINTER(S) / S exactly for a record declared in the headers, and a ctypes POINTER's own pointee likewise."""
    t = clang.canonical(qual_type)
    if t == "void":
        assert ct is None, where
        return
    assert ct is not None and C.sizeof(ct) == measured["typesize " + qual_type.split("[")[0]] * (ct._length_ if hasattr(ct, "_length_") else 1), (where, qual_type, ct)
    if hasattr(ct, "_length_"):
        assert qual_type.endswith(f"[{ct._length_}]"), (where, qual_type, ct)
        return _agrees(clang, measured, qual_type.split("[")[0], ct._type_, where)
    assert "[" not in qual_type, (where, qual_type, ct)
    if t.endswith("*"):
        inner = clang.pointee(t)
        target = clang.canonical(inner)
        if target == "char":
            assert ct is C.c_char_p, (where, qual_type, ct)
        elif target in clang.records:
            assert ct is C.POINTER(_cabi.STRUCTS[target]), (where, qual_type, ct)
        elif issubclass(ct, C._Pointer):
            _agrees(clang, measured, inner, ct._type_, where)
        else:
            assert ct is C.c_void_p, (where, qual_type, ct)
    elif t in clang.records:
        assert ct is _cabi.STRUCTS[t], (where, qual_type, ct)
    elif t in ("float", "double"):
        assert ct is {"float": C.c_float, "double": C.c_double}[t], (where, qual_type, ct)
    else:
        assert set(t.split()) <= {"unsigned", "signed", "char", "short", "int", "long"}, (where, qual_type, t)
        assert ct in _INTEGERS and (ct(-1).value < 0) == ("unsigned" not in t.split()), (where, qual_type, ct)


def test_prototypes_match_clangs_reading_of_each_header(clang, measured):
    assert sum(len(clang.functions[h]) for h in HEADERS) == 62 and len(clang.functions["smplsim_mlp.h"]) == 24
    for h in HEADERS:
        assert set(_cabi.PROTOTYPES[h]) == set(clang.functions[h]), set(_cabi.PROTOTYPES[h]) ^ set(clang.functions[h])
        for name, (ret, params) in clang.functions[h].items():
            restype, argtypes = _cabi.PROTOTYPES[h][name]
            assert len(argtypes) == len(params), name
            for i, (p, a) in enumerate(zip(params, argtypes)):
                _agrees(clang, measured, p, a, f"{name} parameter {i}")
            _agrees(clang, measured, ret, restype, f"{name} result")
    assert _cabi.EXPORTS == list(clang.functions["smplsim_hip.h"]) + list(clang.functions["smplsim_motion.h"])
    assert _cabi.MLP_EXPORTS == list(clang.functions["smplsim_mlp.h"])

    class Recorder:                                         # bind / bind_mlp attach exactly these tables
        def __getattr__(self, name):
            self.__dict__[name] = type("F", (), {})()
            return self.__dict__[name]
    r, m = _cabi.bind(Recorder()), _cabi.bind_mlp(Recorder())
    assert list(vars(r)) == _cabi.EXPORTS and list(vars(m)) == _cabi.MLP_EXPORTS
    for h, rec in (("smplsim_hip.h", r), ("smplsim_motion.h", r), ("smplsim_mlp.h", m)):
        for name, (restype, argtypes) in _cabi.PROTOTYPES[h].items():
            assert getattr(rec, name).restype is restype and getattr(rec, name).argtypes == argtypes, name


def test_struct_layouts_match_the_compiler(clang, measured):
    assert {c: cls.__name__ for c, cls in _cabi.STRUCTS.items()} == STRUCT_NAMES
    assert set(clang.records) == set(STRUCT_NAMES)
    for cname, cls in _cabi.STRUCTS.items():
        assert getattr(_cabi, cls.__name__) is cls and issubclass(cls, C.Structure)
        assert [f for f, _ in cls._fields_] == [f for f, _ in clang.records[cname]], cname          # names and order: clang's FieldDecls
        assert C.sizeof(cls) == measured[f"sizeof {cname}"], cname
        for (f, ct), (_, qual_type) in zip(cls._fields_, clang.records[cname]):
            assert getattr(cls, f).offset == measured[f"offsetof {cname} {f}"], (cname, f)
            _agrees(clang, measured, qual_type, ct, f"{cname}.{f}")
    assert _cabi.MOTION_DATA_ARRAYS == tuple(f for f, t in clang.records["ss_motion_data"] if t.endswith("*")) and len(_cabi.MOTION_DATA_ARRAYS) == 17
    assert _cabi.MOTION_STATE_FIELDS == tuple(f for f, _ in clang.records["ss_motion_state"]) and len(_cabi.MOTION_STATE_FIELDS) == 12


def test_constants_match_the_compiler(clang, measured):
    assert clang.enumerators <= set(_cabi.CONSTANTS), clang.enumerators - set(_cabi.CONSTANTS)
    for k, v in _cabi.CONSTANTS.items():
        assert measured[f"const {k}"] == v, k
    for k in ("SS_MAX_SELF_CONTACTS_N", "SS_NORM_BLOCK_ROWS", "SS_EPISODE_MAX_PARTS"):                 # the defines: not in the AST
        assert k in _cabi.CONSTANTS and k not in clang.enumerators
    K = _cabi.CONSTANTS
    assert (_cabi.TASK_BASE, _cabi.TASK_SPEED, _cabi.TASK_GETUP, _cabi.TASK_REACH) == tuple(K["SS_TASK_" + n] for n in ("BASE", "SPEED", "GETUP", "REACH"))
    assert (_cabi.INIT_DEFAULT, _cabi.INIT_FALL, _cabi.INIT_EXTERNAL) == tuple(K["SS_INIT_" + n] for n in ("DEFAULT", "FALL", "EXTERNAL"))
    assert _cabi.CONTROL_MODES == {n.lower(): K["SS_CTRL_" + n] for n in ("UHC_PD", "PD", "TORQUE", "SIMPLE_PID", "DEFAULT")}
    assert _cabi.TASKS == {"HumanoidEnv": K["SS_TASK_BASE"], "HumanoidSpeed": K["SS_TASK_SPEED"], "HumanoidGetup": K["SS_TASK_GETUP"], "HumanoidReach": K["SS_TASK_REACH"]}
    assert _cabi.STATE_INITS == {"Default": K["SS_INIT_DEFAULT"], "Fall": K["SS_INIT_FALL"], "External": K["SS_INIT_EXTERNAL"]}
    assert _cabi.FIELDS == {k[len("SS_FIELD_"):].lower(): v for k, v in K.items() if k.startswith("SS_FIELD_")} and len(_cabi.FIELDS) == 9
    assert _cabi.ACTIVATIONS == {"none": K["SS_ACT_NONE"], "silu": K["SS_ACT_SILU"], "tanh": K["SS_ACT_TANH"], "relu": K["SS_ACT_RELU"]}
    assert _cabi.SS_MAX_SELF_CONTACTS == K["SS_MAX_SELF_CONTACTS"] == 64 and _cabi.NORM_BLOCK_ROWS == K["SS_NORM_BLOCK_ROWS"]
    assert _cabi.EPISODE_MAX_PARTS == K["SS_EPISODE_MAX_PARTS"]
    assert [K["SS_EP_" + n.upper()] for n in _cabi.EPISODE_STATS] == list(range(K["SS_EP_PARTS"]))
    assert [K["SS_CLIP_" + n.upper()] for n in _cabi.CLIP_COLUMNS] == list(range(K["SS_CLIP_COLUMNS"])) and _cabi.CLIP_COLUMNS == ("failed", "completed", "steps")


def test_every_derived_name_resolves_in_the_built_library():
    import torch  # noqa: F401  (always before the library: one HIP runtime per process)
    from smplsim_amd import _lib
    lib = C.CDLL(_lib.build())
    assert len(_cabi.EXPORTS) == 38 and len(_cabi.MLP_EXPORTS) == 24
    for name in _cabi.EXPORTS + _cabi.MLP_EXPORTS:
        assert getattr(lib, name) is not None
    lib.ss_last_error.restype = C.c_char_p
    assert lib.ss_last_error() is not None


FORMS = """
/* every declarator form of the public headers */
#ifndef FORMS_H
#define FORMS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef enum { F_OK = 0, F_BAD = -1 } f_status;
enum { F_A, F_B = 4, F_C };   // implicit values count up
#ifndef F_LANES_N
#define F_LANES_N 64
#endif
enum { F_LANES = F_LANES_N };
#define F_ROWS 0x100
struct f_batch;
typedef struct f_model f_model;
typedef struct { float k, w; } f_cfg;
typedef struct f_desc {
  int32_t n; const double *kp, *kd, *lim;
  double timestep, gravity, solref[2], solimp[5], margin;
  float lo, hi; int32_t a, b;
  f_cfg cfg;
  const f_cfg *shared;
  const char *const *names;
  void *w, *wt;
} f_desc;
int f_create(const f_desc *desc, int device, f_model **out);
void f_destroy(f_model *m);
const char *f_last_error(void);
int64_t f_workspace(int32_t M,
                    size_t bytes);
int f_bind(struct f_batch *b, const uint8_t *mask, unsigned long long *ticks, char *buf, float gamma,
           double lr, void *stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_parses_every_declarator_form():
    h = _cheader.parse(FORMS, "forms.h")
    assert h.constants == {"F_OK": 0, "F_BAD": -1, "F_A": 0, "F_B": 4, "F_C": 5, "F_LANES_N": 64, "F_LANES": 64, "F_ROWS": 256}
    assert h.opaque == ["f_batch", "f_model"]
    assert h.structs == {
        "f_cfg": [("k", "float"), ("w", "float")],
        "f_desc": [("n", "int32_t"), ("kp", "const double *"), ("kd", "const double *"), ("lim", "const double *"), ("timestep", "double"),
                   ("gravity", "double"), ("solref", "double[2]"), ("solimp", "double[5]"), ("margin", "double"), ("lo", "float"), ("hi", "float"),
                   ("a", "int32_t"), ("b", "int32_t"), ("cfg", "f_cfg"), ("shared", "const f_cfg *"), ("names", "const char *const *"),
                   ("w", "void *"), ("wt", "void *")]}
    assert h.functions == {
        "f_create": ("int", ["const f_desc *", "int", "f_model **"]),
        "f_destroy": ("void", ["f_model *"]),
        "f_last_error": ("const char *", []),
        "f_workspace": ("int64_t", ["int32_t", "size_t"]),
        "f_bind": ("int", ["struct f_batch *", "const uint8_t *", "unsigned long long *", "char *", "float", "double", "void *"])}
    assert list(h.structs) == ["f_cfg", "f_desc"] and list(h.functions) == ["f_create", "f_destroy", "f_last_error", "f_workspace", "f_bind"]


@pytest.mark.parametrize("text, offending", [
    ("int f_walk(void (*visit)(int), void *stream);", "(*visit)(int)"),                          # function-pointer parameter
    ("typedef struct { int32_t ready : 1; int32_t n; } f_flags;", "ready : 1"),                    # bit-field
    ("typedef union { int32_t i; float f; } f_word;", "union"),                                    # union
    ("typedef struct { int32_t n; union { int32_t i; float f; } u; } f_mixed;", "union"),
    ("int f_step(f_batch *b, void *stream);", "f_batch *b"),                                       # unknown typedef name
    ("int f_step(int32_t n, __fp16 *x);", "__fp16 *x"),                                            # unknown scalar type
    ("typedef struct {\n  int32_t n;\n#if F_WIDE\n  int64_t big;\n#endif\n} f_s;", "#if F_WIDE"),   # conditional inside a struct
    ("#ifdef F_EXTRA\nint f_extra(void);\n#endif", "#ifdef F_EXTRA"),                              # conditional around a prototype
    ("int f_one(int32_t n)\nint f_two(void);", "int f_one(int32_t n)"),                            # closing ';' missing
    ("int f_two(void);\nint f_last(int32_t n)", "int f_last(int32_t n)"),
    ("#define F_SCALE 1.5", "F_SCALE"),                                                            # not an integer
    ("#define F_MAX(a, b) 3", "F_MAX(a, b)"),                                                      # function-like macro
    ("enum { F_X = 1 << 3 };", "1 << 3"),                                                          # an expression
    ("int f_unnamed(int32_t, void *stream);", "int32_t"),                                          # unnamed parameter
    ("typedef struct { void x; } f_v;", "void x"),
])
def test_reader_refuses_what_it_does_not_understand(text, offending):
    with pytest.raises(_cheader.HeaderError) as e:
        _cheader.parse("#include <stdint.h>\n" + text + "\n", "bad.h")
    assert "bad.h" in str(e.value) and offending in str(e.value), str(e.value)


def test_env_cfg_by_keyword_fills_the_bytes_of_the_positional_form():
    cfg = _cabi.make_env_cfg(task=_cabi.TASK_REACH, state_init=_cabi.INIT_FALL, self_obs_v=2, control_mode=_cabi.CTRL_SIMPLE_PID, episode_length=77,
                             control_freq_inv=5, root_height_obs=False, power_scale=0.75, tar_speed=(0.5, 3.5), speed_change=(11, 23), tar_height=(0.25, 1.5),
                             height_change=(31, 47), recovery_steps=9, newton_iters=13, tar_dist_max=2.5, reach_body=17, self_collision=True, solver_tolerance=1e-6)
    # ss_env_cfg in the order of the header: task, state_init, self_obs_v, control_mode, episode_length, control_freq_inv, root_height_obs, power_scale,
    # tar_speed_min / max, speed_change_min / max, tar_height_min / max, height_change_min / max, recovery_steps, newton_iters, tar_dist_max, reach_body,
    # self_collision, solver_tolerance
    assert bytes(cfg) == struct.pack("<7if2f2i2f4ifiif", 3, 1, 2, 3, 77, 5, 0, 0.75, 0.5, 3.5, 11, 23, 0.25, 1.5, 31, 47, 9, 13, 2.5, 17, 1, 1e-6)
    assert bytes(_cabi.make_env_cfg()) == struct.pack("<7if2f2i2f4ifiif", 0, 0, 1, 0, 300, 15, 1, 1.0, 0.0, 5.0, 100, 200, 0.5, 1.2, 100, 200, 60, 0, 1.0, 0, 0, 0.0)


def test_vec_env_state_by_keyword_fills_the_bytes_of_the_positional_form(emu_backend, monkeypatch):
    from smplsim_amd.batch import SMPLSimVecEnv
    seen, create = [], emu_backend.ss_batch_create
    monkeypatch.setattr(emu_backend, "ss_batch_create", lambda m, cfg, st, out: seen.append(bytes(st._obj)) or create(m, cfg, st, out))
    env = SMPLSimVecEnv(3, task="HumanoidSpeed", seed=1)
    # ss_state in the order of the header: num_envs, then sixteen pointers (shape_id NULL: a single-shape model)
    order = (env.qpos, env.qvel, env.qpos_prev, env.qvel_prev, env.qacc_warm, env.body_vel, env.touch, env.cur_t, env.task_state, env.nwarn,
             env.solver_iters, env.pid_integral, env.pid_last_error, env.pid_started, None, env.self_contacts)
    assert seen == [struct.pack("<i4x16Q", 3, *[0 if t is None else t.data_ptr() for t in order])]
    assert len({t.data_ptr() for t in order if t is not None}) == 15
