"""CPU-side checks of the drop-in boundary: the binding read from include/fragnet_hip.h lays structs out as the C compiler does
and refuses header text it does not know; the shared library loads and exports exactly the entry points the header declares;
CPU tensors are refused (no fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from tests.conftest import ROOT

HEADER_PATH = os.path.join(ROOT, "include", "fragnet_hip.h")


def _declared():
    from fragnet_amd import _lib
    return sorted(_lib.HEADER.functions)


def test_struct_layouts_match_the_compilers(tmp_path):
    """The reader against the C++ compiler's own reading of the same file: a host-only probe prints sizeof of every struct and
    offsetof / sizeof of every field."""
    from fragnet_amd import _lib, build
    structs = _lib.HEADER.structs
    assert len(structs) >= 19
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "fragnet_hip.h"', "int main() {"]
    for name, cls in structs.items():
        lines.append(f'    std::printf("{name} %zu\\n", sizeof({name}));')
        for field, *_ in cls._fields_:
            lines.append(f'    std::printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    lines += ["    return 0;", "}", ""]
    (tmp_path / "layout_probe.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout_probe")
    subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.dirname(HEADER_PATH), str(tmp_path / "layout_probe.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = []
    for name, cls in structs.items():
        want.append(f"{name} {C.sizeof(cls)}")
        want += [f"{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}" for field, *_ in cls._fields_]
    assert len(got) == len(want) >= 19 + 200
    for g, w in zip(got, want):
        assert g == w, f"compiler: {g}; binding: {w}"
    for name, cls in structs.items():
        assert getattr(_lib, _lib.camel(name)) is cls


def test_signatures_have_the_declared_arity_and_scalar_widths():
    """An independent reading of every prototype: the number of arguments, and the width of each one passed by value."""
    from fragnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    width = {"int": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8, "float": 4, "double": 8, "fn_stream_t": 8}
    protos = re.findall(r"\b(fn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert sorted(n for n, _ in protos) == _declared() and len(protos) >= 113
    for name, args in protos:
        args = [] if args.strip() == "void" else [a.split() for a in args.split(",")]
        argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(args), f"{name}: {len(args)} declared, {len(argtypes)} bound"
        for words, t in zip(args, argtypes):
            if "*" in " ".join(words):
                assert C.sizeof(t) == C.sizeof(C.c_void_p), (name, words)
                assert t is C.c_void_p or hasattr(t, "contents"), (name, words)
            else:
                assert C.sizeof(t) == width[words[-2]], (name, words)
                assert (t in (C.c_float, C.c_double)) == (words[-2] in ("float", "double")), (name, words)
    ret = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "char*": C.c_char_p}
    for r, name in re.findall(r"(\w+\s*\*?)\s*\b(fn_[a-z0-9_]+)\s*\([^()]*\)\s*;", text):
        assert _lib.HEADER.functions[name][0] is ret[r.replace(" ", "")], name


_STRUCT = "typedef struct fn_s { %s } fn_s;"


@pytest.mark.parametrize("text, offender", [
    (_STRUCT % "int32_t a; size_t n;", "size_t"),                                  # a member of unknown type
    (_STRUCT % "int32_t flags : 3;", "flags : 3"),                                 # a bit-field
    ("typedef union fn_u { int32_t i; float f; } fn_u;", "union"),
    (_STRUCT % "void (*done)(int status);", "(*done)"),                           # a function-pointer member
    ("int fn_log(const char* fmt, ...);", "..."),
    ("int fn_a(void);\nstray\nint fn_b(void);", "stray"),
    ("int fn_a(void);\nint x;\n" + _STRUCT % "int32_t a;", "int x;"),
    ("#define FN_N (1 + 2)\n", "FN_N"),
    ("#define LIMIT 3\n", "LIMIT"),
    ("#if 0\nint fn_a(void);\n#endif\n", "#if 0"),
    (_STRUCT % "int32_t a[FN_UNDEFINED];", "FN_UNDEFINED"),
    ("size_t fn_count(void);", "size_t"),
    (_STRUCT % "int32_t a;" + "\nint fn_take(fn_s by_value);", "by value"),
])
def test_the_reader_refuses_what_it_does_not_know(text, offender):
    from fragnet_amd._header import FragnetHipError, parse
    with pytest.raises(FragnetHipError) as e:
        parse(text)
    assert offender in str(e.value)


def _offsets(cls):
    return [(field, getattr(cls, field).offset) for field, *_ in cls._fields_]


def test_the_reader_accepts_what_the_header_uses():
    from fragnet_amd._header import parse
    s = parse(_STRUCT % "int32_t n; const float *a, *b;").structs["fn_s"]
    assert _offsets(s) == [("n", 0), ("a", 8), ("b", 16)] and C.sizeof(s) == 24
    s = parse(_STRUCT % "float* p;  const float* g; int64_t m;").structs["fn_s"]
    assert _offsets(s) == [("p", 0), ("g", 8), ("m", 16)]
    assert all(t is C.c_void_p for _, t in s._fields_[:2]) and s._fields_[2][1] is C.c_int64
    h = parse("#define FN_MAX_SPACES 8\n" + _STRUCT % "int32_t k; int64_t cap[FN_MAX_SPACES], lit[3]; float tail;")
    assert _offsets(h.structs["fn_s"]) == [("k", 0), ("cap", 8), ("lit", 72), ("tail", 96)] and C.sizeof(h.structs["fn_s"]) == 104
    h = parse("typedef struct fn_in { int64_t n; int32_t k; } fn_in;\n" + _STRUCT % "int32_t a; fn_in one; fn_in two[2]; int32_t z;")
    assert _offsets(h.structs["fn_s"]) == [("a", 0), ("one", 8), ("two", 24), ("z", 56)] and list(h.structs) == ["fn_in", "fn_s"]
    h = parse("struct fn_x;\n" + _STRUCT % "int32_t a; struct fn_x* p; const struct fn_x* q; double d;")
    assert _offsets(h.structs["fn_s"]) == [("a", 0), ("p", 8), ("q", 16), ("d", 24)]
    h = parse("#define FN_E (-1)\n#define FN_H 0x10\n#define FN_WS(n) ((n) + 4)\n#define FN_N 7 /* seven */\n#ifndef G\n#define G\n#endif\n")
    assert h.constants == {"FN_E": -1, "FN_H": 16, "FN_N": 7}
    h = parse('extern "C" {\ntypedef void* fn_stream_t;\n' + _STRUCT % "int32_t a;" + """
        const char* fn_last(void);
        int64_t fn_ws(int64_t M, int K);
        int fn_run(const fn_s* s, int* n_part, const int64_t* index, void* const* events, float p, double q,
                   uint64_t seed, fn_stream_t stream);
        }""")
    assert h.functions["fn_last"] == (C.c_char_p, []) and h.functions["fn_ws"] == (C.c_int64, [C.c_int64, C.c_int])
    restype, (s_ptr, n_part, *rest) = h.functions["fn_run"]
    assert restype is C.c_int and s_ptr._type_ is h.structs["fn_s"] and n_part._type_ is C.c_int
    assert rest == [C.c_void_p, C.c_void_p, C.c_float, C.c_double, C.c_uint64, C.c_void_p]


def test_binding_names_follow_the_header():
    """Both spellings of every constant, the CamelCase classes, and a missing header is an error that says where it was looked for."""
    from fragnet_amd import _lib, build, ops
    for name, value in _lib.HEADER.constants.items():
        assert getattr(_lib, name) == getattr(_lib, name[len("FN_"):]) == value
    assert (_lib.FN_EINVAL, _lib.STAGE_ROWS_I64, _lib.TUNE_COUNT, _lib.FN_D) == (-1, 8, 35, 128)
    assert _lib.LAYER_FIELDS[0] == "proj_b_w" and len(_lib.LAYER_FIELDS) * 8 == C.sizeof(_lib.LayerWeights)
    assert (ops.SMALL_LINEAR_MAX, ops.DENSE_MAX_ROWS) == (_lib.FN_SMALL_LINEAR_MAX, _lib.FN_DENSE_MAX_ROWS) == (16, 4096)
    found = build.HEADERS[0]
    try:
        build.HEADERS[0] = os.path.join(ROOT, "include", "no_such_header.h")
        with pytest.raises(_lib.FragnetHipError, match="no_such_header.h"):
            _lib._read_header()
    finally:
        build.HEADERS[0] = found


def test_library_exports_every_declared_symbol():
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in fragnet_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes binding and header disagree"
    assert lib.fn_abi_version() == _lib.ABI_VERSION == 12


def test_tuning_table_reads_back_through_the_abi():
    """fn_get_tuning (added under ABI 12: additions do not bump the version) is declared, exported and bound, and is the inverse of
    fn_set_tuning; tests/test_tuning_ranges_host.py has the ranges."""
    from fragnet_amd import _lib
    lib = _lib.load()
    assert "fn_get_tuning" in _declared() and _lib.SIGNATURES["fn_get_tuning"] == _lib.SIGNATURES["fn_set_tuning"][:1]
    old = lib.fn_get_tuning(31)
    try:
        _lib.call("fn_set_tuning", 31, old + 5)
        assert lib.fn_get_tuning(31) == old + 5
    finally:
        _lib.call("fn_set_tuning", 31, old)
    assert lib.fn_get_tuning(31) == old
    assert lib.fn_set_tuning(31, -1) == -1 and b"FWD_TAIL_ROWS" in lib.fn_last_error() and lib.fn_get_tuning(31) == old


def test_library_exports_nothing_but_the_declared_entry_points():
    """Every defined function symbol of the .so is a declared fn_* entry point (helpers must be static: a namespace-scope
    function inside the extern "C" block is exported under its plain name)."""
    import shutil
    import subprocess
    from fragnet_amd.build import OUT, build_lib
    build_lib()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", OUT], capture_output=True, text=True, check=True).stdout
    funcs = sorted(line.split()[-1] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] == "T")
    assert funcs == _declared(), f"exported but not declared: {sorted(set(funcs) - set(_declared()))}"


def test_plan_layout_is_host_side_and_validates():
    import ctypes as C
    from fragnet_amd import _lib
    lib = _lib.load()
    tasks = (_lib.CsrTask * 16)()
    tasks[0] = _lib.CsrTask(None, None, 10, 3, 5, 0, 0, 0, -1)
    tasks[1] = _lib.CsrTask(None, None, 7, 0, 4, 0, 0, 0, -1)
    ti, ts = C.c_int64(), C.c_int64()
    assert lib.fn_plan_layout(tasks, 2, C.byref(ti), C.byref(ts)) == 0
    assert (ti.value, ts.value) == (20, 9)
    assert (tasks[1].item_base, tasks[1].seg_base) == (13, 5)
    assert lib.fn_plan_layout(tasks, 17, C.byref(ti), C.byref(ts)) == -3
    assert b"FN_MAX_TASKS" in lib.fn_last_error()
    tasks[0].n_real = -1
    assert lib.fn_plan_layout(tasks, 1, C.byref(ti), C.byref(ts)) == -1


def test_argument_errors_do_not_touch_the_gpu():
    from fragnet_amd import _lib
    lib = _lib.load()
    assert lib.fn_segment_sum_f32(None, 128, None, None, 0, None, 4, 128, 16, None) == -1
    assert lib.fn_row_dots_sorted_f32(None, None, 128, 0, 9, None, None, None) == -1
    assert lib.fn_dropout_act_f32(None, None, 8, 1.5, 0, 0, None, 1, None) == -1


def test_cpu_tensors_are_refused_not_silently_computed():
    from fragnet_amd import _lib, ops
    with pytest.raises(_lib.FragnetHipError):
        ops.scatter_add(torch.ones(4, 2), torch.tensor([0, 1, 0, 1]))
    from fragnet_amd import data, synth
    from fragnet_amd.model import FragNetFineTune
    model = FragNetFineTune(num_layer=1, h1=8, h2=8, h3=8, h4=8)
    batch = data.collate_fn(synth.synth_molecules(2, seed=1))
    with pytest.raises(_lib.FragnetHipError):
        model(batch)


def test_state_dict_layout_matches_reference_key_order():
    """Same module tree as the reference => same keys in the same order (tests/golden pkeys)."""
    from fragnet_amd.model import FragNetFineTune, FragNetPreTrain
    from tests.helpers import check_params_match, load_case
    for case, cls in (("ft_esol_b8", FragNetFineTune), ("ft_tox21_b4", FragNetFineTune), ("pt_esol_b4", FragNetPreTrain)):
        cfg, _, _, _, pkeys, psums = load_case(case)
        torch.manual_seed(cfg["seed"])
        check_params_match(cls(**cfg["ctor"]), pkeys, psums)
