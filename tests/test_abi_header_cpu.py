"""The Python binding is derived from include/l4p_hip.h (l4p_amd/_header.py): the host compiler referees the reader, the
C-to-ctypes mapping is pinned on literal cases, and what the reader does not understand raises and names the declaration."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from l4p_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)
STRUCTS = {"l4p_gemm_desc": _lib.GemmDesc, "l4p_encoder_cfg": _lib.EncoderCfg, "l4p_dpt_cfg": _lib.DptCfg,
           "l4p_track_cfg": _lib.TrackCfg, "l4p_gt_field": _lib.GtField}


def test_reader_counts_and_public_surface():
    h = _lib.HEADER
    raw = open(os.path.join(ROOT, "include", "l4p_hip.h")).read()
    assert set(h.constants) == set(re.findall(r"^#define[ \t]+(L4P_\w+)[ \t]+\S", raw, re.M)) and len(h.constants) >= 37
    assert set(h.structs) == set(STRUCTS) and h.handles == ("l4p_stream",) and h.opaque == ("l4p_engine",)
    assert set(h.protos) == set(_lib.SIGNATURES) and len(h.protos) >= 108
    for name, value in h.constants.items():  # every constant by its header name, the three families also without the prefix
        assert getattr(_lib, name) == value and type(getattr(_lib, name)) is type(value)
    assert (_lib.L4P_BF16, _lib.L4P_F32, _lib.L4P_F16) == (0, 1, 2) and _lib.L4P_E_INVALID == -1
    assert (_lib.EPI_DENSE, _lib.EPI_QKV, _lib.EPI_CONVT, _lib.EPI_MASKDOT) == (0, 1, 2, 3)
    assert (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_RELU) == (0, 1, 2)
    assert (_lib.GT_MAX_FIELDS, _lib.GT_NEAREST, _lib.GT_BILINEAR) == (10, 0, 1)
    assert _lib.L4P_ATTN_PRESCALED == 0.0 and isinstance(_lib.L4P_ATTN_PRESCALED, float)


def test_compiler_agrees_with_the_reader(tmp_path):
    """One translation unit over the real header, written from the reader's output: the compiler's sizeof / offsetof of every struct
    and field and its value of every #define against ctypes and _lib, and a static_assert per function that its type is the one the
    reader spelled."""
    if CXX is None:
        pytest.skip("no host C++ compiler")
    h = _lib.HEADER
    src = ["#include <cstddef>", "#include <cstdio>", "#include <type_traits>", '#include "l4p_hip.h"']
    for name, p in h.protos.items():
        args = ", ".join(a.spell() for a in p.args)
        src.append(f'static_assert(std::is_same<decltype(&{name}), {p.ret.spell()} (*)({args})>::value, "{name}");')
    src.append("int main() {")
    for sname, fields in h.structs.items():
        src.append(f'  printf("sizeof {sname} %zu\\n", sizeof({sname}));')
        for f in fields:
            src.append(f'  printf("field {sname}.{f.name} %zu %zu\\n", offsetof({sname}, {f.name}), sizeof((({sname}*)0)->{f.name}));')
    for name in h.constants:
        src.append(f'  printf("define {name} %d %.17g\\n", (int)std::is_integral<decltype({name})>::value, (double)({name}));')
    src.append("  return 0;\n}")
    cpp, exe = tmp_path / "abi_check.cpp", tmp_path / "abi_check"
    cpp.write_text("\n".join(src) + "\n")
    out = subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"),
                          str(cpp), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    want = []
    for sname, cls in STRUCTS.items():
        want.append(f"sizeof {sname} {C.sizeof(cls)}")
        assert [n for n, _ in cls._fields_] == [f.name for f in h.structs[sname]]
        want += [f"field {sname}.{n} {getattr(cls, n).offset} {getattr(cls, n).size}" for n, _ in cls._fields_]
    want += [f"define {n} {int(isinstance(v, int))} {float(v):.17g}" for n, v in h.constants.items()]
    assert run.stdout.splitlines() == want


VP, I, LL, F, D, SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double, C.c_size_t


def test_mapping_on_literal_cases():
    S, P = _lib.SIGNATURES, _lib.HEADER.protos
    assert S["l4p_recon_cameras"] == (I, [VP, VP, I, I, I, I, D, D, D, VP, VP, VP])
    assert S["l4p_metric_ws_bytes"] == (SZ, [I, LL, I])
    assert S["l4p_metric_depth"] == (I, [VP, VP, VP, VP, I, LL, I, F, F, VP, SZ, VP])
    assert P["l4p_dpt_forward"].args[4].spell() == "const void* const*" and P["l4p_encoder_forward"].args[8].spell() == "float* const*"
    assert S["l4p_dpt_forward"] == (I, [VP, VP, C.c_char_p, C.POINTER(_lib.DptCfg), VP, I, VP, SZ, VP])
    assert S["l4p_last_error"] == (C.c_char_p, []) and S["l4p_prof_class_name"] == (C.c_char_p, [I])
    assert S["l4p_prof_detail"] == (LL, [C.c_char_p, LL]) and S["l4p_set_knob"] == (I, [C.c_char_p, I])
    assert S["l4p_gemm"] == (I, [VP, I, C.POINTER(_lib.GemmDesc)]) and S["l4p_gemm_group"] == (I, [VP, I, C.POINTER(_lib.GemmDesc), I])
    assert S["l4p_gt_dense_clip"][1][1] is C.POINTER(_lib.GtField)
    assert S["l4p_track_window_workspace_bytes"] == (SZ, [VP, C.POINTER(_lib.TrackCfg), I, I])
    assert S["l4p_encoder_configure"] == (I, [VP, C.POINTER(_lib.EncoderCfg)])
    assert S["l4p_point_map_samples"][1][-1] is C.c_uint and S["l4p_similarity_ransac"][1][8] is C.c_uint
    assert S["l4p_view_splat"][1][-1] is VP and P["l4p_view_splat"].args[-1].spell() == "unsigned long long*"
    # host out-parameters and handles: plain addresses
    assert S["l4p_create"] == (I, [I, I, VP]) and S["l4p_destroy"] == (I, [VP]) and S["l4p_stream_create_cu_mask"] == (I, [I, I, VP])
    assert S["l4p_prof_read"] == (I, [I, VP, VP]) and S["l4p_pil_coeffs"] == (I, [I, I, VP, VP, I, VP])
    # what callers pass still type-checks: byref of the very struct class, a ctypes array of it, byref of a scalar, None
    S["l4p_gemm"][1][2].from_param(C.byref(_lib.GemmDesc()))
    S["l4p_gemm_group"][1][2].from_param((_lib.GemmDesc * 2)())
    for arg in (C.byref(C.c_int(0)), (C.c_void_p * 4)(), None, 4096):
        VP.from_param(arg)
    with pytest.raises(TypeError):
        S["l4p_gemm"][1][2].from_param(C.byref(_lib.DptCfg()))
    assert _lib.DptCfg.actpost.size == 48 and _lib.DptCfg().actpost[3][2] == 0 and len(_lib.DptCfg().layer_dims) == 4


def test_mapping_of_a_small_header():
    h = _header.parse("""
        #define L4P_A 3
        #define L4P_B (-2) /* negative */
        #define L4P_C 0.5f
        typedef void* l4p_stream;
        typedef struct l4p_engine l4p_engine;
        typedef struct l4p_s { int a, b; const float* p; long long n; unsigned char tag[3]; int m[4][3]; double d; } l4p_s;
        // a line comment
        long long l4p_f(l4p_stream s, const l4p_s* x, l4p_s** xs, unsigned char* y, float* const* z, double d, unsigned u,
                        unsigned long long big, size_t n, const char* name, char* buf, l4p_engine** out, float);
        void l4p_g(void);
    """)
    assert h.constants == {"L4P_A": 3, "L4P_B": -2, "L4P_C": 0.5}
    b = _header.bind(h)
    s = b.structs["l4p_s"]
    assert [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_] == [
        ("a", 0, 4), ("b", 4, 4), ("p", 8, 8), ("n", 16, 8), ("tag", 24, 3), ("m", 28, 48), ("d", 80, 8)] and C.sizeof(s) == 88
    assert b.signatures["l4p_f"] == (LL, [VP, C.POINTER(s), VP, VP, VP, D, C.c_uint, C.c_ulonglong, SZ, C.c_char_p, C.c_char_p, VP, F])
    assert b.signatures["l4p_g"] == (None, [])


@pytest.mark.parametrize("text, names", [
    ("typedef struct l4p_s { int a; short x; } l4p_s;", ["short x", "l4p_s"]),
    ("int l4p_f(int n, void (*done)(int));", ["l4p_f"]),
    ("typedef struct l4p_s { int a : 3; } l4p_s;", ["int a : 3", "l4p_s"]),
    ("typedef union l4p_u { int a; float b; } l4p_u;", ["l4p_u"]),
    ("typedef struct l4p_s { int a; union { int b; float c; } u; } l4p_s;", ["l4p_s"]),
    ("int l4p_f(hipStream_t stream, int n);", ["hipStream_t", "l4p_f"]),
    ("uint64_t l4p_f(int n);", ["uint64_t", "l4p_f"]),
    ("int l4p_f(int n)\nint l4p_g(int n);", ["l4p_f"]),  # a lost ';': the prototype pattern would match only half
    ("int l4p_f(unsigned long n);", ["unsigned long", "l4p_f"]),
    ("typedef struct l4p_engine l4p_engine;\nint l4p_f(l4p_engine e);", ["l4p_engine", "l4p_f"]),
    ("int l4p_f(int n[4]);", ["l4p_f"]),
    ("#define L4P_X (1 << 4)", ["L4P_X"]),
    ("#define L4P_MAX(a, b) ((a) > (b) ? (a) : (b))", ["L4P_MAX"]),
    ("#if L4P_X\nint l4p_f(void);\n#endif", ["#if L4P_X"]),
    ("static inline int l4p_f(int n) { return n; }", ["l4p_f"]),
    ("int l4p_f(int n); /* never closed", ["comment"]),
], ids=["short-field", "function-pointer", "bit-field", "union", "nested-union", "unknown-typedef", "unknown-return", "lost-semicolon",
        "unsigned-long", "opaque-by-value", "array-parameter", "expression-define", "function-macro", "if-directive", "function-body",
        "open-comment"])
def test_reader_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(_header.HeaderError) as err:
        _header.parse(text)
    for name in names:
        assert name in str(err.value), str(err.value)


def test_header_is_read_once_per_process(monkeypatch):
    def again(text):
        raise AssertionError("the header was parsed again")

    monkeypatch.setattr(_header, "parse", again)
    monkeypatch.setattr(_header, "bind", again)
    assert _lib.load() is _lib.load()
    assert _lib.SIGNATURES["l4p_gemm"][1][2] is C.POINTER(_lib.GemmDesc)
