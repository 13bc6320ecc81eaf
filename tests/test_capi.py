"""CPU: the C-ABI library loads without a GPU and exports every symbol include/glare_hip.h
declares; the product refuses CPU tensors instead of falling back."""
import ast
import ctypes
import os
import re
import subprocess

import pytest
import torch

from glare_amd import _lib


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (glare_[a-z0-9_]+)", out))


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    names = _lib.header_symbols()
    assert "glare_vq_nearest_f32" in names and "glare_version" in names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.glare_version() >= 100
    assert lib.glare_status_string(0) == b"ok"
    assert lib.glare_status_string(-1) == b"invalid argument"


def test_glare_error_carries_the_numeric_status():
    """callers decide on `e.status` (a GLARE_ERR_* code of the header), never on the wording of the message."""
    src = open(_lib.HEADER_PATH).read()
    for name, val in (("INVALID", _lib.ERR_INVALID), ("LAUNCH", _lib.ERR_LAUNCH), ("WORKSPACE", _lib.ERR_WORKSPACE), ("UNSUPPORTED", _lib.ERR_UNSUPPORTED)):
        assert re.search(r"#define GLARE_ERR_%s \(%d\)" % (name, val), src), name
    with pytest.raises(_lib.GlareError) as ei:
        _lib.check(_lib.ERR_UNSUPPORTED, "glare_something")
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "glare_something" in str(ei.value)
    assert _lib.GlareError("raised on the Python side").status is None
    _lib.check(0, "fine")
    # the DCN's single-pass opt-in falls back on the status, not on the text
    dd = open(os.path.join(os.path.dirname(_lib.__file__), "modules", "deformableDecoder_arch.py")).read()
    assert "e.status != _lib.ERR_UNSUPPORTED" in dd and '"unsupported" not in' not in dd


def test_no_extra_exports():
    """Everything exported with the glare_ prefix is declared in the header (the ABI is the header), and the prototypes the binding
    parses from it (header_symbols() is a view of signatures()) are exactly the exports."""
    assert _exports(_lib.LIB_PATH) == set(_lib.header_symbols())


def test_library_is_gfx950_only():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", _lib.LIB_PATH], capture_output=True, text=True)
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    for other in (b"gfx942", b"gfx90a", b"sm_80"):
        assert other not in data


def test_product_refuses_cpu_tensors():
    from glare_amd import ops

    z = torch.zeros(4, 3)
    cb = torch.zeros(16, 3)
    with pytest.raises(NotImplementedError):
        ops.vq_nearest(z, cb)


def test_half_library_exports_the_inference_entry_points():
    """libglare_hip_f16.so (IEEE-half activations / filters; since round 4 a build of EVERY source, training kernels included):
    each export is declared in the header -- a *_bf16 entry point under the name *_f16, identical signature -- and it exports
    nothing the header does not declare."""
    exported = _exports(_lib.LIB_F16_PATH)
    declared = set(_lib.header_symbols())
    as_f16 = {n.replace("bf16", "f16") for n in declared}
    assert exported <= as_f16, sorted(exported - as_f16)
    for must in ("glare_conv2d_f16", "glare_conv1x1_ws_f16", "glare_attention_kv512_f16", "glare_groupnorm_apply_f16",
                 "glare_mdcn_forward_nhwc", "glare_flow_h1_f32", "glare_flow_tail_f32", "glare_conv2d_smallcin_f32", "glare_mix_f16"):
        assert must in exported, must
    assert not any("bf16" in n for n in exported)
    data = open(_lib.LIB_F16_PATH, "rb").read()
    assert b"gfx950" in data and b"gfx942" not in data
    # the precision switch resolves names through it, and refuses what it does not have
    from glare_amd import ops

    with ops.use_precision("fp16"):
        assert ops.act_dtype() == torch.float16
        assert _lib.lib().glare_conv2d_bf16 is not None          # -> glare_conv2d_f16
        with pytest.raises(_lib.GlareError):
            _lib.lib().glare_wgrad_nhwc_bf16
        assert _lib.lib().glare_vq_nearest_f32 is not None       # dtype-agnostic: the main library's
    assert ops.act_dtype() == torch.bfloat16
    assert ops.inference_precision() == "fp16" and ops.inference_precision("bf16") == "bf16"


def _assert_typed(fn, name):
    restype, argtypes = _lib.signatures()[name]
    assert fn.restype is restype, (name, fn.restype, restype)
    assert fn.argtypes is not None and list(fn.argtypes) == argtypes, (name, fn.argtypes, argtypes)


def test_every_entry_point_is_typed_from_the_header():
    """Both libraries come out of lib() with argtypes / restype of every declared entry point set from its prototype: call sites pass
    plain Python values, and no caller sets a type."""
    lib = _lib.lib()
    for name in _lib.header_symbols():
        _assert_typed(getattr(lib, name), name)
    half = {n.replace("bf16", "f16") for n in _exports(_lib.LIB_F16_PATH)}
    with _lib.use_precision("fp16"):
        lib16 = _lib.lib()
        checked = 0
        for name in _lib.header_symbols():
            if name.replace("bf16", "f16") in half:
                fn = getattr(lib16, name)
                assert fn is getattr(lib16._c, name.replace("bf16", "f16"))       # the half library's export, typed as x_bf16
                _assert_typed(fn, name)
                checked += 1
        assert checked == len(half)


def test_header_parse_maps_the_closed_type_table_and_refuses_unknown_types():
    c = ctypes
    sigs = _lib.parse_prototypes("""
        #define GLARE_PAD_SYMMETRIC 1   /* a define right above a prototype */
        int glare_pad(const unsigned char* x, int mode, glare_stream_t stream);
        typedef struct glare_thing { int a; float* b; } glare_thing;
        const char* glare_name(int status);   // trailing comment
        size_t glare_bytes(int B,
                           long long HW);
        long long glare_count(void);
        int glare_fill(const glare_thing* t, float v, const float* M_3x3_host, double* out);""")
    assert sigs == {"glare_pad": (c.c_int, [c.c_void_p, c.c_int, c.c_void_p]),
                    "glare_name": (c.c_char_p, [c.c_int]),
                    "glare_bytes": (c.c_size_t, [c.c_int, c.c_longlong]),
                    "glare_count": (c.c_longlong, []),
                    "glare_fill": (c.c_int, [c.c_void_p, c.c_float, c.c_void_p, c.c_void_p])}
    for bad in ("int glare_x(double v);", "int glare_x(unsigned n);", "double glare_x(int n);", "int glare_x(int);"):
        with pytest.raises(_lib.GlareError):
            _lib.parse_prototypes(bad)


_SCALAR_CTYPE = re.compile(r"c_(u?(byte|short|int|long|longlong)\d*|size_t|ssize_t|float|double|longdouble|bool)$")


def test_call_sites_pass_the_declared_number_of_arguments():
    """A static audit of every literal `.glare_<name>(...)` call: ctypes accepts EXTRA arguments to a typed cdecl function silently,
    so this is what catches one.  Outside glare_amd/_lib.py nothing sets a restype / argtypes, constructs a scalar ctypes value
    or aliases a scalar ctypes type -- the header's prototypes are the only binding."""
    sigs = _lib.signatures()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(d, f) for sub in ("glare_amd", "tests", "tools") for d, _, fs in os.walk(os.path.join(root, sub))
             for f in fs if f.endswith(".py")]
    lib_py = os.path.join(root, "glare_amd", "_lib.py")
    calls, bad = 0, []
    for path in files:
        where = os.path.relpath(path, root)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("glare_"):
                if any(isinstance(a, ast.Starred) for a in node.args) or node.keywords:
                    continue
                name = node.func.attr
                if name not in sigs:
                    bad.append("%s:%d calls %s, which the header does not declare" % (where, node.lineno, name))
                elif len(node.args) != len(sigs[name][1]):
                    bad.append("%s:%d passes %d arguments to %s (declared: %d)" % (where, node.lineno, len(node.args), name, len(sigs[name][1])))
                calls += 1
            if path == lib_py:
                continue
            if isinstance(node, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
                targets = node.targets if isinstance(node, ast.Assign) else [node.target]
                if any(isinstance(t, ast.Attribute) and t.attr in ("restype", "argtypes") for t in targets):
                    bad.append("%s:%d sets a restype / argtypes" % (where, node.lineno))
                v = node.value
                if isinstance(v, ast.Attribute) and _SCALAR_CTYPE.match(v.attr):
                    bad.append("%s:%d aliases ctypes.%s" % (where, node.lineno, v.attr))
                if isinstance(v, ast.Tuple) and any(isinstance(e, ast.Attribute) and _SCALAR_CTYPE.match(e.attr) for e in v.elts):
                    bad.append("%s:%d aliases a scalar ctypes type" % (where, node.lineno))
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and _SCALAR_CTYPE.match(node.func.attr):
                bad.append("%s:%d constructs ctypes.%s" % (where, node.lineno, node.func.attr))
            if isinstance(node, ast.ImportFrom) and node.module == "ctypes" and any(_SCALAR_CTYPE.match(a.name) for a in node.names):
                bad.append("%s:%d imports a scalar ctypes type" % (where, node.lineno))
    assert calls > 150
    assert not bad, "\n".join(bad)


def test_size_queries_return_their_full_width_without_caller_types():
    """A size_t / long long result past 2^32 comes back whole with no restype set by the caller (host-only queries: no GPU needed)."""
    lib = _lib.lib()
    one = lib.glare_groupnorm_workspace_bytes(1, 64)
    assert one > 0 and lib.glare_groupnorm_workspace_bytes(2 ** 30, 64) == 2 ** 30 * one > 2 ** 32
    # glare_hip.h: [wz hi | lo] 2 x 2 KB, [W2 hi | lo] 2 x 8 KB, [W4 hi | lo] 2 x 8 KB, fp32 b2 [2][2][16] and b4[4]
    assert lib.glare_flow_step_fused_image_bytes() == 2 * 2048 + 4 * 8192 + 4 * (2 * 2 * 16 + 4)


_STRUCTS = ("glare_conv_desc", "glare_pack_job")


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """ops.ConvDesc / ops._PackJob are parsed from the header; a host C compiler (the oracle Makefile's $CC, default gcc) says what the
    header means: sizeof and every field's offset and size, in declaration order."""
    import keyword

    from glare_amd import ops

    classes = _lib.structs()
    assert ops.ConvDesc is classes["glare_conv_desc"] and ops._PackJob is classes["glare_pack_job"]
    src = open(_lib.HEADER_PATH).read()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "glare_hip.h"', "int main(void) {"]
    c_names = {}
    for s in _STRUCTS:
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (s, s), re.sub(r"/\*.*?\*/", " ", src, flags=re.S), flags=re.S).group(1)
        c_names[s] = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f) for f in c_names[s]]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.dirname(_lib.HEADER_PATH), "-o", exe, str(tmp_path / "layout.c")], check=True)
    said = dict(line.split(" ", 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for s in _STRUCTS:
        cls = classes[s]
        assert len(c_names[s]) > 10 - 2 * (s == "glare_pack_job")
        assert [f[0] for f in cls._fields_] == [n + "_" if keyword.iskeyword(n) else n for n in c_names[s]]
        assert ctypes.sizeof(cls) == int(said[s]), s
        for (py, _), c in zip(cls._fields_, c_names[s]):
            off, size = map(int, said["%s.%s" % (s, c)].split())
            assert (getattr(cls, py).offset, getattr(cls, py).size) == (off, size), (s, c)
    assert len(ops.ConvDesc._fields_) == 36 and ops.ConvDesc._fields_[0][0] == "in_"


def test_struct_parse_maps_the_closed_type_table_and_refuses_unknown_types():
    c = ctypes
    got = _lib.parse_structs("""
        #define GLARE_N 4
        typedef struct glare_thing {
          const void* in;      /* a Python keyword */
          int B, H,
              W;               // three declarators, two lines
          /* a block comment; with a semicolon, { a brace } and
             a second line between fields */
          long long total;
          const float * bias;
          size_t bytes; float eps;
        } glare_thing;
        int glare_use(const glare_thing* t);
        typedef struct glare_other { void* p; } glare_other;""")
    assert list(got) == ["glare_thing", "glare_other"]
    assert got["glare_thing"]._fields_ == [("in_", c.c_void_p), ("B", c.c_int), ("H", c.c_int), ("W", c.c_int), ("total", c.c_longlong),
                                           ("bias", c.c_void_p), ("bytes", c.c_size_t), ("eps", c.c_float)]
    assert issubclass(got["glare_other"], c.Structure) and got["glare_other"]._fields_ == [("p", c.c_void_p)]
    for bad in ("double x;", "unsigned n;", "struct { int a; } inner;", "int a[4];", "int a, *b;", "int a : 3;"):
        with pytest.raises(_lib.GlareError):
            _lib.parse_structs("typedef struct glare_x { int ok; %s } glare_x;" % bad)


def test_constants_come_from_the_header():
    from glare_amd import harness, ops

    k = _lib.parse_constants("""
        #define GLARE_HIP_H
        #define GLARE_A 3   /* comment */
        #define GLARE_B (-4)
        // #define GLARE_C 5
        #define OTHER 7
        enum { GLARE_X = 0, GLARE_Y = 12 };""")
    assert k == {"GLARE_A": 3, "GLARE_B": -4, "GLARE_X": 0, "GLARE_Y": 12}
    assert ops.ACT == {"none": 0, "relu": 1, "sigmoid": 2, "swish": 3} and ops.ACT["swish"] == 3
    assert (ops.OUT_NHWC_BF16, ops.OUT_NHWC_F32, ops.OUT_PLANAR_F32, ops.OUT_PLANAR_BF16) == (0, 1, 2, 3)
    assert ops.PACK_BLOCK_ELEMS == 2048
    assert (_lib.ERR_INVALID, _lib.ERR_LAUNCH, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED) == (-1, -2, -3, -4)
    assert (ops.MDCN_GENERAL_KERNEL, ops.MDCN_SINGLE_PASS) == (1, 2)
    assert (harness.PAD_REFLECT101, harness.PAD_SYMMETRIC) == (0, 1)
    consts = _lib.constants()
    assert (consts["GLARE_PACK_FORWARD"], consts["GLARE_PACK_DGRAD"], consts["GLARE_PACK_PLAIN_BF16"]) == (0, 1, 2)


def test_ops_does_not_probe_packed_conv_attributes():
    """Every PackedConv has every field (ops.PackedConv.__slots__): consumers read the attribute, so that a misspelt name is an
    AttributeError and not a silent "feature off"."""
    from glare_amd import ops

    fields = {"split", "w16", "w16_lo", "k_wrap", "cout_tile", "subpixel", "_src"}
    assert fields < set(ops.PackedConv.__slots__)
    probes = [node.lineno for node in ast.walk(ast.parse(open(ops.__file__).read()))
              if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr" and len(node.args) >= 2
              and isinstance(node.args[1], ast.Constant) and node.args[1].value in fields]
    assert not probes, probes
