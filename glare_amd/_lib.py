"""ctypes binding of libglare_hip.so (the C ABI declared in include/glare_hip.h).

The product path has no fallback: if the shared library is missing or a symbol cannot be
resolved, importing/using an op raises.  torch is imported first so that the HIP runtime the
library resolves (`libamdhip64.so.7`) is the one torch already loaded -- device pointers and
streams are then shared between torch and the kernels.

Every entry point is typed once, at load, from its prototype in the header (signatures()); callers pass plain Python
numbers, ptr() of a tensor and stream_handle(), and never set a restype or argtypes themselves.
"""
import ctypes
import keyword
import os
import re
import threading

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libglare_hip.so")
LIB_F16_PATH = os.path.join(_HERE, "libglare_hip_f16.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "glare_hip.h")

_lib = None
_lib_f16 = None
# The 16-bit activation / filter format of the kernels in use: "bf16" (libglare_hip.so) or "fp16" (libglare_hip_f16.so).
# None = not set by any enclosing use_precision() of THIS thread: plain ops (and everything with a tape) then run bf16, the inference entry
# points (VQLLFLOWDeformable.reverse_flow_nhwc, glare_amd.infer, bench.py) run INFERENCE_PRECISION.
# Thread-local: the reference boundary is entered from one thread per GPU under nn.DataParallel, and a precision
# switched by one thread's context manager must not leak into another's launches.
_TLS = threading.local()
INFERENCE_PRECISION = "fp16"


def _current():
    return getattr(_TLS, "precision", None)


class GlareError(RuntimeError):
    """`status`: the numeric GLARE_ERR_* code of include/glare_hip.h (None for errors raised on the Python side)."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


# The closed table of C types the ABI uses: any pointer (and glare_stream_t) is a void*; anything else raises.
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "float": ctypes.c_float}


def _ctype(decl, is_return=False):
    decl = re.sub(r"\s*\*", "*", " ".join(decl.split()))
    if is_return and decl == "const char*":
        return ctypes.c_char_p
    if decl.endswith("*") or decl == "glare_stream_t":
        return ctypes.c_void_p
    if decl in _SCALARS:
        return _SCALARS[decl]
    raise GlareError("no ctypes binding for the C type %r (glare_amd/_lib.py _SCALARS)" % decl)


def _strip(text, preprocessor=True):
    """C header text without its comments and (unless preprocessor=False) without its preprocessor lines."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M) if preprocessor else text      # `#define GLARE_PAD_SYMMETRIC 1` must not glue onto the next return type


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every glare_* function prototype in C header text."""
    text = re.sub(r"\{[^{}]*\}", " ", _strip(text).replace('extern "C" {', " "))     # struct / enum bodies
    sigs = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*(.*?)\b(glare_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m is None:
            continue
        ret, name, params = m.groups()
        params = [" ".join(p.split()) for p in params.split(",")]
        argtypes = []
        if params != ["void"]:
            for p in params:
                decl = re.fullmatch(r"(.+?)\s*\b\w+", p)
                if decl is None:
                    raise GlareError("%s: cannot parse the parameter %r" % (name, p))
                argtypes.append(_ctype(decl.group(1)))
        sigs[name] = (_ctype(ret, is_return=True), argtypes)
    return sigs


def parse_structs(text):
    """{name: ctypes.Structure subclass} of every `typedef struct glare_X { ... } glare_X;` in C header text: fields in the header's
    order and of the closed type table; `int B, H, W;` declares three; a field named like a Python keyword gets a trailing underscore."""
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(glare_\w+)\s*\{(.*?)\}\s*\1\s*;", _strip(text), flags=re.S):
        if "{" in body or "}" in body:
            raise GlareError("%s: nested struct / union / enum bodies are not supported" % name)
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            m = re.fullmatch(r"(.+?)\s*\b(\w+)", first)
            if m is None or not all(re.fullmatch(r"\w+", p) for p in more):      # arrays, bit fields, `*b` after a comma, ...
                raise GlareError("%s: cannot parse the field declaration %r" % (name, decl))
            ctype = _ctype(m.group(1))
            fields += [(f + "_" if keyword.iskeyword(f) else f, ctype) for f in [m.group(2)] + more]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "`%s` of include/glare_hip.h." % name})
    return structs


def parse_constants(text):
    """{name: int} of every `#define GLARE_<NAME> <integer>` / `(<integer>)` and every `GLARE_<NAME> = <integer>` of an enum in C header text."""
    text = _strip(text, preprocessor=False)
    consts = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GLARE_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", text):
        consts.update((n, int(v)) for n, v in re.findall(r"\b(GLARE_\w+)\s*=\s*(-?\d+)\s*(?:,|$)", body))
    return consts


_PARSED = {}


def _header(parser):
    if parser not in _PARSED:
        with open(HEADER_PATH) as f:
            _PARSED[parser] = parser(f.read())
    return _PARSED[parser]


def signatures():
    """{name: (restype, [argtypes])} of every function declared in include/glare_hip.h (parsed once)."""
    return _header(parse_prototypes)


def structs():
    """{name: ctypes.Structure subclass} of every struct declared in include/glare_hip.h (parsed once)."""
    return _header(parse_structs)


def constants():
    """{name: int} of every integer GLARE_* constant of include/glare_hip.h (parsed once)."""
    return _header(parse_constants)


ERR_INVALID, ERR_LAUNCH, ERR_WORKSPACE, ERR_UNSUPPORTED = (constants()["GLARE_ERR_" + n] for n in ("INVALID", "LAUNCH", "WORKSPACE", "UNSUPPORTED"))


def header_symbols():
    """Names of every function declared in include/glare_hip.h."""
    return sorted(signatures())


def _bind(cdll, half=False):
    """Types every declared entry point the library exports from its header prototype, once at load: call sites pass plain Python
    values and ctypes converts each to the declared type.  half: libglare_hip_f16.so, whose x_f16 has the signature of the declared x_bf16."""
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(cdll, name.replace("bf16", "f16") if half else name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes


def host_f32(values, n=None):
    """A host `const float*` argument (the *_host arrays of the ABI) from a sequence of numbers: float[n], default float[len(values)]."""
    values = [float(v) for v in values]
    return (ctypes.c_float * (len(values) if n is None else n))(*values)


def precision():
    return _current() or "bf16"


def inference_precision(requested=None):
    """Precision of an inference entry point: the caller's request, else the enclosing use_precision(), else fp16 -- the
    reference's own autocast dtype (infer_dataset_lol.py:134) and what the end-to-end tolerance needs."""
    return requested or _current() or INFERENCE_PRECISION


def act_dtype():
    """torch dtype of 16-bit activations / packed filters under the current precision."""
    return torch.bfloat16 if precision() == "bf16" else torch.float16


class use_precision:
    """`with use_precision("fp16"):` -- ops run the IEEE-half twin of the inference kernels (libglare_hip_f16.so: same kernels,
    same MFMA rate, 11 instead of 8 mantissa bits in every stored activation and filter: the path's parity mode; the
    reference's own autocast dtype, infer_dataset_lol.py:134).  None keeps the current one."""

    def __init__(self, name):
        assert name in (None, "bf16", "fp16"), name
        self.name = name

    def __enter__(self):
        self._prev = _current()
        if self.name is not None:
            _TLS.precision = self.name
        return self

    def __exit__(self, *exc):
        _TLS.precision = self._prev


def keeps_precision(cls):
    """Class decorator for torch.autograd.Function subclasses: the backward runs under the precision the forward ran under.
    The autograd engine calls `backward` from ITS OWN worker threads, where this module's thread-local precision is unset -- without
    this an fp16 training step would run its backward kernels of the bf16 library on fp16 tensors."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args, **kw):
        ctx._glare_precision = _current()
        return fwd(ctx, *args, **kw)

    def backward(ctx, *grads):
        with use_precision(getattr(ctx, "_glare_precision", None)):
            return bwd(ctx, *grads)

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


# entry points without any 16-bit tensor in their signature: under "fp16" they resolve to the main library
_DTYPE_AGNOSTIC = ("glare_vq_", "glare_harness_", "glare_ssim_")


class _F16Lib:
    """libglare_hip_f16.so behind the main library's names: `x_bf16` resolves to its export `x_f16`.  Since round 4 the half
    library is a build of EVERY source (inference and training kernels); an entry point it should ever lack raises -- it must
    never silently run a bf16 kernel on fp16 data."""

    def __init__(self, cdll):
        self._c = cdll

    def __getattr__(self, name):          # reached on the FIRST use of a name only: the resolved function is kept on the instance
        try:
            fn = getattr(self._c, name.replace("bf16", "f16"))
        except AttributeError:
            if not name.startswith(_DTYPE_AGNOSTIC):
                raise GlareError("%s is not part of libglare_hip_f16.so (the fp16 precision covers the inference kernels)" % name)
            fn = getattr(main_lib(), name)
        self.__dict__[name] = fn
        return fn


def lib():
    """The library of the current precision (use_precision); raises GlareError when the HIP extension has not been built."""
    if precision() == "fp16":
        global _lib_f16
        if _lib_f16 is None:
            main_lib()
            if not os.path.exists(LIB_F16_PATH):
                raise GlareError("libglare_hip_f16.so is not built (%s): run __graft_entry__.build()" % LIB_F16_PATH)
            c = ctypes.CDLL(LIB_F16_PATH, mode=ctypes.RTLD_LOCAL)
            _bind(c, half=True)
            _lib_f16 = _F16Lib(c)
        return _lib_f16
    return main_lib()


def main_lib():
    """libglare_hip.so (bf16 activations; every entry point of include/glare_hip.h)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GlareError(
                "libglare_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` -- there is no CPU or eager fallback." % LIB_PATH)
        try:
            c = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover
            raise GlareError("cannot load %s: %s" % (LIB_PATH, e))
        _bind(c)
        _lib = c
    return _lib


def check(status, what):
    if status != 0:
        raise GlareError("%s failed: %s (%d)" % (what, main_lib().glare_status_string(status).decode(), status), status)


def ptr(t):
    """Device pointer of a tensor (None = NULL) for a pointer argument of the ABI."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_handle():
    """The calling thread's current HIP stream as a void* (what every launch of the C ABI takes).  Through torch's two C entry points:
    `torch.cuda.current_stream().cuda_stream` builds a Stream object behind three Python-level device lookups -- 9 us per call, measured
    (tools/probes/train_host_profile.py), i.e. ~12 ms of the ~1 400 launches of a training step that the HOST paces (round 6)."""
    if _raw_stream is not None:
        try:
            return _raw_stream(_cur_device())
        except RuntimeError:   # no initialised HIP context (CPU-side tests of the error paths): the documented route decides what to raise
            pass
    return torch.cuda.current_stream().cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError(
                "glare_amd ops run on MI355X only (HIP kernels, no CPU path); got a %s tensor" % t.device)
