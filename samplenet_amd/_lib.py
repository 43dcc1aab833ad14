"""ctypes binding of libsamplenet_hip.so (the C ABI declared in include/samplenet_hip.h).

There is NO fallback: if the HIP library is missing or does not export a symbol, importing
samplenet_amd fails loudly -- the product path never routes through a CPU or eager-PyTorch
substitute.

The two headers under include/ are the only place a signature is written: PROTOTYPES / RESTYPES are
parsed from them at import (parse_header), so a binding cannot disagree with the declaration the
compiler held the definition to.
"""
import ctypes
import os
import re

import torch  # noqa: F401  -- first: its bundled HIP runtime (libamdhip64.so.7) must be the one this process uses,
# because the streams and device pointers handed to the library come from torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAMPLENET_AMD_LIB: another build of the SAME library (same ABI; build.py --variant / --timeline -- same-box A/B of a kernel change)
LIB_PATH = os.environ.get("SAMPLENET_AMD_LIB") or os.path.join(_HERE, "lib", "libsamplenet_hip.so")
# include/samplenet_hip.h: the drop-in boundary; include/samplenet_hip_internal.h: the fused-step entry points behind it
HEADERS = [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("samplenet_hip.h", "samplenet_hip_internal.h")]

# every type the headers pass by value; a pointer is c_void_p whatever it points to, except `const char *`
_BY_VALUE = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
             "unsigned long long": ctypes.c_ulonglong, "sn_stream_t": ctypes.c_void_p}
_TYPE_WORDS = {w for t in _BY_VALUE for w in t.split()} | {"const", "void", "char"}


def _declarator(text, where, returns=False):
    """(ctypes type, name) of one `type name` as the headers spell it; anything else is an error that says `where`."""
    for mark, what in (("...", "a variadic list"), ("[", "an array"), ("(", "a function pointer")):
        if mark in text:
            raise ValueError("%s: %s is not supported: %r" % (where, what, text))
    *ty, name = re.findall(r"\w+|\S", text) or [""]
    if not ty or name in _TYPE_WORDS or not name.isidentifier():
        raise ValueError("%s: %r has no name" % (where, text))
    plain = " ".join(t for t in ty if t != "const")
    if "*" in ty:
        if ty[0] != "*" and not set(ty[ty.index("*"):]) - {"*", "const"}:
            return (ctypes.c_char_p if ty == ["const", "char", "*"] else ctypes.c_void_p), name
    elif plain in _BY_VALUE or (returns and plain == "void"):
        return _BY_VALUE.get(plain), name
    raise ValueError("%s %s: type %r is none of %s or a pointer" % (where, name, " ".join(ty), ", ".join(_BY_VALUE)))


def parse_header(text):
    """{name: [argument ctypes types]}, {name: restype} of every function a header's text declares.  Strict: once the
    comments, the preprocessor lines, the extern "C" braces and the typedefs are set aside, every statement must be a
    prototype made of the types above, with every parameter named."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^[ \t]*(#[^\n]*|extern\s+"C"\s*\{|\})[ \t]*$', " ", text, flags=re.M)
    text = re.sub(r"\btypedef\b[^;{}]*(\{[^{}]*\})?[^;{}]*;", " ", text)  # (a struct's name maps to no type: by value it is refused)
    argtypes, restypes = {}, {}
    *statements, rest = (" ".join(s.split()) for s in text.split(";"))
    for st in statements:
        head, paren, args = st.partition("(")
        if not paren or not args.endswith(")"):
            raise ValueError("header: not a function declaration: %r" % st[:120])
        restype, name = _declarator(head, "header: function", returns=True)
        if name in argtypes:
            raise ValueError("header: %s is declared twice" % name)
        args = args[:-1].strip()
        argtypes[name] = [] if args == "void" else [_declarator(a, "%s: parameter %d" % (name, i))[0]
                                                    for i, a in enumerate(args.split(","))]
        restypes[name] = restype
    if rest:
        raise ValueError("header: no ';' behind the last declaration: %r" % rest[:120])
    return argtypes, restypes


def _parse_headers():
    texts = []
    for path in HEADERS:
        if not os.path.exists(path):
            raise ImportError("samplenet_amd: %s not found. The ctypes prototypes are derived from it." % path)
        with open(path) as f:
            texts.append(f.read())
    return parse_header("".join(texts))


PROTOTYPES, RESTYPES = _parse_headers()  # name -> argument types, name -> return type


class SampleNetHipError(RuntimeError):
    pass


def bind(cdll, names=None):
    """Set argtypes / restype of the given entries (default: all) on a loaded build of the library."""
    for name in PROTOTYPES if names is None else names:
        try:
            fn = getattr(cdll, name)
        except AttributeError as e:
            raise ImportError("samplenet_amd: %s does not export %s (stale build?)" % (cdll._name, name)) from e
        fn.argtypes = PROTOTYPES[name]
        fn.restype = RESTYPES[name]
    return cdll


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "samplenet_amd: %s not found. Build it with `python samplenet_amd/build.py` (hipcc, gfx950). "
            "There is no CPU / eager fallback." % LIB_PATH)
    return bind(ctypes.CDLL(LIB_PATH))


lib = _load()
if lib.sn_abi_version() != 1:
    raise ImportError("samplenet_amd: ABI version mismatch in %s" % LIB_PATH)


def check(rc, what=""):
    if rc != 0:
        msg = lib.sn_last_error_string()
        raise SampleNetHipError("%s failed (code %d): %s" % (what or "samplenet_hip call", rc, (msg or b"").decode()))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


try:  # the current stream's handle without building a torch.cuda.Stream object (~0.3 us instead of ~4 us per lookup; the eager
    from torch._C import _cuda_getCurrentRawStream as _raw_stream  # module surface issues dozens of them per step)
except ImportError:  # pragma: no cover
    _raw_stream = None


def stream_of(t):
    """hipStream_t (as an int) of torch's current stream on tensor t's device."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream
