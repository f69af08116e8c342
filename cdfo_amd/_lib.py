"""ctypes binding of libcdfo_hip.so (declared in include/cdfo_hip.h).

There is no CPU fallback: if the library is missing this module raises at import time of the first call, and
every entry point's non-zero status becomes a RuntimeError."""
from __future__ import annotations

import ctypes as C
import os
import re

# torch first: its wheel bundles the HIP/HSA runtime (libamdhip64.so.7).  libcdfo_hip.so must bind to THAT copy --
# the streams and device pointers handed across the C-ABI come from it -- so it has to be in the process before
# our library's DT_NEEDED entries are resolved.  (Loading /opt/rocm's copy first leaves two HSA runtimes in one
# process and every launch fails with hipErrorNoDevice.)
import torch  # noqa: F401,E402

from . import switches  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = switches.get("CDFO_LIB_PATH") or os.path.join(_HERE, "lib", "libcdfo_hip.so")   # (developer A/B builds)

_lib = None


class CdfoError(RuntimeError):
    pass


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cdfo_hip.h")


def _header_text(path: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def _ctype(decl: str, where: str):
    """A C declaration that starts with its type -> the ctypes type (every pointer crosses as void*)."""
    if "*" in decl:
        return C.c_void_p
    for prefix, ct in (("long long", C.c_longlong), ("float", C.c_float), ("int", C.c_int)):
        if decl.startswith(prefix):
            return ct
    raise CdfoError(f"cannot map C type in {where}: {decl!r}")


def header_prototypes(path: str = HEADER_PATH):
    """Parse include/cdfo_hip.h -> {symbol: (restype, [argtypes])}; the header is the single source of truth."""
    protos = {}
    for m in re.finditer(r"(const char\*|long long|int)\s+(cdfo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text(path)):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        at = []
        if args and args != "void":
            decls = [" ".join(a.split()) for a in args.split(",")]
            # a double by value crosses only as an argument (adam.hip's hyper-parameters); cdfo_conv_args has none, and _ctype refuses it
            at = [C.c_double if "*" not in d and d.startswith("double") else _ctype(d, f"prototype of {name}") for d in decls]
        protos[name] = (C.c_char_p if ret.startswith("const char") else C.c_longlong if ret == "long long" else C.c_int, at)
    return protos


def header_conv_args_fields(path: str = HEADER_PATH):
    """Parse the body of `typedef struct { ... } cdfo_conv_args;` -> ctypes `_fields_`, in declaration order."""
    text = _header_text(path)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*cdfo_conv_args\s*;", text)
    if m is None:
        raise CdfoError(f"{path} does not define cdfo_conv_args")
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *more = (d.strip() for d in decl.split(","))      # `T a[N]` or `T a, b, c`
        head = re.fullmatch(r"(.*[\s*])(\w+(?:\[\w+\])?)", first)
        if head is None:
            raise CdfoError(f"cannot parse field of cdfo_conv_args: {decl!r}")
        ct = _ctype(head.group(1), "cdfo_conv_args")
        for item in (head.group(2), *more):
            f = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", item)
            if f is None:
                raise CdfoError(f"cannot parse field of cdfo_conv_args: {decl!r}")
            name, dim = f.groups()
            if dim is not None and not dim.isdigit():
                d = re.search(rf"#define\s+{dim}\s+(\d+)\s", text)
                if d is None:
                    raise CdfoError(f"array bound {dim} of cdfo_conv_args.{name} is not defined in {path}")
                dim = d.group(1)
            fields.append((name, ct if dim is None else ct * int(dim)))
    return fields


class ConvArgs(C.Structure):
    """ctypes mirror of cdfo_conv_args, derived from the header; lib() checks its size against the built library's."""
    _fields_ = header_conv_args_fields()


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CdfoError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -m cdfo_amd.build`).  There is no CPU fallback for the product path.")
        switches.check_hip_environment()      # a malformed switch of the library's own is an error here, not a silent default
        loaded = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in header_prototypes().items():
            fn = getattr(loaded, name)        # AttributeError here = header/library mismatch: fail loudly
            fn.restype = restype
            fn.argtypes = argtypes
        if loaded.cdfo_sizeof_conv_args() != C.sizeof(ConvArgs):
            raise CdfoError(f"{LIB_PATH} was built with sizeof(cdfo_conv_args) = {loaded.cdfo_sizeof_conv_args()}, "
                            f"{HEADER_PATH} gives {C.sizeof(ConvArgs)}: rebuild the library")
        _lib = loaded
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        kind = {-1: "invalid argument", -2: "misaligned pointer/pitch"}.get(status, f"hipError_t {status}")
        raise CdfoError(f"{what} failed: {kind}")


def _vp(t) -> C.c_void_p:
    """A tensor's device pointer, or NULL for None, as a C-ABI pointer argument."""
    return C.c_void_p(None if t is None else t.data_ptr())
