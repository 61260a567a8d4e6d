"""ctypes binding of libmhe_hip.so (the C ABI declared in include/mhe.h).

There is NO fallback: if the shared library is missing or a symbol cannot be
bound, importing the product path fails loudly."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmhe_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mhe.h")


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("B", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "dtype", "relu_in", "relu_out", "tile", "res_half")]


class WgradItem(C.Structure):
    """mhe_wgrad_item of include/mhe.h: one problem of mhe_conv_wgrad_multi_nhwc"""
    _fields_ = [("d", ConvDesc), ("x", C.c_void_p), ("gy", C.c_void_p), ("dw", C.c_void_p), ("ldw", C.c_int)]


_SCALARS = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "unsigned long long": C.c_ulonglong}


def _ctype(decl, text, ret=False):
    """the ctypes type of one named parameter, or of the return type, of `decl`"""
    words = text.replace("const ", " ").replace("*", " * ").split()
    if "*" not in words:
        kind = " ".join(words if ret else words[:-1])
        if kind in _SCALARS:
            return _SCALARS[kind]
    elif not ret:
        return C.POINTER(ConvDesc) if words[0] == "mhe_conv_desc" else C.c_void_p
    elif words == ["char", "*"]:
        return C.c_char_p
    raise ImportError(f"include/mhe.h: cannot bind `{text.strip()}` of `{decl}`")


def _signatures(header):
    """name -> (restype, argtypes) of every function include/mhe.h declares.  A declaration that does not parse fails the import."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    src = re.sub(r"^\s*#.*$|extern\s+\"C\"\s*\{", " ", src, flags=re.M)
    table = {}
    for stmt in src.split(";"):
        if not re.search(r"\bmhe_\w+\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"(.+?)\b(mhe_\w+) ?\((.*)\)", decl)
        if m is None:
            raise ImportError(f"include/mhe.h: cannot parse `{decl}`")
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        table[m.group(2)] = (_ctype(decl, m.group(1), ret=True), [_ctype(decl, p) for p in params])
    return table


with open(HEADER_PATH) as _f:
    SIGNATURES = _signatures(_f.read())

_lib = None
ABI_VERSION = 4          # MHE_ABI_VERSION of include/mhe.h


class MheError(RuntimeError):
    pass


def lib():
    """Load (once) and return the bound library; raise if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MheError(
                f"{LIB_PATH} is missing: build it with `python -m mhentropy_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm ships its own HIP runtime; it has to be in the process BEFORE this library is loaded, otherwise the library
        # binds the system runtime and its kernels later find "no ROCm-capable device" next to torch's tensors
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the export is absent
            fn.restype, fn.argtypes = res, args
        if L.mhe_abi_version() != ABI_VERSION:       # struct layouts (ConvDesc) below are this version's
            raise MheError(f"{LIB_PATH} has ABI version {L.mhe_abi_version()}, these bindings are for {ABI_VERSION}: rebuild "
                           "(`python -m mhentropy_amd.build`)")
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise MheError(f"{what} failed ({status}): {lib().mhe_last_error().decode()}")
