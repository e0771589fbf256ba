"""The C ABI as Python sees it, read from include/ngp_amd.h: the header is the
only description of libngp_amd.so's entry points and constants (the .hip
definitions are held to it by the compiler; nothing is retyped here).

FUNCS    name -> (restype, argtypes) of every declared function
C        every integer `#define NGP_*` and every enum member
POINTER_TO  pointee type -> the argtype of a `T*` parameter: it takes a tensor
         (dtype, contiguity and device checked before the call) or anything
         c_void_p takes
declare  sets restype / argtypes (and an errcheck on status returns) on a
         loaded library

A declaration this parser cannot map raises at import: it never guesses.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_uint32, c_void_p

import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngp_amd.h")

_SCALARS = {"int": c_int, "int64_t": ctypes.c_int64, "float": c_float, "double": ctypes.c_double,
            "uint32_t": c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "unsigned long long": ctypes.c_ulonglong}


# the project keeps unsigned words in signed tensors of the same width; void: any dtype
_DTYPES = {"float": torch.float32, "int64_t": torch.int64, "uint64_t": torch.int64, "int32_t": torch.int32,
           "uint32_t": torch.int32, "uint8_t": torch.uint8, "void": None}
# int-returning functions whose return is a value, not a status (declare's errcheck skips them)
INT_VALUES = {"ngp_probe_count"}


class _TensorPointer:
    """argtypes entry of a `T*` parameter.  A tensor is checked -- dtype,
    contiguous, on the device, in this order -- and passed as its data_ptr();
    a TypeError here reaches the caller as ctypes.ArgumentError with the
    argument's position, and the C function is not entered.  Anything else
    (None, int, c_void_p, a ctypes array, byref) is c_void_p's to convert."""
    pointee = dtype = None

    @classmethod
    def from_param(cls, x):
        if not isinstance(x, torch.Tensor):
            return c_void_p.from_param(x)
        if cls.dtype is not None and x.dtype != cls.dtype:
            raise TypeError(f"{cls.pointee}* takes a {cls.dtype} tensor, got {x.dtype}")
        if not x.is_contiguous():
            raise TypeError(f"{cls.pointee}* takes a contiguous tensor, got strides {tuple(x.stride())} "
                            f"for shape {tuple(x.shape)}")
        if not x.is_cuda:
            raise TypeError(f"{cls.pointee}* takes a CUDA tensor, got one on {x.device}")
        return c_void_p(x.data_ptr())


POINTER_TO = {base: type(base + "_p", (_TensorPointer,), {"pointee": base, "dtype": dtype})
              for base, dtype in _DTYPES.items()}


def _read(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def _constants(text):
    out = {}
    define = r"^[ \t]*#[ \t]*define[ \t]+(NGP_\w+)[ \t]+\(?[ \t]*(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*\)?[ \t]*$"
    for name, val in re.findall(define, text, re.M):
        out[name] = int(val, 0)
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        nxt = 0
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, _, val = (s.strip() for s in item.partition("="))
            out[name] = nxt = int(val, 0) if val else nxt
            nxt += 1
    return out


def _ctype(decl, func, named):
    words = decl.replace("*", " * ").split()
    words = [w for w in words if w != "const"]
    if "*" in words:
        base = " ".join(words[:words.index("*")])
        if base in ("ngp_hashgrid_t", "char"):
            return POINTER(ngp_hashgrid_t) if base == "ngp_hashgrid_t" else c_char_p
        if base not in POINTER_TO:
            raise TypeError(f"{func}: no ctypes mapping for `{decl.strip()}`")
        return POINTER_TO[base]
    base = " ".join(words[:-1] if named and len(words) > 1 else words)
    if base not in _SCALARS:
        raise TypeError(f"{func}: no ctypes mapping for `{decl.strip()}`")
    return _SCALARS[base]


def _functions(text):
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(ngp_\w+)\s*\(([^()]*)\)\s*;", text):
        name, params = m.groups()
        ret = text[max(text.rfind(c, 0, m.start()) for c in ";{}") + 1:m.start()]  # back to the statement's start
        args = [] if params.strip() in ("", "void") else [_ctype(p, name, True) for p in params.split(",")]
        out[name] = (_ctype(ret, name, False), args)
    lost = set(re.findall(r"\b(ngp_\w+)\s*\(", text)) - set(out)
    if lost:
        raise TypeError(f"declarations not understood: {sorted(lost)}")
    return out


def parse(path):
    """-> (FUNCS, C) of the header at `path`"""
    text = _read(path)
    return _functions(text), _constants(text)


_TEXT = _read(HEADER)
C = _constants(_TEXT)


class ngp_hashgrid_t(ctypes.Structure):
    _fields_ = [("n_levels", c_int), ("scales", c_float * C["NGP_MAX_LEVELS"]), ("res", c_uint32 * C["NGP_MAX_LEVELS"]),
                ("offsets", c_uint32 * (C["NGP_MAX_LEVELS"] + 1)), ("sizes", c_uint32 * C["NGP_MAX_LEVELS"]),
                ("xyz_min", c_float * 3), ("xyz_max", c_float * 3)]


FUNCS = _functions(_TEXT)
del _TEXT


def declare(L, strict=True, errcheck=None):
    """Set restype and argtypes of every header function on the CDLL `L`.
    strict: a function L does not export raises AttributeError; otherwise it
    is skipped (libraries built from a part of the sources).  errcheck
    (ctypes': (result, func, args) -> result) is set on every function that
    returns a status: `int`, but for INT_VALUES."""
    for name, (restype, argtypes) in FUNCS.items():
        if strict or hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
            if errcheck is not None and restype is c_int and name not in INT_VALUES:
                f.errcheck = errcheck
