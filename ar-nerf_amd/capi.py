"""The C ABI as Python sees it, read from include/ngp_amd.h: the header is the
only description of libngp_amd.so's entry points and constants (the .hip
definitions are held to it by the compiler; nothing is retyped here).

FUNCS    name -> (restype, argtypes) of every declared function
C        every integer `#define NGP_*` and every enum member
declare  sets restype / argtypes on a loaded library

A declaration this parser cannot map raises at import: it never guesses.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_uint32, c_void_p

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngp_amd.h")

_SCALARS = {"int": c_int, "int64_t": ctypes.c_int64, "float": c_float, "double": ctypes.c_double,
            "uint32_t": c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "unsigned long long": ctypes.c_ulonglong}


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
        return {"ngp_hashgrid_t": POINTER(ngp_hashgrid_t), "char": c_char_p}.get(base, c_void_p)
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


def declare(L, strict=True):
    """Set restype and argtypes of every header function on the CDLL `L`.
    strict: a function L does not export raises AttributeError; otherwise it
    is skipped (libraries built from a part of the sources)."""
    for name, (restype, argtypes) in FUNCS.items():
        if strict or hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
