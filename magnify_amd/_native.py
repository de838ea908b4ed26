"""ctypes binding of the C-ABI hot-path library (``include/magnify_hip.h``).

The library is built in-tree by ``magnify_amd/csrc/Makefile`` (``__graft_entry__.build()``)
into ``magnify_amd/_lib/libmagnify_hip.so``.  There is NO CPU fallback: if the library is
missing every product entry point raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libmagnify_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "magnify_hip.h")


class NativeLibraryMissing(RuntimeError):
    pass


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}


def _ctype(decl: str, what: str):
    """ctypes type of one declared parameter or return type; every pointer is passed as an address."""
    if "*" in decl:
        return C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not words or words[0] not in _CTYPES or len(words) > 2:
        raise TypeError(f"{HEADER_PATH}: no ctypes mapping for `{decl.strip()}` in {what}")
    return _CTYPES[words[0]]


def _parse_header():
    """(name -> argtypes, name -> restype) of every `int|int64_t mg_*(...);` declared in the header, and name -> value
    of every `#define MG_NAME <integer or float literal>` (in parentheses or not, with or without an f suffix)."""
    if not os.path.exists(HEADER_PATH):
        raise NativeLibraryMissing(f"{HEADER_PATH} not found: the ctypes binding is read from it.  "
                                   "magnify_amd has no fallback table.")
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    defines = {}
    for name, number, is_float in re.findall(r"^[ \t]*#define[ \t]+(MG_\w+)[ \t]+\(?(-?\d+(\.\d*)?)f?\)?[ \t]*$", text, flags=re.M):
        defines[name] = float(number) if is_float else int(number)
    argtypes, restypes = {}, {}
    for ret, name, args in re.findall(r"\b(\w+)\s+(mg_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [] if args.strip() in ("", "void") else args.split(",")
        argtypes[name] = [_ctype(a, name) for a in args]
        restypes[name] = _ctype(ret, name)
    return argtypes, restypes, defines


# name -> argtypes / restype / value: the prototypes and the constants of include/magnify_hip.h, read from it
PROTOTYPES, RESTYPES, DEFINES = _parse_header()
MG_U8, MG_U16, MG_F32, MG_F64 = (DEFINES[k] for k in ("MG_U8", "MG_U16", "MG_F32", "MG_F64"))
MG_NO_EDGE, MG_SCORE_SKIPPED = DEFINES["MG_NO_EDGE"], DEFINES["MG_SCORE_SKIPPED"]

_lib = None


def lib():
    """The loaded library; raises loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C magnify_amd/csrc).  magnify_amd has no CPU fallback."
            )
        handle = C.CDLL(LIB_PATH)
        for name, argtypes in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = RESTYPES[name]
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc == -1:
        raise ValueError(f"{what}: invalid argument (MG_EINVAL)")
    raise RuntimeError(f"{what}: HIP launch failure (code {rc})")


def dtype_code(dtype) -> int:
    """MG_* code of a numpy/torch dtype (by name)."""
    name = str(dtype).replace("torch.", "")
    try:
        return {"uint8": MG_U8, "uint16": MG_U16, "float32": MG_F32, "float64": MG_F64}[name]
    except KeyError:
        raise TypeError(f"unsupported image dtype {dtype}; supported: uint8, uint16, float32, float64") from None


# ---- host tables ---------------------------------------------------------------------------


def circle_points(r: int, four_connected: bool = False) -> np.ndarray:
    n = lib().mg_circle_points(int(r), int(bool(four_connected)), None, 0)
    if n < 0:
        raise ValueError("radius must be non-negative")
    out = np.empty((n, 2), dtype=np.int32)
    lib().mg_circle_points(int(r), int(bool(four_connected)), out.ctypes.data, n)
    return out


def disk_halfwidths(r: int) -> np.ndarray:
    out = np.empty(2 * r + 1, dtype=np.int32)
    if lib().mg_disk_halfwidths(int(r), out.ctypes.data) < 0:
        raise ValueError("filled disk is undefined for r < 2 (reference utils.py:398-430)")
    return out


def cv_disk_halfwidths(r: int) -> np.ndarray:
    out = np.empty(r + 1, dtype=np.int32)
    if lib().mg_cv_disk_halfwidths(int(r), out.ctypes.data) < 0:
        raise ValueError("radius must be non-negative")
    return out


def perimeter_table(min_r: int, max_r: int):
    starts = np.empty(max_r - min_r + 2, dtype=np.int32)
    total = lib().mg_perimeter_table(int(min_r), int(max_r), None, None, starts.ctypes.data, 0)
    if total < 0:
        raise ValueError("bad radius range")
    rc = np.empty((total, 2), dtype=np.int32)
    expected = np.empty(total, dtype=np.float64)
    lib().mg_perimeter_table(int(min_r), int(max_r), rc.ctypes.data, expected.ctypes.data, starts.ctypes.data, total)
    return rc, expected, starts


def score_pair_table():
    """Bound tables of mg_score_circles_keyed: uint64 (27, 80), 8 signed bytes per pair of opposite points."""
    total = lib().mg_score_pair_table(None, 0)
    entries = np.zeros(total, dtype=np.uint64)
    check(min(lib().mg_score_pair_table(entries.ctypes.data, total), 0), "mg_score_pair_table")
    return entries.reshape(27, 80)


def score_pairs(r: int):
    """First points (dr, dc) of the pairs of opposite perimeter points of radius r, in table order."""
    n = lib().mg_score_pairs(int(r), None, 0)
    out = np.empty((n, 2), dtype=np.int32)
    lib().mg_score_pairs(int(r), out.ctypes.data, n)
    return out


def dedup_layout(h: int, w: int, min_r: int, max_r: int):
    """(tile_rows, tile_cols, n_layers, bitmap_words) of the circle de-duplication bitmap."""
    a, b = C.c_int(0), C.c_int(0)
    n, words = C.c_int64(0), C.c_int64(0)
    check(lib().mg_dedup_layout(h, w, min_r, max_r, C.byref(a), C.byref(b), C.byref(n), C.byref(words)), "mg_dedup_layout")
    return a.value, b.value, n.value, words.value
