"""C prototypes read from the headers, and ctypes signatures derived from them.

The headers (include/bitnet_hip.h, the extern "C" tails of host/*.hpp) are the only statement of a prototype: prototypes() parses them,
bind() sets argtypes / restype on a loaded library from what it found.  tools/gen_rust_extern.py maps the same tuples to Rust.
"""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
           "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "unsigned long long": C.c_ulonglong, "bitnet_hip_weights_t": C.c_uint64,
           "bitnet_host_allgather_fn": C.c_void_p}  # the function-pointer typedef: callers pass cast(callback, c_void_p)


def prototypes(text: str, prefix: str) -> list[tuple[str, str, list[tuple[str, str]]]]:
    """(name, return type, [(parameter type, parameter name), ...]) of every `prefix...(...);` declaration, in order.  Comments and
    preprocessor lines are dropped first; an array parameter `T x[n]` is reported as the pointer it decays to, `T *`."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    out = []
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(%s[a-z0-9_]+)\s*\(([^()]*)\)\s*;" % re.escape(prefix), text):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        params = []
        for a in ([] if args in ("", "void") else args.split(",")):
            a, n_arr = re.subn(r"\s*\[[^\]]*\]", "", a.strip())
            mm = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a, flags=re.S)
            if not mm or not mm.group(1).strip():
                raise ValueError(f"{name}: cannot read parameter '{a}' (a parameter needs a type and a name)")
            params.append((" ".join(mm.group(1).split()) + " *" * n_arr, mm.group(2)))
        out.append((name, ret, params))
    return out


def ctype(c: str, structs: dict, where: str = "?"):
    """The ctypes class of one C type: char pointers c_char_p, a pointer to a struct of `structs` (C name -> ctypes.Structure) POINTER of it,
    every other pointer (opaque handles, tables, device memory) c_void_p, scalars through SCALARS.  Anything else raises and names `where`."""
    stars = c.count("*")
    base = " ".join(re.sub(r"\b(?:const|struct)\b|\*", " ", c).split())
    if stars == 0:
        if base not in SCALARS:
            raise TypeError(f"{where}: no ctypes mapping for the C type '{c}'")
        return SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    return C.c_void_p


def bind(cdll, protos, structs: dict) -> None:
    """argtypes and restype of every prototype, set on `cdll` when the library is loaded and never on first use: a pointer that goes
    through ctypes' default int conversion is cut to 32 bits (this crashed a process once).  A declared symbol the library does not
    export raises AttributeError here."""
    for name, ret, params in protos:
        f = getattr(cdll, name)
        f.argtypes = [ctype(t, structs, name) for t, _ in params]
        f.restype = None if ret == "void" else ctype(ret, {}, name)
