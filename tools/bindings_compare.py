#!/usr/bin/env python3
"""Compares the ctypes signatures revision REV's bitnet-rs_amd/__init__.py set by hand with the ones this tree derives from the headers.

    python tools/bindings_compare.py REV

REV's __init__.py is executed with ctypes.CDLL replaced by a recorder that stores every argtypes / restype assignment; its constructors
and every method that assigns one are driven with stand-in arguments.  No library is loaded and no GPU is touched.  Per symbol it prints
`same`, or the difference in parameter count, in the class of a parameter or of the return (every pointer class counts as "pointer").
Exit status 0 when nothing differs apart from the two expected deviations: a pointer-to-scalar class (POINTER(c_float), ...) that is now
c_void_p, and a symbol REV never bound that is bound now."""
import ctypes as C
import importlib
import inspect
import linecache
import os
import subprocess
import sys
import types
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "bitnet-rs_amd"


class Fn:
    """one symbol of a recorded library: remembers what is assigned to it, returns 0 (1 from a *_create*, whose result is a handle)"""

    def __init__(self, name, log):
        self.__dict__.update(_name=name, _log=log)

    def __setattr__(self, key, value):
        self._log.setdefault(self._name, {})[key] = value

    def __call__(self, *args):
        return 1 if "create" in self._name else 0


class Recorder:
    log = {}

    def __init__(self, name, mode=0):
        self._name = name

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = Fn(name, Recorder.log)
        self.__dict__[name] = fn
        return fn


def record(rev: str) -> dict:
    """every {symbol: {"argtypes": ..., "restype": ...}} REV's bindings assign"""
    src = subprocess.run(["git", "show", f"{rev}:{PKG}/__init__.py"], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    mod = types.ModuleType("_bindings_rev")
    mod.__file__ = os.path.join(ROOT, PKG, "__init__.py")
    mod.__package__, mod.__path__ = mod.__name__, [os.path.join(ROOT, PKG)]  # a relative import in REV finds this tree's module
    sys.modules[mod.__name__] = mod
    here = os.path.abspath(__file__)  # any existing file: the constructors only ask whether the library is there
    with mock.patch.object(C, "CDLL", Recorder), mock.patch("os.makedirs"):
        shown = f"<{rev}:{PKG}/__init__.py>"
        linecache.cache[shown] = (len(src), None, src.splitlines(True), shown)  # inspect.getsource below reads REV's text, not this tree's
        exec(compile(src, shown, "exec"), mod.__dict__)
        mod.LIB_PATH = here
        mod._lib = mod.HipLib(here)  # load() hands this out and never imports torch
        cfg = types.SimpleNamespace(asdict=lambda: dict.fromkeys([n for n, _ in mod.HostConfig._fields_], 1), vocab=1, hidden=1)
        objects = [mod._lib, mod.GgufFile(lib_path=here), mod.HostDecoder(cfg, path=here), mod.HostBatch(1, path=here)]
        mod.blake3_hex(b"")
        mod.host_device_bytes()
        for obj in objects:
            for name, method in inspect.getmembers(obj, inspect.ismethod):
                text = inspect.getsource(method) if name != "__init__" else ""
                if ".argtypes" in text or ".restype" in text:
                    try:  # the assignment stands at the head of the method; what follows may refuse the stand-ins
                        method(*[mock.MagicMock() for p in inspect.signature(method).parameters.values() if p.default is p.empty])
                    except Exception:  # noqa: BLE001
                        pass
    return Recorder.log


def kind(cls) -> str:
    if cls is None:
        return "void"
    if cls in (C.c_void_p, C.c_char_p) or issubclass(cls, C._Pointer):
        return "pointer"
    return cls.__name__


def is_struct_pointer(cls) -> bool:
    return cls is not None and issubclass(cls, C._Pointer) and issubclass(cls._type_, C.Structure)


def main() -> int:
    rev = sys.argv[1]
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    protos = pkg.cproto.prototypes(open(pkg.HEADER_PATH).read(), "bitnet_hip_") + pkg.host_prototypes()
    old = record(rev)
    bad, new, loosened = 0, [], 0
    for name, ret, params in protos:
        args = [pkg.cproto.ctype(t, pkg.C_STRUCTS, name) for t, _ in params]
        res = None if ret == "void" else pkg.cproto.ctype(ret, {}, name)
        was = old.pop(name, None)
        if was is None:
            new.append(name)
            print(f"{name}: newly bound ({len(args)} parameters, returns {kind(res)})")
            continue
        diffs, notes = [], []
        if "argtypes" in was:
            a = list(was["argtypes"])
            if len(a) != len(args):
                diffs.append(f"{len(a)} parameters, the header has {len(args)}")
            for i, (x, y) in enumerate(zip(a, args)):
                if kind(x) != kind(y) or (is_struct_pointer(x) and x.__name__ != y.__name__):
                    diffs.append(f"parameter {i}: {x.__name__} -> {y.__name__}")
                elif x.__name__ != y.__name__:  # REV's Structure classes are its own objects: held by name
                    notes.append(f"{i}: {x.__name__} -> {y.__name__}")
        else:
            notes.append("argtypes were unset")
        r = was.get("restype", C.c_int)  # ctypes' default
        if kind(r) != kind(res) and not ("restype" not in was and res is None):  # an unset restype on a void function read a register nobody used
            diffs.append(f"return: {kind(r)} -> {kind(res)}")
        if diffs:
            bad += 1
            print(f"{name}: DIFFERENT: " + "; ".join(diffs))
        else:
            loosened += bool(notes)
            print(f"{name}: same" + (f"  ({'; '.join(notes)})" if notes else ""))
    for name in sorted(old):  # bound by REV, declared by no header of this tree
        bad += 1
        print(f"{name}: DIFFERENT: bound by {rev}, declared by no header")
    print(f"{len(protos)} prototypes: {len(protos) - bad - len(new)} same ({loosened} of them with a pointer class that is c_void_p now or argtypes "
          f"that were unset), {len(new)} newly bound, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
