"""The one place in tests/ that holds a g++ command line for a host harness (tests only): the shared object a test loads, the stand-alone program a
test runs under AddressSanitizer and UBSan, and the ctypes call into the former."""
import ctypes
import os
import subprocess

import numpy as np

# -ffp-contract=off everywhere: a harness must round as the kernels' un-fused products do, whatever the host (on x86-64 without -march there is
# no fused multiply-add to contract to and the flag changes nothing; on a host that has one it would)
COMMON = ["-std=c++17", "-Wall", "-ffp-contract=off"]
_LIBS = {}


def _make(target, source, deps, flags):
    """rebuild when the target is missing or older than any of source + deps"""
    if not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in [source] + list(deps)):
        subprocess.run(["g++"] + flags + ["-o", target, source], check=True)
    return target


def shared(target, source, deps):
    """the shared object -> its ctypes.CDLL, one per path for the process"""
    path = os.path.abspath(_make(target, source, deps, ["-O2"] + COMMON + ["-shared", "-fPIC"]))
    if path not in _LIBS:
        _LIBS[path] = ctypes.CDLL(path)
    return _LIBS[path]


def program(target, source, deps, defines, extra=()):
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything) -> its path"""
    return _make(target, source, deps, ["-O1", "-g"] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                                  "-fno-omit-frame-pointer"] + ["-D" + d for d in defines] + list(extra))


def call(lib, name, restype, argtypes, *args):
    """lib.name(*args), its prototype set the first time.  A numpy array goes as its data pointer, None as a null pointer."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        fn.restype, fn.argtypes = restype, argtypes
    return fn(*(a.ctypes.data if isinstance(a, np.ndarray) else a for a in args))
