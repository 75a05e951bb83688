"""Build + load the CPU emulation of the kernel source (tests only; see ccsd_amd/csrc/ccsd_rt.h)."""
import glob
import os
import subprocess

from ccsd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "ccsd_emu.cpp")
OUT = os.path.join(ROOT, "tests", "emu", "_build", "libccsd_emu.so")
CSRC = os.path.join(ROOT, "ccsd_amd", "csrc")
DEPS = [SRC] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))

_emu = None


def emu_library() -> _lib.Library:
    global _emu
    if _emu is None:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        stale = not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS)
        if stale:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCCSD_EMU", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                                   SRC, "-o", OUT])
        _emu = _lib.Library(OUT, is_hip=False)
    return _emu


PROBE_SRC = os.path.join(ROOT, "tests", "emu", "ccsd_probe.cpp")
_probe = {}


def probe_library(csrc: str = CSRC, defines=()):
    """tests/emu/ccsd_probe.cpp built against the kernel source in `csrc` (ctypes handle): the device helpers of the noise stream
    on the host.  Another `csrc` / `defines` builds a library of its own beside it (a kernel source to compare against)."""
    import ctypes
    import hashlib

    key = (os.path.abspath(csrc), tuple(defines))
    if key not in _probe:
        tag = "" if key == (CSRC, ()) else "_" + hashlib.sha1(repr(key).encode()).hexdigest()[:10]
        out = os.path.join(ROOT, "tests", "emu", "_build", f"libccsd_probe{tag}.so")
        deps = [PROBE_SRC] + glob.glob(os.path.join(csrc, "*.h"))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCCSD_EMU", *[f"-D{d}" for d in defines], "-fPIC", "-shared",
                                   "-Wno-unknown-pragmas", "-I", csrc, PROBE_SRC, "-o", out])
        _probe[key] = ctypes.CDLL(out)
    return _probe[key]
