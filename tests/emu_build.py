"""Builds the CPU emulator libraries of tests/emu when they are stale -- TEST INFRASTRUCTURE ONLY.  What a library depends on is
what the compiler read: g++ -MMD writes the list next to the library (<library>.d), and the next call compares against it."""
import os
import subprocess

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def _deps(dfile):
    """The prerequisites of a make rule `target: a b \\ c ...` as g++ -MMD writes it, or None when there is no such file."""
    if not os.path.exists(dfile):
        return None
    return open(dfile).read().replace("\\\n", " ").split(":", 1)[1].split()


def build(src, lib, flags=(), force=False):
    """tests/emu/<src> -> tests/emu/<lib> with g++ <flags>, if the library is missing or older than anything it was compiled from;
    returns the library's path."""
    src, lib = os.path.join(EMU, src), os.path.join(EMU, lib)
    deps = _deps(lib + ".d")
    if force or deps is None or not os.path.exists(lib) or \
            any(not os.path.exists(d) or os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-std=c++20", *flags, "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-MMD", "-MF", lib + ".d",
                               "-o", lib, src], cwd=EMU)
    return lib
