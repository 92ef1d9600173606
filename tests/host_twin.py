"""The one compile recipe of the host twins under tests/hostcheck: the device source's scalar rules, compiled for the CPU as the
device compiles them (-ffp-contract=off)."""
import ctypes
import os
import subprocess

from conftest import ROOT


def build_shim(stem, directory, sanitize=False, std=None):
    """tests/hostcheck/<stem>_check.cpp -> ctypes library (the caller sets its argtypes); sanitize=True: the stand-alone program with
    -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded).  std: the -std= the twin is built with,
    None: the compiler's own."""
    src = os.path.join(ROOT, "tests", "hostcheck", stem + "_check.cpp")
    std = ["-std=" + std] if std else []
    if sanitize:
        exe = os.path.join(str(directory), stem + "_check_san")
        subprocess.check_call(["g++", "-O1", "-g", *std, "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
        return exe
    so = os.path.join(str(directory), "lib" + stem + "_check.so")
    subprocess.check_call(["g++", "-O3", *std, "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)
