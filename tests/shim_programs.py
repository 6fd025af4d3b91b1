"""The C++ test programs of tests/cpp/, each written against oxylus_amd/host/RendererInstance.hpp on top of tests/cpp/shim_io.hpp: how one is
compiled and run, and how the `<name>.out` files it leaves are read.  The compiler line is here once, for every test_*_shim module."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oxylus_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, tmp_path):
    """tests/cpp/<name>.cpp compiled with plain g++ against the shim header and linked to liboxcull.so; the path of the program."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    L.build()
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "oxylus_amd", "host"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "oxylus_amd"), "-loxcull", "-Wl,-rpath," + os.path.join(ROOT, "oxylus_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True)


def read_out(tmp_path, name, dtype, shape):
    return np.frombuffer((tmp_path / f"{name}.out").read_bytes(), dtype=dtype).reshape(shape)
