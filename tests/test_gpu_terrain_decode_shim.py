"""The C++ shim reaches oxc_decode_terrain: tests/cpp/shim_terrain_decode.cpp runs ox::amd::decode_terrain on the fixture's 17 x 9 frame over
the baked 24 x 20 map, every buffer distinct in size or content; the four attachments it writes equal the Python path's bytes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oxylus_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_program(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    L.build()
    exe = str(tmp_path / "shim_terrain_decode")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "oxylus_amd", "host"), os.path.join(ROOT, "tests", "cpp", "shim_terrain_decode.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "oxylus_amd"), "-loxcull", "-Wl,-rpath," + os.path.join(ROOT, "oxylus_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- TerrainDecodeContext and the free function -- and links to liboxcull.so."""
    p = subprocess.run([build_program(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_free_function_decodes_the_terrain(tmp_path, renderer):
    import torch

    import terrain_decode_frames as DF
    from gpu_passes import same

    exe = build_program(tmp_path)
    f = DF.golden_frame()
    h, w = f.inputs["splatmap"].shape
    params = (np.array([f.W, f.H], np.uint32).tobytes() + f.ipv.astype(np.float32).tobytes() + bytes(DF.renderer_terrain(f.T).c())
              + np.array([w, h, f.material_count], np.uint32).tobytes())
    assert len(params) == 8 + 64 + C.sizeof(L.TerrainData) + 12
    (tmp_path / "params.bin").write_bytes(params)
    for name, a in {**f.inputs, **f.init}.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "terrain decode ok" in p.stdout, p.stderr + p.stdout

    # the Python path: the same call through the renderer
    gs = DF.guards(f)
    renderer.decode_terrain(DF.context(f, gs))
    torch.cuda.synchronize()
    python = DF.got_of(gs, f)
    assert (python["albedo"] != f.init["albedo"]).sum() > 100 and (python["emissive"] != python["albedo"]).any()
    for name, want in python.items():
        got = np.frombuffer((tmp_path / f"{name}.out").read_bytes(), dtype=want.dtype).reshape(want.shape)
        same(got, want, f"the shim's {name}")
