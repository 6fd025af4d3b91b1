"""The C++ shim reaches oxc_apply_debug_view: tests/cpp/shim_debug_view.cpp runs RendererInstance::apply_debug_view under the fourteen main
views on the golden 17 x 9 frame; the image each view writes equals the fixture's bytes."""
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
    exe = str(tmp_path / "shim_debug_view")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "oxylus_amd", "host"), os.path.join(ROOT, "tests", "cpp", "shim_debug_view.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "oxylus_amd"), "-loxcull", "-Wl,-rpath," + os.path.join(ROOT, "oxylus_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- DebugContext and the member function -- and links to liboxcull.so."""
    p = subprocess.run([build_program(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_function_draws_the_fourteen_views(tmp_path):
    import debug_view_frames as DF
    import debug_view_model as DV
    from gpu_passes import same

    exe = build_program(tmp_path)
    g = np.load(DF.GOLDEN)
    f = DF.golden_frame()
    W, H = f.extent
    params = np.array([W, H, len(f.meshlet_instances), len(f.mesh_instances), len(f.meshes)], np.uint32).tobytes() + np.float32(f.heatmap_scale).tobytes()
    (tmp_path / "params.bin").write_bytes(params)
    for name in DF.IMAGES + DF.RECORDS:
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(g["in_" + name]).tobytes())
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "debug views ok" in p.stdout, p.stderr + p.stdout
    for view in DV.MAIN_VIEWS:
        got = np.frombuffer((tmp_path / f"view{view}.out").read_bytes(), dtype=np.uint16).reshape(H, W, 4)
        same(got, g["out_" + DV.NAMES[view]], f"the shim's {DV.NAMES[view]}")
