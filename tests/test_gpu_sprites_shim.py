"""The C++ shim reaches oxc_draw_sprites and oxc_pick_sprite: tests/cpp/shim_sprites.cpp runs RendererInstance::draw_sprites in both formats and
the three stage sets, then RendererInstance::pick_sprite, on the golden 17 x 9 frame; what they write equals the fixture's bytes."""
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
    exe = str(tmp_path / "shim_sprites")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "oxylus_amd", "host"), os.path.join(ROOT, "tests", "cpp", "shim_sprites.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "oxylus_amd"), "-loxcull", "-Wl,-rpath," + os.path.join(ROOT, "oxylus_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- SpriteContext, SpritePickingContext and the two member functions -- and
    links to liboxcull.so."""
    p = subprocess.run([build_program(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_functions_draw_and_pick(tmp_path):
    import sprites_frames as SF
    import sprites_model as SM
    from gpu_passes import same

    exe = build_program(tmp_path)
    g = np.load(SF.GOLDEN)
    f = SF.golden_frame()
    W, H = f.extent
    both = g[f"vis_format1_stages{SM.ALL}"]
    ys, xs = np.nonzero(both != SM.EMPTY)
    pick = (int(xs[0]), int(ys[0]))
    (tmp_path / "params.bin").write_bytes(np.array([W, H, len(f.sprites), len(f.materials), len(f.transforms), *pick], np.uint32).tobytes())
    for name in ("sprites", "materials", "transforms", "depth", "pv", "color_format0", "color_format1"):
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(g["in_" + name]).tobytes())
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "sprites ok" in p.stdout, p.stderr + p.stdout
    out = lambda name, dtype: np.frombuffer((tmp_path / f"{name}.out").read_bytes(), dtype=dtype)  # noqa: E731
    for fmt in SF.FORMATS:
        for stages in SF.STAGES:
            tag = f"_format{fmt}_stages{stages}"
            same(out("depth" + tag, np.uint32).reshape(H, W), g["depth" + tag].view(np.uint32), "the shim's depth" + tag)
            if stages & SM.VIS:
                same(out("vis" + tag, np.uint32).reshape(H, W), g["vis" + tag], "the shim's vis" + tag)
            if stages & SM.COLOR:
                same(out("color" + tag, np.uint16 if fmt else np.uint32).reshape(g["color" + tag].shape), g["color" + tag], "the shim's color" + tag)
    assert int(out("pick", np.uint32)[0]) == int(both[pick[1], pick[0]]) != SM.EMPTY
