"""The C++ shim reaches oxc_draw_terrain: tests/cpp/shim_terrain_draw.cpp runs RendererInstance::draw_terrain_for_visbuffer on a 33 x 19 frame
over the baked 24 x 20 map with projection_scale from the C++ terrain_projection_scale; the image and both resolves equal the Python
path's bytes, whose projection_scale comes from the Python twin, and the checker's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oxylus_amd import lib as L

import shim_programs

RESOLUTION_Y, FOV = 19.0, 53.13


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- the member and the projection-scale helper -- and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_terrain_draw", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_draws_the_terrain(tmp_path, renderer):
    import torch

    import terrain_decode_frames as DF
    import terrain_draw_frames as FR
    import terrain_draw_model as TM
    from gpu_passes import same
    from oxylus_amd.renderer import terrain_projection_scale

    exe = shim_programs.build("shim_terrain_draw", tmp_path)
    f = FR.frame((33, 19), (3, 2), "oblique", target_edge_pixels=2.0)  # with clear: the image before is poison to both paths
    scale = terrain_projection_scale(RESOLUTION_Y, FOV)
    assert scale == TM.projection_scale(RESOLUTION_Y, FOV)
    f = dataclasses.replace(f, cam=dataclasses.replace(f.cam, projection_scale=scale))
    h, w = f.heightmap.shape
    params = (np.array([f.W, f.H, 1, len(f.visible)], np.uint32).tobytes() + f.cam.projection_view.astype(np.float32).tobytes()
              + np.array(list(f.cam.position) + [f.cam.near_clip], np.float32).tobytes() + np.array([RESOLUTION_Y, FOV], np.float64).tobytes()
              + bytes(DF.renderer_terrain(f.T).c()) + np.array([w, h, 0], np.uint32).tobytes())
    assert len(params) == 16 + 64 + 16 + 16 + C.sizeof(L.TerrainData) + 12
    (tmp_path / "params.bin").write_bytes(params)
    for name, a in (("heightmap", f.heightmap), ("visible", f.visible), ("draw_cmd", f.draw_cmd), ("visdepth", f.before)):
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "terrain draw ok" in p.stdout, p.stderr + p.stdout
    assert np.float32(float(p.stdout.split("terrain draw ok")[1].split()[0])) == np.float32(scale)  # nine digits name a binary32: the C++ helper's value, rounded once

    python = FR.run(renderer, f, "the Python path")  # ... which is the checker's image
    torch.cuda.synchronize()
    assert (python["vis"] == TM.VIS).any() and (python["visdepth"] != f.before).any()
    for name, want in python.items():
        same(shim_programs.read_out(tmp_path, name, want.dtype, want.shape), want, f"the shim's {name}")
