"""The C++ shim reaches oxc_apply_terrain_brush: tests/cpp/shim_terrain_brush.cpp runs ox::amd::apply_terrain_brush -- trace, apply and the
three regional passes with the reference's dispatch sizes -- on the 24 x 20 map; what it writes equals the Python path's bytes."""
import dataclasses

import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- TerrainBrushContext and the free function -- and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_terrain_brush", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_free_function_runs_the_edit_step(tmp_path, renderer):
    import torch

    import terrain_brush_frames as BF
    import terrain_brush_model as TB
    import terrain_maps_frames as TF
    from gpu_passes import same

    exe = shim_programs.build("shim_terrain_brush", tmp_path)
    res, pc = BF.GOLDEN_SHAPE
    G, D = TF.engine(res)
    he, se = BF.edits(res)
    images = TF.want(G, D, res, pc, TF.initial(res, pc, he, se))  # a baked map with earlier strokes
    B = BF.params(res, pc, (-300.0, 420.0, -150.0), (0.6, -0.7, 0.35), mode=TB.SMOOTH, radius_texels=2.5, strength=0.75)
    g, d = TF.renderer_settings(G, D, res)
    (tmp_path / "params.bin").write_bytes(bytes(BF.renderer_params(B).c()) + bytes(g.c()) + bytes(d.c()))
    for name in TF.IMAGES:
        (tmp_path / f"{name}.bin").write_bytes(images[name].tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "terrain brush ok" in p.stdout, p.stderr + p.stdout

    # the Python path: the same calls through the renderer
    gs = TF.guards(images)
    records = BF.guards({"hit": np.zeros(4, np.uint32), "region": np.zeros(4, np.uint32)}, ("hit", "region"))
    renderer.apply_terrain_brush(BF.context(B, {"heightmap": gs["heightmap"], "height_edit": gs["height_edit"], "splat_edit": gs["splat_edit"], **records}))
    derive_texels = 2 * int(np.ceil(np.float32(B.radius_texels) + np.float32(1.0))) + 1
    derive_patches = int(np.ceil(np.float32(derive_texels) / min(np.float32(res[0]) / np.float32(pc[0]), np.float32(res[1]) / np.float32(pc[1])))) + 1
    rebake = TF.context(G, D, res, pc, gs, region=records["region"].tensor, dispatch_texels=(derive_texels,) * 2, dispatch_patches=(derive_patches,) * 2)
    for stage in (TF.TM.GENERATE, TF.TM.DERIVE, TF.TM.MINMAX):
        renderer.generate_terrain_maps(dataclasses.replace(rebake, stages=stage))
    torch.cuda.synchronize()
    python = {**TF.got_of(gs, images), **BF.got_of(records, {"hit": np.zeros(4, np.uint32), "region": np.zeros(4, np.uint32)})}
    assert python["hit"][3] == 1 and (python["height_edit"] != images["height_edit"]).any() and (python["heightmap"] != images["heightmap"]).any()
    for name, want in python.items():
        same(shim_programs.read_out(tmp_path, name, want.dtype, want.shape), want, f"the shim's {name}")
