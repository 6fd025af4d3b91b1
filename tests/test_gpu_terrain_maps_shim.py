"""The C++ shim reaches oxc_generate_terrain_maps: tests/cpp/shim_terrain_maps.cpp runs ox::amd::terrain_generate_pass, terrain_derive_pass
and terrain_minmax_pass, one stage each, on the 33 x 17 map; the five images it writes equal the checker's."""
import struct

import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- TerrainMaps and the three passes with the reference's argument lists -- and
    links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_terrain_maps", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_three_passes_bake_the_maps(tmp_path):
    import terrain_maps_frames as TF
    from gpu_passes import same

    exe = shim_programs.build("shim_terrain_maps", tmp_path)
    res, pc = (33, 17), (3, 2)
    G, D = TF.engine(res)
    height_edit, splat_edit = TF.edits(res)
    g, d = TF.renderer_settings(G, D, res)
    (tmp_path / "params.bin").write_bytes(bytes(g.c()) + bytes(d.c()) + struct.pack("<2I", *pc))
    (tmp_path / "height_edit.bin").write_bytes(height_edit.tobytes())
    (tmp_path / "splat_edit.bin").write_bytes(splat_edit.tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "terrain maps ok" in p.stdout, p.stderr + p.stdout
    zero = {"heightmap": np.zeros((17, 33), np.uint16), "ridgemap": np.zeros((17, 33), np.uint16), "normalmap": np.zeros((17, 33, 2), np.uint16),
            "splatmap": np.zeros((17, 33), np.uint32), "height_edit": height_edit, "splat_edit": splat_edit, "patch_minmax": np.zeros((2, 3, 2), np.float32)}
    want = TF.want(G, D, res, pc, zero)
    for name in TF.OUTPUTS:
        same(shim_programs.read_out(tmp_path, name, want[name].dtype, want[name].shape), want[name], f"the shim's {name}")
