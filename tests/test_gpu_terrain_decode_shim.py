"""The C++ shim reaches oxc_decode_terrain: tests/cpp/shim_terrain_decode.cpp runs ox::amd::decode_terrain on the fixture's 17 x 9 frame over
the baked 24 x 20 map, every buffer distinct in size or content; the four attachments it writes equal the Python path's bytes."""
import ctypes as C

import numpy as np
import pytest

from oxylus_amd import lib as L

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- TerrainDecodeContext and the free function -- and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_terrain_decode", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_free_function_decodes_the_terrain(tmp_path, renderer):
    import torch

    import terrain_decode_frames as DF
    from gpu_passes import same

    exe = shim_programs.build("shim_terrain_decode", tmp_path)
    f = DF.golden_frame()
    h, w = f.inputs["splatmap"].shape
    params = (np.array([f.W, f.H], np.uint32).tobytes() + f.ipv.astype(np.float32).tobytes() + bytes(DF.renderer_terrain(f.T).c())
              + np.array([w, h, f.material_count], np.uint32).tobytes())
    assert len(params) == 8 + 64 + C.sizeof(L.TerrainData) + 12
    (tmp_path / "params.bin").write_bytes(params)
    for name, a in {**f.inputs, **f.init}.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "terrain decode ok" in p.stdout, p.stderr + p.stdout

    # the Python path: the same call through the renderer
    gs = DF.guards(f)
    renderer.decode_terrain(DF.context(f, gs))
    torch.cuda.synchronize()
    python = DF.got_of(gs, f)
    assert (python["albedo"] != f.init["albedo"]).sum() > 100 and (python["emissive"] != python["albedo"]).any()
    for name, want in python.items():
        same(shim_programs.read_out(tmp_path, name, want.dtype, want.shape), want, f"the shim's {name}")
