"""The C++ shim reaches oxc_apply_pbr_atmosphere: tests/cpp/shim_atmosphere.cpp sets HasAtmosphere in gpu_scene_flags and calls
ox::amd::RendererInstance::apply_pbr on the 33 x 17 synthetic frame; the image it writes equals the checker's."""
import struct

import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_atmosphere", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_shim_takes_the_atmosphere_branch(tmp_path):
    import atmosphere_frames as AF
    import pbr_atmosphere_frames as PF
    from gpu_passes import same
    from oxylus_amd.synth import pack_lights
    from scenes import CAMERA, INV_PV, PBR_SUN, SUN_INTENSITY

    exe = shim_programs.build("shim_atmosphere", tmp_path)
    inp = PF.frame()
    H, W = inp["depth"].shape
    A = PF.atmosphere("far")
    sky = PF.sky_images(A, cube_size=32)  # the shim passes the engine's IBL_CUBE_RES
    lights = pack_lights(PF.TWO_LIGHTS).numpy()
    record = bytes(AF.renderer_atmosphere(A).c())
    assert len(record) == 136
    (tmp_path / "params.bin").write_bytes(struct.pack("<4I23f", W, H, 32, 0, *INV_PV, *CAMERA, *PBR_SUN, SUN_INTENSITY) + record)
    for name, data in dict(inp, lights=lights, **sky).items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(data).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "atmosphere branch ok" in p.stdout, p.stderr + p.stdout
    got = np.frombuffer((tmp_path / "final.bin").read_bytes(), dtype=np.uint32).reshape(H, W)
    same(got, PF.want(inp, PF.ALL_READ, A, sky, lights), "the shim's image")
