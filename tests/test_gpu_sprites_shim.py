"""The C++ shim reaches oxc_draw_sprites and oxc_pick_sprite: tests/cpp/shim_sprites.cpp runs RendererInstance::draw_sprites in both formats and
the three stage sets, then RendererInstance::pick_sprite, on the golden 17 x 9 frame; what they write equals the fixture's bytes."""
import functools

import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- SpriteContext, SpritePickingContext and the two member functions -- and
    links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_sprites", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_functions_draw_and_pick(tmp_path):
    import sprites_frames as SF
    import sprites_model as SM
    from gpu_passes import same

    exe = shim_programs.build("shim_sprites", tmp_path)
    g = np.load(SF.GOLDEN)
    f = SF.golden_frame()
    W, H = f.extent
    both = g[f"vis_format1_stages{SM.ALL}"]
    ys, xs = np.nonzero(both != SM.EMPTY)
    pick = (int(xs[0]), int(ys[0]))
    (tmp_path / "params.bin").write_bytes(np.array([W, H, len(f.sprites), len(f.materials), len(f.transforms), *pick], np.uint32).tobytes())
    for name in ("sprites", "materials", "transforms", "depth", "pv", "color_format0", "color_format1"):
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(g["in_" + name]).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "sprites ok" in p.stdout, p.stderr + p.stdout
    out = functools.partial(shim_programs.read_out, tmp_path)
    for fmt in SF.FORMATS:
        for stages in SF.STAGES:
            tag = f"_format{fmt}_stages{stages}"
            same(out("depth" + tag, np.uint32, (H, W)), g["depth" + tag].view(np.uint32), "the shim's depth" + tag)
            if stages & SM.VIS:
                same(out("vis" + tag, np.uint32, (H, W)), g["vis" + tag], "the shim's vis" + tag)
            if stages & SM.COLOR:
                same(out("color" + tag, np.uint16 if fmt else np.uint32, g["color" + tag].shape), g["color" + tag], "the shim's color" + tag)
    assert int(out("pick", np.uint32, 1)[0]) == int(both[pick[1], pick[0]]) != SM.EMPTY
