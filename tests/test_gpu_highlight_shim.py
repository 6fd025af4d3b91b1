"""The C++ shim reaches oxc_pick_transform and oxc_apply_highlight: tests/cpp/shim_highlight.cpp runs RendererInstance::pick_transform and
RendererInstance::apply_highlight, the mask and then the composite in the three formats and modes, on the golden 17 x 9 frame; what they
write equals the fixture's bytes."""
import functools

import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- PickingContext, HighlightContext and the two member functions -- and links
    to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_highlight", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_functions_pick_mask_and_composite(tmp_path):
    import highlight_frames as HF
    from gpu_passes import same

    exe = shim_programs.build("shim_highlight", tmp_path)
    g = np.load(HF.GOLDEN)
    f = HF.golden_frame()
    W, H = f.extent
    ys, xs = np.nonzero(HF.want_mask(f))
    pick = (int(xs[0]), int(ys[0]))
    (tmp_path / "params.bin").write_bytes(np.array([W, H, len(f.meshlet_instances), len(f.mesh_instances), len(f.selected), f.terrain_transform_index, *pick], np.uint32).tobytes())
    for name in ("vis", "depth", "color", "meshlet_instances", "mesh_instances", "selected"):
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(g["in_" + name]).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "highlight ok" in p.stdout, p.stderr + p.stdout
    out = functools.partial(shim_programs.read_out, tmp_path)
    picked = int(out("pick", np.uint32, 1)[0])
    assert picked == HF.want_pick(f, *pick) and picked in f.selected.tolist()
    same(out("mask_bits", np.uint64, (H, -1)), g["mask_bits"], "the shim's mask words")
    same(out("mask_attachment", np.uint8, (H, W)), g["mask_attachment"], "the shim's mask image")
    for fmt in HF.FORMATS:
        for mode in HF.MODES:
            name = f"dst_format{fmt}_mode{mode}"
            same(out(name, np.uint32, (H, W)), g[name], f"the shim's {name}")
