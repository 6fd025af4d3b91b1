"""The C++ shim reaches oxc_apply_debug_view: tests/cpp/shim_debug_view.cpp runs RendererInstance::apply_debug_view under the fourteen main
views on the golden 17 x 9 frame; the image each view writes equals the fixture's bytes."""
import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- DebugContext and the member function -- and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_debug_view", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


@pytest.mark.gpu
def test_the_member_function_draws_the_fourteen_views(tmp_path):
    import debug_view_frames as DF
    import debug_view_model as DV
    from gpu_passes import same

    exe = shim_programs.build("shim_debug_view", tmp_path)
    g = np.load(DF.GOLDEN)
    f = DF.golden_frame()
    W, H = f.extent
    params = np.array([W, H, len(f.meshlet_instances), len(f.mesh_instances), len(f.meshes)], np.uint32).tobytes() + np.float32(f.heatmap_scale).tobytes()
    (tmp_path / "params.bin").write_bytes(params)
    for name in DF.IMAGES + DF.RECORDS:
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(g["in_" + name]).tobytes())
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "debug views ok" in p.stdout, p.stderr + p.stdout
    for view in DV.MAIN_VIEWS:
        same(shim_programs.read_out(tmp_path, f"view{view}", np.uint16, (H, W, 4)), g["out_" + DV.NAMES[view]], f"the shim's {DV.NAMES[view]}")
