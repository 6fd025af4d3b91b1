"""The C++ shim reaches oxc_decode_visbuffer_textured: tests/cpp/shim_textured_decode.cpp runs RendererInstance::decode_visbuffer(context,
images, samplers) on the golden 17 x 9 frame -- five sampler presets, three formats, flip-y, a two-component map, 64-way divergent tiles --
with the table counts taken from the buffers' sizes and Camera::position from the cull camera; the four images equal the Python path's
bytes, which are the checker's."""
import numpy as np
import pytest

import shim_programs


def test_the_program_builds(tmp_path):
    """(no GPU) the program compiles against the shim header -- the member with its two tables -- and links to liboxcull.so."""
    p = shim_programs.run(shim_programs.build("shim_textured_decode", tmp_path))
    assert p.returncode == 2 and "usage" in p.stdout


def relocatable(records, word, base, null_ok=True):
    """Column `word` of int64 records as 1 + the byte offset from `base`; a null pointer stays 0."""
    out = records.copy()
    ptr = out[:, word]
    assert null_ok or (ptr != 0).all()
    out[:, word] = np.where(ptr != 0, ptr - base + 1, 0)
    return out


@pytest.mark.gpu
def test_the_member_decodes_with_the_tables(tmp_path, renderer):
    import torch

    import textured_decode_frames as FR
    from gpu_passes import decode_got_of, same

    exe = shim_programs.build("shim_textured_decode", tmp_path)
    f = FR.golden_frame()
    s = f.cpu
    lods = s.lods.numpy().reshape(-1, 8)
    for word, stream in ((1, s.meshlets), (3, s.micro), (4, s.vidx)):
        lods = relocatable(lods, word, stream.data_ptr(), null_ok=False)
    lods[:, 0] = lods[:, 2] = 0  # the index list and the bounds: the decode reads neither
    meshes = s.meshes.numpy().reshape(-1, 8)
    for word, stream in ((0, s.positions), (1, s.normals), (2, s.texcoords), (4, s.lods)):
        meshes = relocatable(meshes, word, stream.data_ptr())
    # the image records over one blob of texels, each level 4-byte aligned
    blob, records = bytearray(), np.zeros((len(f.images), 18), np.uint64)
    for i, im in enumerate(f.images):
        records[i, 0] = len(blob) + 1
        start = len(blob)
        for k, level in enumerate(im["levels"]):
            records[i, 3 + k] = len(blob) - start
            blob += np.ascontiguousarray(level).tobytes()
            blob += bytes(-len(blob) % 4)
        records[i].view(np.uint32)[2:6] = (im["width"], im["height"], len(im["levels"]), im["format"])
    samplers = np.array([list(r) + [0] for r in f.samplers], np.uint32)
    n_materials = s.materials.numel() // 56
    params = (np.array([f.W, f.H, s.n_meshlet_instances, s.n_mesh_instances, s.n_meshes, n_materials, len(f.images), len(samplers)], np.uint32).tobytes()
              + np.asarray(s.camera["projection_view"], np.float32).tobytes() + np.array(list(f.camera_position) + [0.0], np.float32).tobytes())
    assert len(params) == 32 + 64 + 16
    (tmp_path / "params.bin").write_bytes(params)
    files = dict(positions=s.positions, normals=s.normals, texcoords=s.texcoords, meshlets=s.meshlets, micro=s.micro, vidx=s.vidx, lods=lods, meshes=meshes,
                 meshlet_instances=s.meshlet_instances, mesh_instances=s.mesh_instances, transforms=s.transforms, materials=s.materials, images=records,
                 samplers=samplers, vis=f.vis, depth=f.depth)
    for name, a in files.items():
        (tmp_path / f"{name}.bin").write_bytes(np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    (tmp_path / "texels.bin").write_bytes(bytes(blob))
    p = shim_programs.run(exe, tmp_path)
    assert p.returncode == 0 and "textured decode ok" in p.stdout, p.stderr + p.stdout

    ctx, images, _gpu, _keep = FR.contexts(renderer, f)
    renderer.decode_visbuffer_textured(ctx, images)
    python = decode_got_of(ctx)
    same(python, FR.want(f, None, FR.init_images(f)), "the Python path against the checker")
    assert (python["normal"][..., :2] != python["normal"][..., 2:]).any()  # a normal map was sampled
    for name, want in python.items():
        same(shim_programs.read_out(tmp_path, name, want.dtype, want.shape), want, f"the shim's {name}")
