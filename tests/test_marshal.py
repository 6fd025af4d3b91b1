"""oxylus_amd/_marshal.py: a context's `.c()` fills its ctypes structure from the structure's `_fields_`, and every C field is accounted for
by exactly one of a same-named attribute, `_derived` and `_leave` -- checked when the class is created (no GPU needed)."""
import ctypes as C
import re
from dataclasses import dataclass

import pytest
import torch

from oxylus_amd import lib as L
from oxylus_amd import renderer as R
from oxylus_amd._marshal import Marshalled


class Toy(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("count", C.c_uint32), ("scale", C.c_float), ("_pad", C.c_uint32), ("data", L.Buffer)]


def test_an_unaccounted_c_field_is_a_type_error():
    with pytest.raises(TypeError, match=r"Forgetful.*Toy\.scale"):
        @dataclass
        class Forgetful(Marshalled):
            _ctype = Toy
            _leave = ("_pad",)
            count: int
            data: object


def test_a_derived_name_that_is_no_c_field_is_a_type_error():
    with pytest.raises(TypeError, match=r"Misspelt\._derived names scael"):
        @dataclass
        class Misspelt(Marshalled):
            _ctype = Toy
            _derived = {"scael": lambda s: 1.0}
            _leave = ("_pad",)
            count: int
            scale: float
            data: object


def test_a_leave_alone_name_that_is_no_c_field_is_a_type_error():
    with pytest.raises(TypeError, match=r"Stale\._leave names _pad2"):
        @dataclass
        class Stale(Marshalled):
            _ctype = Toy
            _leave = ("_pad", "_pad2")
            count: int
            scale: float
            data: object


def test_a_complete_toy_class_marshals():
    @dataclass
    class Whole(Marshalled):
        _ctype = Toy
        _derived = {"scale": lambda s: s.factor * 2}
        _leave = ("_pad",)
        count: int
        data: object
        factor: float = 1.5  # not a C field: only C fields need accounting

    c = Whole(True, None).c()
    assert (c.struct_size, c.count, c.scale, c._pad, c.data.dptr, c.data.bytes) == (C.sizeof(Toy), 1, 3.0, 0, None, 0)


def _contexts():
    return [c for c in vars(R).values() if isinstance(c, type) and issubclass(c, Marshalled) and c is not Marshalled]


def test_every_context_class_accounts_for_every_c_field():
    """Importing renderer.py has run the check; this spells its result out: the three sources partition the structure's fields."""
    classes = _contexts()
    assert {c.__name__ for c in classes} >= {
        "PreparedFrame", "CullGeometryContext", "MainGeometryContext", "VirtualShadowmapContext", "VsmDrawContext", "ShadowResolveContext",
        "ContactShadowsContext", "AmbientOcclusionContext", "VisbufferDecodeContext", "PBRContext", "EyeAdaptationContext", "BloomContext",
        "TonemapContext", "FxaaContext", "Atmosphere", "SkyLutContext", "AtmosphereContext"}
    for cls in classes:
        assigned = set(re.findall(r"\bc\.(\w+)(?:\[:\])? = ", cls._fill_source))
        assert assigned == set(cls._filled) and not assigned & set(cls._leave), cls.__name__
        assert sorted(cls._filled + tuple(cls._leave)) == sorted(n for n, _ in cls._ctype._fields_), cls.__name__
        assert all(n.startswith("_") or n.endswith("_buffer") for n in cls._leave), cls.__name__  # padding / reserved, or written back


H = W = 4


@pytest.fixture(scope="module")
def final():
    return torch.zeros((H, W), dtype=torch.int32)


def test_struct_size_and_a_buffer_field(final):
    ctx = R.FxaaContext.create(final)
    c = ctx.c()
    assert isinstance(c, L.FxaaContext) and c.struct_size == C.sizeof(L.FxaaContext)
    assert (c.width, c.height, c.source_format) == (W, H, L.EYE_SOURCE_B10G11R11)
    assert c.final_attachment.dptr == final.data_ptr() and c.final_attachment.bytes == final.numel() * final.element_size() == 64
    assert c.fxaa_attachment.dptr == ctx.fxaa_attachment.data_ptr() != final.data_ptr()


def test_a_none_tensor_is_a_null_buffer_and_a_none_image_stays_zero(final):
    tone = R.TonemapContext.create(final)  # no exposure buffer, no bloom
    c = tone.c()
    assert (c.exposure_buffer.dptr, c.exposure_buffer.bytes) == (None, 0)
    assert bytes(c.bloom_upsampled_attachment) == bytes(C.sizeof(L.ImagePyramid))
    assert c.dst_attachment.dptr == tone.dst_attachment.data_ptr()


def test_an_image_field_is_the_attributes_own_c(final):
    bloom = R.BloomContext.create(final)
    tone = R.TonemapContext.create(final, bloom=bloom)
    assert bytes(tone.c().bloom_upsampled_attachment) == bytes(bloom.bloom_upsampled_attachment.c())
    assert tone.c().bloom_upsampled_attachment.dptr == bloom.bloom_upsampled_attachment.data.data_ptr()
    assert bytes(bloom.c().bloom_downsampled_attachment) == bytes(bloom.bloom_downsampled_attachment.c())


def test_bools_ints_floats_and_arrays():
    depth = torch.zeros((H, W), dtype=torch.float32)
    normal = torch.zeros((H, W, 4), dtype=torch.int16)
    hilbert = torch.zeros((64, 64), dtype=torch.int16)
    view = [float(i) for i in range(16)]
    ao = R.AmbientOcclusionContext.create(depth, normal, hilbert, view, view[::-1], far_clip=100, noise_index=-1, slice_count=True)
    c = ao.c()
    assert c.noise_index == 0xFFFFFFFF   # masked to 32 bits
    assert c.slice_count == 1            # a bool becomes 1
    assert c.far_clip == 100.0 and list(c.view) == view and list(c.projection) == view[::-1] and list(c.resolution) == [float(W), float(H)]
    assert (c.depth_attachment.dptr, c.depth_attachment.width, c.depth_attachment.height) == (depth.data_ptr(), W, H)
    cull = R.CullGeometryContext(use_hiz=True, small_triangle_cull=True)
    assert (cull.c().use_hiz, cull.c().small_triangle_cull, cull.c().use_hpb) == (1, 1, 0)


def test_nested_records_and_u32_arrays():
    atm = R.Atmosphere.engine(sky_view_lut_size=(8, 4, 1))
    ctx = R.AtmosphereContext.create(atm, device="cpu", sun_dir=(0.0, 0.6, 0.8))
    c = ctx.c()
    assert bytes(c.atmosphere) == bytes(atm.c()) and list(c.atmosphere.sky_view_lut_size) == [8, 4, 1]
    assert c.atmosphere.planet_radius == 6360.0 and [round(x, 6) for x in c.sun_dir] == [0.0, 0.6, 0.8]
    assert c.sky_view_lut.dptr == ctx.sky_view_lut_attachment.data_ptr() and c.sky_view_lut.bytes == 4 * 8 * 4 * 2  # derived: *_attachment
    assert (c._pad, c._pad1) == (0, 0)


def test_derived_fields_and_the_persistent_cull_structure(final):
    depth = torch.zeros((H, 2 * W), dtype=torch.float32)
    eye = R.EyeAdaptationContext.create(final, R.exposure_buffer("cpu"), adaptation_speed=2.0)
    assert eye.c(0.5).time_coeff == pytest.approx(R.eye_adaptation_time_coeff(2.0, 0.5)) and eye.c().time_coeff == 0.0
    eye.time_coeff = 0.25
    assert eye.c(0.5).time_coeff == 0.25
    vis = torch.zeros((H, 2 * W), dtype=torch.int32)
    dec = R.VisbufferDecodeContext.create(vis, depth, [0.0] * 16, 3)
    assert (dec.c().width, dec.c().height, dec.c().clear) == (2 * W, H, 1)       # width / height from depth_attachment
    cull = R.CullGeometryContext()
    assert cull.c() is cull._c                                                   # filled in place
    cull._c.draw_geometry_cmd_buffer = L.Buffer(0x1000, 20)                      # what the library writes back
    assert (cull.c().draw_geometry_cmd_buffer.dptr, cull.c().draw_geometry_cmd_buffer.bytes) == (0x1000, 20)
