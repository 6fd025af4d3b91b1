"""tests/refusals.py against a stub renderer, without a GPU: the harness passes on an entry point that keeps its rules and fails on every way
one can break them, so that a limits test that goes through it cannot pass by asserting nothing."""
import ctypes as C
import dataclasses
import types

import pytest
import torch

import refusals as R
from oxylus_amd import lib as L


class Ctx(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("count", C.c_uint32), ("data", C.c_void_p)]


class Records(C.Structure):
    _fields_ = [("own", C.c_void_p), ("shared", C.c_void_p)]


@dataclasses.dataclass
class Context:
    width: int = 4
    data: object = 64

    def c(self):
        return Ctx(C.sizeof(Ctx), self.width, 2, self.data)


@dataclasses.dataclass
class Frame:
    scene: object
    own: object = 128

    def c(self):
        return Records(self.own, self.scene.shared)


# (broken(context), message), or (broken(frame), message, "frame") for what only the entry point with a frame asks, in the stub's documented order
RULES = [(lambda c: c.struct_size != C.sizeof(Ctx), "bad context / struct_size"), (lambda c: c.width == 0, "the extent must not be zero"),
         (lambda c: c.count > 8, "count must be in 0 .. 8"), (lambda f: f is None, "the frame must not be null", "frame"), (lambda c: not c.data, "data must not be null"),
         (lambda f: f is not None and not f.own, "own must not be null", "frame"), (lambda f: f is not None and not f.shared, "shared must not be null", "frame")]
CHANGES = [{"raw:struct_size": 8}, dict(width=0), {"raw:count": 9}, {"frame": None}, dict(data=None), {"frame:own": None}, {"frame:shared": None}]
CASES = [(str(change), change, rule[1]) for change, rule in zip(CHANGES, RULES)]
FRAME = Frame(types.SimpleNamespace(shared=256))
no_sync = lambda: None  # noqa: E731


class Stub:
    """A renderer as far as the harness looks at one: _ctx, _stream, _lib with two entry points, and oxc_last_error."""

    def __init__(self, rules=RULES, status=L.OXC_INVALID_ARG):
        self._ctx, self._lib, self._stream, self.rules, self.status, self.error = object(), self, lambda stream: None, rules, status, b""

    def oxc_last_error(self, ctx):
        return self.error

    def check(self, name, rules, c, *frame):
        for broken, message, *on_frame in rules:
            if broken(*frame) if on_frame else broken(c._obj):
                self.error = f"{name}: {message}".encode()
                return self.status
        self.error = b""
        return L.OXC_OK

    def oxc_probe(self, ctx, c, stream):
        return self.check("probe", [rule for rule in self.rules if len(rule) == 2], c)

    def oxc_probe_frame(self, ctx, frame, c, stream):
        return self.check("probe_frame", self.rules, c, frame._obj if frame is not None else None)


def run(stub, unwritten=lambda label: None):
    R.alone_and_in_pairs(stub, "oxc_probe_frame", CASES, Context(), FRAME, unwritten, synchronize=no_sync)


@pytest.mark.parametrize("symbol,frame,cases", [("oxc_probe_frame", FRAME, CASES), ("oxc_probe", R.NO_FRAME, [c for c, rule in zip(CASES, RULES) if len(rule) == 2])],
                         ids=["frame", "no frame"])
def test_the_honest_stub_passes_and_unwritten_is_asked_twice_a_case(symbol, frame, cases):
    labels, syncs = [], []
    R.alone_and_in_pairs(Stub(), symbol, cases, Context(), frame, labels.append, synchronize=lambda: syncs.append(len(labels)))
    assert labels == [label for name, _, _ in cases for label in (name, f"{name} and a later one")]
    assert syncs == list(range(2 * len(cases)))   # a synchronise in front of every check
    assert FRAME.scene.shared == 256 and FRAME.own == 128   # the frame handed in is not changed


@pytest.mark.parametrize("k", range(len(RULES)))
def test_an_accepted_broken_case_and_another_message_fail(k):
    with pytest.raises(AssertionError, match="status 0"):
        run(Stub(RULES[:k] + RULES[k + 1:]))
    with pytest.raises(AssertionError, match=f"status {L.OXC_INVALID_ARG}"):
        run(Stub(RULES[:k] + [(RULES[k][0], "not " + RULES[k][1]) + RULES[k][2:]] + RULES[k + 1:]))


def test_the_later_rule_named_in_a_pair_fails():
    """Two neighbouring rules swapped: every case alone is still refused with its message, the pair of the two is not."""
    asked = []
    with pytest.raises(AssertionError, match="'width': 0} \\+ {'raw:count': 9}"):
        run(Stub(RULES[:1] + [RULES[2], RULES[1]] + RULES[3:]), asked.append)
    assert asked == [CASES[0][0], CASES[0][0] + " and a later one", CASES[1][0]]


def test_another_status_with_the_right_text_fails():
    with pytest.raises(AssertionError, match=f"status {L.OXC_HIP_ERROR}"):
        run(Stub(status=L.OXC_HIP_ERROR))


@pytest.mark.parametrize("label", [CASES[2][0], CASES[2][0] + " and a later one"], ids=["after a single case", "after a case's pairs"])
def test_a_written_output_fails(label):
    def unwritten(asked):
        assert asked != label, "written after a refusal"

    with pytest.raises(AssertionError, match="written after a refusal"):
        run(Stub(), unwritten)


def test_raises_refusal():
    def raising(status, text):
        def call():
            raise L.OxcError(status, text)
        return call

    text = R.raises_refusal(raising(L.OXC_INVALID_ARG, "probe: mode must be in 0 .. 4"), "mode must be in 0 .. 4", prefix="probe", synchronize=no_sync)
    assert text.endswith("probe: mode must be in 0 .. 4")
    for status, said, prefix in ((L.OXC_INVALID_ARG, "probe: mode must be in 0 xx 4", None),   # a pattern would match: the dots
                                 (L.OXC_HIP_ERROR, "probe: mode must be in 0 .. 4", None), (L.OXC_INVALID_ARG, "other: mode must be in 0 .. 4", "probe")):
        with pytest.raises(AssertionError, match="expected"):
            R.raises_refusal(raising(status, said), "0 .. 4", prefix, synchronize=no_sync)
    with pytest.raises(AssertionError, match="accepted"):
        R.raises_refusal(lambda: None, "0 .. 4", synchronize=no_sync)


@pytest.mark.parametrize("unit", [torch.int8, torch.int16, torch.int32])
def test_buffer_cases_null_unaligned_short(unit):
    t = torch.zeros((3, 8), dtype=torch.int32)
    (n0, null, m0), (n1, unaligned, m1), (n2, short, m2) = R.buffer_cases("frame:records", t, unit, " is smaller than count records", "records_buffer")
    assert (n0, n1, n2) == ("records_buffer null", "records_buffer unaligned", "records_buffer small")
    assert (m0, m1, m2) == ("records_buffer must not be null", "records_buffer must be aligned to its texel", "records_buffer is smaller than count records")
    assert null == {"frame:records": None}
    assert unaligned["frame:records"].data_ptr() - t.data_ptr() == torch.empty(0, dtype=unit).element_size()
    assert short["frame:records"].data_ptr() == t.data_ptr() and short["frame:records"].numel() == t.numel() - 1
    # what it is told to leave out, and the defaults
    assert [c[0] for c in R.buffer_cases("b", t, None)] == ["b null", "b small"] and [c[0] for c in R.buffer_cases("b", t, unit, None)] == ["b null", "b unaligned"]
    assert [c[2] for c in R.buffer_cases("b", t, unit, aligned=" must be aligned to 8 bytes")[1:]] == ["b must be aligned to 8 bytes", "b is smaller than its extent"]


def test_raw_sets_plain_nested_and_computed_fields():
    class Outer(C.Structure):
        _fields_ = [("inner", Ctx), ("pair", C.c_uint32 * 2)]

    base = types.SimpleNamespace(c=lambda: Outer(Ctx(1, 2, 3, 4), (5, 6)))
    c = R.Raw(base, pair=(7, 8), **{"inner.width": 9, "inner.count": lambda count: count + 10}).c()
    assert (c.inner.struct_size, c.inner.width, c.inner.count, list(c.pair)) == (1, 9, 13, [7, 8])
