"""What the limits tests share: one broken rule of a context, the call refused with OXC_INVALID_ARG and that rule's message, nothing written.
A case is (name, changes, message).  A key of `changes` is a field of the context, "raw:<name>" a field of the filled C structure, "frame" the
prepared frame, "frame:<name>" one of the frame's record buffers.  What `unwritten` means stays with the pass: the caller brings the check."""
import ctypes as C
import dataclasses
import functools
import types

import torch

from oxylus_amd import lib as L

rep = dataclasses.replace
NO_FRAME = object()   # `frame` of an entry point that takes no frame argument; None is a frame argument that is null
# the three rules of a buffer where the passes word them alike; where a pass words one differently the module says so itself
NULL, ALIGNED, SHORT = " must not be null", " must be aligned to its texel", " is smaller than its extent"


def later(tensor, unit):
    """The tensor's bytes from the size of the dtype `unit` onwards: a start aligned to `unit` and to nothing larger."""
    return tensor.view(-1).view(unit)[1:]


def null_image(W, H):
    """A one-level image descriptor of W x H with no memory behind it."""
    im = L.Image()
    im.width, im.height, im.levels = W, H, 1
    return types.SimpleNamespace(width=W, height=H, c=lambda: im)


def buffer_cases(field, tensor, unit, smaller=SHORT, name=None, aligned=ALIGNED):
    """Null, then unaligned, then one element short: the three rules of one buffer, in the header's order.  `unit` is a dtype half the
    texel's size, by which the unaligned start is later; None leaves that case out, as `smaller` None leaves the short one out.  `name` is
    what the messages call the buffer where that is not the key."""
    name = name or field
    cases = [(f"{name} null", {field: None}, name + NULL)]
    if unit is not None:
        cases.append((f"{name} unaligned", {field: later(tensor, unit)}, name + aligned))
    if smaller is not None:
        cases.append((f"{name} small", {field: tensor.view(-1)[:-1]}, name + smaller))
    return cases


def frame_with_records(frame, **records):
    """`frame` with some record buffers replaced: one that is a field of the frame is its own, the others are its scene's."""
    own = {f.name for f in dataclasses.fields(frame)}
    scene = types.SimpleNamespace(**{**vars(frame.scene), **{k: v for k, v in records.items() if k not in own}})
    return rep(frame, scene=scene, **{k: v for k, v in records.items() if k in own})


class Raw:
    """A context whose C structure is changed by hand after `base` has filled it: what a dataclass derives and cannot be told.  A dotted
    name reaches into a nested structure; a callable value is given the field's filled value and returns the new one."""

    def __init__(self, base, **fields):
        self.base, self.fields = base, fields

    def c(self):
        c = self.base.c()
        for path, value in self.fields.items():
            *outer, leaf = path.split(".")
            target = functools.reduce(getattr, outer, c)
            setattr(target, leaf, value(getattr(target, leaf)) if callable(value) else value)
        return c


def attempt(r, symbol, base, changes, frame=NO_FRAME):
    """One call of the C entry point `symbol` with `changes` applied to the context `base` and, where the entry point takes one, to the
    prepared frame `frame`.  Returns (status, oxc_last_error)."""
    c = Raw(rep(base, **{k: v for k, v in changes.items() if ":" not in k and k != "frame"}), **{k[4:]: v for k, v in changes.items() if k.startswith("raw:")}).c()
    args = [C.byref(c)]
    if frame is not NO_FRAME:
        frame = changes.get("frame", frame)
        records = {k[6:]: v for k, v in changes.items() if k.startswith("frame:")}
        if frame is not None and records:
            frame = frame_with_records(frame, **records)
        fc = frame.c() if frame is not None else None
        args.insert(0, C.byref(fc) if fc is not None else None)
    status = getattr(r._lib, symbol)(r._ctx, *args, r._stream(None))
    return status, r._lib.oxc_last_error(r._ctx).decode()


def refused(r, symbol, base, changes, message, label, frame=NO_FRAME):
    """OXC_INVALID_ARG with `message` right behind the entry point's name: the message of that rule and of no other."""
    status, error = attempt(r, symbol, base, changes, frame)
    assert status == L.OXC_INVALID_ARG and f"{symbol[4:]}: {message}" in error, f"{label}: status {status}, {error!r}, expected {message!r}"


def raises_refusal(call, message, prefix=None, synchronize=torch.cuda.synchronize):
    """`call()`, which goes through a RendererInstance method, raises OxcError with OXC_INVALID_ARG and `message` -- as it stands, no
    pattern -- in its text, with `prefix`: in it where one is given.  Returns the text; the caller then checks that nothing was written."""
    try:
        call()
    except L.OxcError as e:
        text = str(e)
        assert e.status == L.OXC_INVALID_ARG, f"status {e.status}, {text!r}, expected {message!r}"
        assert message in text and (prefix is None or f"{prefix}: " in text), f"{text!r}, expected {message!r}" + (f" from {prefix}" if prefix else "")
    else:
        raise AssertionError(f"accepted, expected {message!r}")
    synchronize()
    return text


def alone_and_in_pairs(r, symbol, cases, base, frame, unwritten, synchronize=torch.cuda.synchronize):
    """Every case alone, then with every later case that changes different things: the message is that of the case earlier in the
    documented order.  `unwritten(label)` asserts that the outputs hold their pre-fill and every band its poison; what a call wrote would
    stay, so it is asked after every single case and again after that case's pairs."""
    for i, (name, first, message) in enumerate(cases):
        refused(r, symbol, base, first, message, name, frame)
        synchronize()
        unwritten(name)
        for other, second, _ in cases[i + 1:]:
            if not set(first) & set(second):
                refused(r, symbol, base, {**first, **second}, message, f"{name} + {other}", frame)
        synchronize()
        unwritten(f"{name} and a later one")
