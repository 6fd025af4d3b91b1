"""Fills the ctypes mirror of a C structure (lib.py) from the dataclass that carries its values (renderer.py).

A dataclass that derives from `Marshalled` names its structure in `_ctype`, and every field of that structure is accounted for by exactly
one of three things:
  - a dataclass field of the same name, converted by the C field's type (`_assignment`);
  - `_derived`: C field -> "attribute.path" read in place of the same-named attribute and converted like it, or function(self) that
    returns the C value itself (either wins over a same-named dataclass field);
  - `_leave`: padding, reserved words and what the library writes back, which are not touched.
`struct_size` is always sizeof(_ctype).  The accounting is checked once, when the class is created: a C field nothing accounts for, or a
`_derived` / `_leave` name the structure does not have, is a TypeError there and not a silently zero field in a call.

`.c()` runs per pass call, so the plan is compiled once per class into one function of plain assignments (`_fill_source` keeps its text),
as dataclasses does for __init__.
"""
from __future__ import annotations

import ctypes as C
import inspect

from . import lib as L


def _buf(t) -> L.Buffer:
    """A tensor's memory as an oxc_buffer; None is {NULL, 0}."""
    if t is None:
        return L.Buffer(None, 0)
    return L.Buffer(t.data_ptr(), t.numel() * t.element_size())


# a bool becomes 1; of an integer ctypes keeps the field's low 32 bits (no overflow check), so a negative u32 arrives masked to 0xFFFFFFFF
_SCALAR = {C.c_float: "float({})", C.c_uint32: "int({})", C.c_int32: "int({})"}


def _assignment(name: str, ftype, source: str, env: dict) -> list:
    """The lines that fill C field `name` of type `ftype` from self.<source>; what they call goes into `env`."""
    if ftype in _SCALAR:
        return [f"c.{name} = {_SCALAR[ftype].format('self.' + source)}"]
    if ftype is L.Buffer:
        return [f"c.{name} = _buf(self.{source})"]
    if issubclass(ftype, C.Structure):  # an image or a nested record: its own .c(), or the structure itself (L.CullCamera); None: untouched
        env["T_" + name] = ftype
        return [f"v = self.{source}", "if v is not None:", f"    c.{name} = v if v.__class__ is T_{name} else v.c()"]
    if issubclass(ftype, C.Array) and ftype._type_ in _SCALAR:  # the sequence's first _length_ elements, each through float() / int()
        one, n = "float" if ftype._type_ is C.c_float else "int", ftype._length_
        return [f"v = self.{source}", f"c.{name}[:] = list(map({one}, v if len(v) == {n} else v[:{n}]))"]
    raise TypeError(f"no conversion rule for a C field of type {ftype.__name__}")


class Marshalled:
    _ctype = None   # the L.<Structure> that .c() fills
    _derived = {}
    _leave = ()

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        fields = dict(cls._ctype._fields_)
        own = inspect.get_annotations(cls)
        for kind, names in (("_derived", cls._derived), ("_leave", cls._leave)):
            for name in names:
                if name not in fields:
                    raise TypeError(f"{cls.__name__}.{kind} names {name}, which is no field of {cls._ctype.__name__}")
        env, body = {"_buf": _buf}, []
        for name, ftype in fields.items():
            if name in cls._leave:
                if name in cls._derived or name in own:
                    raise TypeError(f"{cls.__name__}: {name} is in _leave and is also {'derived' if name in cls._derived else 'an attribute'}")
            elif callable(cls._derived.get(name)):
                env["D_" + name] = cls._derived[name]
                body.append(f"c.{name} = D_{name}(self, *args)")
            elif name == "struct_size":
                body.append(f"c.struct_size = {C.sizeof(cls._ctype)}")
            elif name in cls._derived or name in own:
                try:
                    body += _assignment(name, ftype, cls._derived.get(name, name), env)
                except TypeError as e:
                    raise TypeError(f"{cls.__name__}.{name}: {e}") from None
            else:
                raise TypeError(f"{cls.__name__}: nothing fills {cls._ctype.__name__}.{name} (no attribute, not in _derived, not in _leave)")
        cls._filled = tuple(n for n in fields if n not in cls._leave)
        env["T"] = cls._ctype
        head = "def _fill(self, c=None, *args):\n    if c is None:\n        c = T()\n"
        cls._fill_source = head + "".join(f"    {line}\n" for line in body) + "    return c\n"
        exec(cls._fill_source, env)
        cls._fill = env["_fill"]  # `args` go to the `_derived` functions after self (EyeAdaptationContext's delta_time)
        if "c" not in vars(cls):
            cls.c = cls._fill     # .c(): a fresh structure, filled
