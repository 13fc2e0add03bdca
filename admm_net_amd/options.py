"""Per-model option sets: the A/B switches of INTEGRATION.md section 6 chosen for one model instead of one process.

``Options(spectral=0, eig="ql", spectral_tol=3e-7)`` names overrides of the process defaults (the ``ADMMNET_*`` environment,
read once) in the environment's own vocabulary: the keyword is the variable's name without ``ADMMNET_``, lower case, the
value its string.  ``model.options = Options(...)`` makes every call that takes its ``cfg`` from the model run under them.
"""
from __future__ import annotations

import ctypes
import os
import re

from . import _lib

_PREFIX = "ADMMNET_"


def _rebuild(overrides):
    return Options(**overrides)


class Options:
    """An immutable set of overrides.  A value of None means "inherit" (the keyword is dropped); a bool is written as
    1 / 0, everything else goes through ``str()``.  The object holds the overrides, not the handle: ``handle`` interns them
    in the library of the running process (admmnet_options_intern) on first use and caches the answer per process id, so a
    pickled or deep-copied ``Options`` -- a rank started by ``torch.distributed``, a DataLoader worker -- interns again
    where it lands.  ``==`` and ``hash`` compare the RESOLVED settings: ``Options(spectral=0) == Options(spectral="00")``,
    and an ``Options`` that changes nothing equals ``Options()``.  An unknown keyword raises ``AdmmNetError`` when the
    handle is first needed."""
    __slots__ = ("_overrides", "_cache")

    def __init__(self, **overrides):
        items = []
        for key in sorted(overrides):
            value = overrides[key]
            if not re.fullmatch(r"[a-z][a-z0-9_]*", key):
                raise ValueError(f"option names are the ADMMNET_* names without the prefix, lower case; got {key!r}")
            if value is None:
                continue
            items.append((key, str(int(value)) if isinstance(value, bool) else str(value)))
        object.__setattr__(self, "_overrides", tuple(items))
        object.__setattr__(self, "_cache", None)

    def __setattr__(self, name, value):
        raise AttributeError("Options is immutable")

    __delattr__ = __setattr__

    @property
    def overrides(self) -> dict:
        """{keyword: string} as given (None entries dropped)."""
        return dict(self._overrides)

    @property
    def handle(self) -> int:
        """The option handle of this process (0 = nothing differs from the process defaults)."""
        pid = os.getpid()
        if self._cache is None or self._cache[0] != pid:
            lib = _lib.load()
            n = len(self._overrides)
            names = (ctypes.c_char_p * n)(*[(_PREFIX + k.upper()).encode() for k, _ in self._overrides])
            values = (ctypes.c_char_p * n)(*[v.encode() for _, v in self._overrides])
            h = lib.admmnet_options_intern(names, values, n)
            if h < 0:
                _lib.check(h, "admmnet_options_intern")
            object.__setattr__(self, "_cache", (pid, h))
        return self._cache[1]

    def resolved(self) -> dict:
        """Every switch as the library resolved it (admmnet_options_describe): {keyword: int, or float for spectral_tol}.
        A word switch reads 1 where its word is set (``eig``: 1 = "ql"), ``pad_min`` -1000 where it is unset."""
        return describe(self.handle)

    def __eq__(self, other):
        if not isinstance(other, Options):
            return NotImplemented
        return self._overrides == other._overrides or self.resolved() == other.resolved()

    def __hash__(self):
        return hash(tuple(sorted(self.resolved().items())))

    def __reduce__(self):
        return _rebuild, (self.overrides,)

    def __repr__(self):
        return "Options(%s)" % ", ".join(f"{k}={v!r}" for k, v in self._overrides)


def describe(handle: int) -> dict:
    """The resolved settings of an option handle (0 = the process defaults) as a dict."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    n = lib.admmnet_options_describe(handle, buf, len(buf))
    if n < 0:
        _lib.check(n, "admmnet_options_describe")
    out = {}
    for line in buf.value.decode().splitlines():
        name, value = line.split()
        out[name[len(_PREFIX):].lower()] = float(value) if name == _PREFIX + "SPECTRAL_TOL" else int(value)
    return out
