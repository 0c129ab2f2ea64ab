"""What the runtime-compiled device code of `CustomModel`, `CustomCost` and `CustomConstraint` shares on the host: the compile through
the library (pmpc_amd/csrc/jit_module.hip) with its per-architecture cache, and the checks of `dict(kind="custom", ...)`."""
from __future__ import annotations

import ctypes
from typing import Dict

from . import _lib


class CustomCode:
    """Base of the three front ends."""

    def _compile(self, entry: str, subject: str, source: str, ints, arch: str) -> bytes:
        """The code object of `source` for `arch` (a target id; what follows a ':' is dropped) by the library's entry point `entry`, which
        takes `ints` between the source and the arch; compiled once per object and architecture.  `subject`: what a library without
        `entry` predates."""
        arch = str(arch).split(":")[0]
        cache: Dict[str, bytes] = self.__dict__.setdefault("_code", {})  # the code objects compiled so far, by architecture
        if arch not in cache:
            lib = _lib.load()
            if not hasattr(lib, entry):
                raise RuntimeError(f"{_lib.LIB_PATH} has no {entry}: it predates {subject}, rebuild it (make -C pmpc_amd/csrc)")
            code, n = ctypes.c_void_p(), ctypes.c_size_t(0)
            log = ctypes.create_string_buffer(1 << 16)
            rc = getattr(lib, entry)(source.encode(), *ints, arch.encode(), ctypes.byref(code), ctypes.byref(n), log, len(log))
            text = log.value.decode(errors="replace")
            if rc == 2:
                raise RuntimeError(f"{type(self).__name__}.compile: {text or 'the runtime compiler is not available'}")
            if rc != 0:
                raise ValueError(f"{self!r} does not compile for {arch}:\n{text}")
            try:
                cache[arch] = ctypes.string_at(code, n.value)
            finally:
                lib.pmpc_model_free_code(code)
        return cache[arch]

    def _check_params(self, M: int, params) -> None:
        """`params` must have the shape (M, pdim)."""
        import numpy as np

        shape = tuple(params.shape) if hasattr(params, "shape") else np.shape(params)
        if shape != (int(M), self.pdim):
            raise ValueError(f"{self!r}: params must be (M, pdim) = ({M}, {self.pdim}), got {shape}")


def is_custom(d) -> bool:
    return isinstance(d, dict) and d.get("kind") == "custom"


def check_custom_dict(d, key: str, cls, subject: str, M: int, *dims) -> None:
    """The host-side refusals of dict(kind="custom", <key>=, params=): no `cls` object under `key`, dimensions that are not the problem's
    (`dims`, as `cls.check_problem` takes them), params that are not (M, pdim).  Any other dict passes."""
    if not is_custom(d):
        return
    obj = d.get(key)
    if not isinstance(obj, cls):
        raise ValueError(f'dict(kind="custom") needs {key}=, a pmpc_amd.{cls.__name__} (got {type(obj).__name__})')
    if d.get("params") is None:
        raise ValueError(f'dict(kind="custom") needs params=, the {subject} parameters (M, pdim) = ({M}, {obj.pdim})')
    obj.check_problem(M, *dims, d["params"])
