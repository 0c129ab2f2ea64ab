"""Custom state constraints: g_k(X[i, j]; p_i, j, N) <= 0 for every stage j of every particle i, written as a short piece of device code,
compiled at run time for the GPU with forward-mode automatic differentiation for the rows a_k'x <= h_k the SCP loops impose about the
previous iterate (pmpc_amd/csrc/cstr_jit.hip, model_dual.h, cstr_kernels.h).

    speed = pmpc_amd.CustomConstraint('''
    template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {   // x[XD], p[PD] -> g[KD]
      g[0] = x[3] - (p[0] - p[1] * j / N);          // v <= vmax, tightening along the horizon
      g[1] = p[2] - x[3];                           // v >= vmin
    }''', xdim=4, kdim=2, pdim=3)
    ctl = pmpc_amd.MPCController(builtin_model="bicycle", constraint=dict(cstr=speed, params=P), ...)

`x` is row j of X_prev (0-based stage j: the state after j + 1 steps); `T` is `double` or a dual number with the operator and function set
of `pmpc_amd.CustomModel`.  `p` points into global memory, so `pdim` may be 1 .. 64; `kdim` is 1 .. 4 and `xdim + kdim` at most 16 (the
sub-problem carries one auxiliary state per row).  About xbar = X_prev[i, j] an iteration imposes a_k'x <= h_k with a_k = grad g_k(xbar),
h_k = a_k'xbar - g_k(xbar).  The constraint reads states only.  The dict `dict(kind="custom", cstr=CustomConstraint, params=(M, pdim))`
enters wherever the keep-out constraint does: `solve(..., device=..., builtin_cstr=)`, `DeviceSolver.scp_loop(cstr=, aug=)`; the controller
takes it as `MPCController(constraint=dict(cstr=, params=))`.  Compiling needs no GPU.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

from . import _lib

MAX_DIM, MAX_KDIM, MAX_PDIM = 16, 4, 64  # states + rows: the solver's limit; parameters are read from global memory


class CustomConstraint:
    def __init__(self, cstr_source: str, xdim: int, kdim: int, pdim: int, name: Optional[str] = None):
        self.cstr_source, self.name = str(cstr_source), name
        self.xdim, self.kdim, self.pdim = int(xdim), int(kdim), int(pdim)
        for what, d, hi in (("xdim", self.xdim, MAX_DIM), ("kdim", self.kdim, MAX_KDIM), ("pdim", self.pdim, MAX_PDIM)):
            if not 1 <= d <= hi:
                raise ValueError(f"CustomConstraint: {what} = {d} is outside 1 .. {hi}")
        if self.xdim + self.kdim > MAX_DIM:
            raise ValueError(f"CustomConstraint: xdim + kdim = {self.xdim + self.kdim} exceeds the solver's {MAX_DIM} states")
        self._code: Dict[str, bytes] = {}

    def __repr__(self):
        return f"CustomConstraint({self.name or 'unnamed'}, xdim={self.xdim}, kdim={self.kdim}, pdim={self.pdim})"

    def compile(self, arch: str = "gfx950") -> bytes:
        """The code object for `arch` (a target id; what follows a ':' is dropped), compiled once per object and architecture.
        A compile error is a ValueError that carries the compiler's log; a missing runtime compiler a RuntimeError."""
        arch = str(arch).split(":")[0]
        if arch not in self._code:
            lib = _lib.load()
            if not hasattr(lib, "pmpc_cstr_compile"):
                raise RuntimeError(f"{_lib.LIB_PATH} has no pmpc_cstr_compile: it predates custom constraints, rebuild it (make -C pmpc_amd/csrc)")
            code, n = ctypes.c_void_p(), ctypes.c_size_t(0)
            log = ctypes.create_string_buffer(1 << 16)
            rc = lib.pmpc_cstr_compile(self.cstr_source.encode(), self.xdim, self.kdim, self.pdim, arch.encode(), ctypes.byref(code), ctypes.byref(n), log,
                                       len(log))
            text = log.value.decode(errors="replace")
            if rc == 2:
                raise RuntimeError(f"CustomConstraint.compile: {text or 'the runtime compiler is not available'}")
            if rc != 0:
                raise ValueError(f"{self!r} does not compile for {arch}:\n{text}")
            try:
                self._code[arch] = ctypes.string_at(code, n.value)
            finally:
                lib.pmpc_model_free_code(code)
        return self._code[arch]

    def check_problem(self, M: int, xdim: int, params) -> None:
        """Refuse a problem whose state dimension or `params` (M, pdim) are not this constraint's (host-side: no device is touched)."""
        import numpy as np

        if int(xdim) != self.xdim:
            raise ValueError(f"{self!r}: the problem has {xdim} states, not the constraint's dimensions")
        shape = tuple(params.shape) if hasattr(params, "shape") else np.shape(params)
        if shape != (int(M), self.pdim):
            raise ValueError(f"{self!r}: params must be (M, pdim) = ({M}, {self.pdim}), got {shape}")


def is_custom(cstr) -> bool:
    return isinstance(cstr, dict) and cstr.get("kind") == "custom"


def check_cstr_dict(cstr, M: int, xdim: int) -> None:
    """The host-side refusals of dict(kind="custom", cstr=, params=): no CustomConstraint, dimensions that are not the problem's, params
    that are not (M, pdim).  Any other constraint passes (the keep-out constraint has checks of its own)."""
    if not is_custom(cstr):
        return
    cc = cstr.get("cstr")
    if not isinstance(cc, CustomConstraint):
        raise ValueError(f'dict(kind="custom") needs cstr=, a pmpc_amd.CustomConstraint (got {type(cc).__name__})')
    if cstr.get("params") is None:
        raise ValueError(f'dict(kind="custom") needs params=, the constraint parameters (M, pdim) = ({M}, {cc.pdim})')
    cc.check_problem(M, xdim, cstr["params"])
