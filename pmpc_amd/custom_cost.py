"""Custom stage costs: J = sum over particles i and stages j of stage_cost(X[i, j], U[i, j]; p_i, j, N) written as a short piece of
device code, compiled at run time for the GPU with forward-mode automatic differentiation for the gradients (cx, cu) the SCP loops
linearise the cost with (pmpc_amd/csrc/cost_jit.hip, model_dual.h, cost_kernels.h).

    speed = pmpc_amd.CustomCost('''
    template <class T>
    __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) {   // x[XD], u[UD], p[CD] -> the stage's cost
      const double vmax = p[0], w = p[1];
      return w * log(1.0 + exp(4.0 * (x[3] - vmax))) / 4.0;                              // a soft speed limit
    }''', xdim=4, udim=2, pdim=2, uses_u=False)
    ctl = pmpc_amd.MPCController(builtin_model="bicycle", builtin_cost=dict(kind="custom", cost=speed, params=P), ...)

`x` / `u` are row j of X_prev / U_prev (0-based stage j: the state after j + 1 steps and the control that led to it); `T` is `double` or
a dual number with the operator and function set of `pmpc_amd.CustomModel`.  `p` points into global memory, so `pdim` may be 1 .. 64.
`uses_u=False` promises that the cost does not depend on `u`: `cu` is not formed and `U_ref` is not shifted.  The dict
`dict(kind="custom", cost=CustomCost, params=(M, pdim))` enters wherever a built-in cost does: `solve(..., device=..., builtin_cost=)`,
`DeviceSolver.scp_loop(cost=)`, `MPCController(builtin_cost=)`; the iteration tracks `X_ref - Q^-1 cx`, `U_ref - R^-1 cu`, so `Q` and `R`
must hold symmetric positive definite blocks stored as float64.  Compiling needs no GPU.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

from . import _lib

MAX_DIM, MAX_PDIM = 16, 64  # states and controls: the solver's limits; parameters are read from global memory


class CustomCost:
    def __init__(self, cost_source: str, xdim: int, udim: int, pdim: int, uses_u: bool = True, name: Optional[str] = None):
        self.cost_source, self.name = str(cost_source), name
        self.xdim, self.udim, self.pdim, self.uses_u = int(xdim), int(udim), int(pdim), bool(uses_u)
        for what, d, hi in (("xdim", self.xdim, MAX_DIM), ("udim", self.udim, MAX_DIM), ("pdim", self.pdim, MAX_PDIM)):
            if not 1 <= d <= hi:
                raise ValueError(f"CustomCost: {what} = {d} is outside 1 .. {hi}")
        self._code: Dict[str, bytes] = {}

    def __repr__(self):
        return f"CustomCost({self.name or 'unnamed'}, xdim={self.xdim}, udim={self.udim}, pdim={self.pdim}, uses_u={self.uses_u})"

    def compile(self, arch: str = "gfx950") -> bytes:
        """The code object for `arch` (a target id; what follows a ':' is dropped), compiled once per object and architecture.
        A compile error is a ValueError that carries the compiler's log; a missing runtime compiler a RuntimeError."""
        arch = str(arch).split(":")[0]
        if arch not in self._code:
            lib = _lib.load()
            if not hasattr(lib, "pmpc_cost_compile"):
                raise RuntimeError(f"{_lib.LIB_PATH} has no pmpc_cost_compile: it predates custom costs, rebuild it (make -C pmpc_amd/csrc)")
            code, n = ctypes.c_void_p(), ctypes.c_size_t(0)
            log = ctypes.create_string_buffer(1 << 16)
            rc = lib.pmpc_cost_compile(self.cost_source.encode(), self.xdim, self.udim, self.pdim, int(self.uses_u), arch.encode(), ctypes.byref(code),
                                       ctypes.byref(n), log, len(log))
            text = log.value.decode(errors="replace")
            if rc == 2:
                raise RuntimeError(f"CustomCost.compile: {text or 'the runtime compiler is not available'}")
            if rc != 0:
                raise ValueError(f"{self!r} does not compile for {arch}:\n{text}")
            try:
                self._code[arch] = ctypes.string_at(code, n.value)
            finally:
                lib.pmpc_model_free_code(code)
        return self._code[arch]

    def check_problem(self, M: int, xdim: int, udim: int, params) -> None:
        """Refuse a problem whose Q / R dimensions or `params` (M, pdim) are not this cost's (host-side: no device is touched)."""
        import numpy as np

        if (int(xdim), int(udim)) != (self.xdim, self.udim):
            raise ValueError(f"{self!r}: the problem has Q (.., {xdim}, {xdim}) and R (.., {udim}, {udim}), not the cost's dimensions")
        shape = tuple(params.shape) if hasattr(params, "shape") else np.shape(params)
        if shape != (int(M), self.pdim):
            raise ValueError(f"{self!r}: params must be (M, pdim) = ({M}, {self.pdim}), got {shape}")


def is_custom(cost) -> bool:
    return isinstance(cost, dict) and cost.get("kind") == "custom"


def check_cost_dict(cost, M: int, xdim: int, udim: int) -> None:
    """The host-side refusals of dict(kind="custom", cost=, params=): no CustomCost, dimensions that are not the problem's, params that
    are not (M, pdim).  Any other cost passes (the built-in ones have checks of their own)."""
    if not is_custom(cost):
        return
    cc = cost.get("cost")
    if not isinstance(cc, CustomCost):
        raise ValueError(f'dict(kind="custom") needs cost=, a pmpc_amd.CustomCost (got {type(cc).__name__})')
    if cost.get("params") is None:
        raise ValueError(f'dict(kind="custom") needs params=, the cost parameters (M, pdim) = ({M}, {cc.pdim})')
    cc.check_problem(M, xdim, udim, cost["params"])
