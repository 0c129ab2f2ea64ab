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

from typing import Optional

from .custom_jit import CustomCode, check_custom_dict, is_custom  # noqa: F401 (is_custom: imported from here by others)

MAX_DIM, MAX_PDIM = 16, 64  # states and controls: the solver's limits; parameters are read from global memory


class CustomCost(CustomCode):
    def __init__(self, cost_source: str, xdim: int, udim: int, pdim: int, uses_u: bool = True, name: Optional[str] = None):
        self.cost_source, self.name = str(cost_source), name
        self.xdim, self.udim, self.pdim, self.uses_u = int(xdim), int(udim), int(pdim), bool(uses_u)
        for what, d, hi in (("xdim", self.xdim, MAX_DIM), ("udim", self.udim, MAX_DIM), ("pdim", self.pdim, MAX_PDIM)):
            if not 1 <= d <= hi:
                raise ValueError(f"CustomCost: {what} = {d} is outside 1 .. {hi}")

    def __repr__(self):
        return f"CustomCost({self.name or 'unnamed'}, xdim={self.xdim}, udim={self.udim}, pdim={self.pdim}, uses_u={self.uses_u})"

    def compile(self, arch: str = "gfx950") -> bytes:
        """The code object for `arch` (a target id; what follows a ':' is dropped), compiled once per object and architecture.
        A compile error is a ValueError that carries the compiler's log; a missing runtime compiler a RuntimeError."""
        return self._compile("pmpc_cost_compile", "custom costs", self.cost_source, (self.xdim, self.udim, self.pdim, int(self.uses_u)), arch)

    def check_problem(self, M: int, xdim: int, udim: int, params) -> None:
        """Refuse a problem whose Q / R dimensions or `params` (M, pdim) are not this cost's (host-side: no device is touched)."""
        if (int(xdim), int(udim)) != (self.xdim, self.udim):
            raise ValueError(f"{self!r}: the problem has Q (.., {xdim}, {xdim}) and R (.., {udim}, {udim}), not the cost's dimensions")
        self._check_params(M, params)


def check_cost_dict(cost, M: int, xdim: int, udim: int) -> None:
    """The host-side refusals of dict(kind="custom", cost=, params=): no CustomCost, dimensions that are not the problem's, params that
    are not (M, pdim).  Any other cost passes (the built-in ones have checks of their own)."""
    check_custom_dict(cost, "cost", CustomCost, "cost", M, xdim, udim)
