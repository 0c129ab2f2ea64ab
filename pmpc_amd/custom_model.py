"""Custom dynamics models: x+ = F(x, u; p) written as a short piece of device code, compiled at run time for the GPU with forward-mode
automatic differentiation for the Jacobians (pmpc_amd/csrc/model_jit.hip, model_dual.h, model_kernels.h).

    bicycle = pmpc_amd.CustomModel('''
    template <class T>
    __device__ void step(const T *x, const T *u, const double *p, T *xn) {   // x[XD], u[UD], p[PD] -> xn[XD]
      const double L = p[0], dt = p[1];
      xn[0] = x[0] + dt * x[3] * cos(x[2]);
      xn[1] = x[1] + dt * x[3] * sin(x[2]);
      xn[2] = x[2] + dt * x[3] * tan(u[1]) / L;
      xn[3] = x[3] + dt * u[0];
    }''', xdim=4, udim=2, pdim=2)
    ctl = pmpc_amd.MPCController(builtin_model=bicycle, params=P, Q=Q, R=R, ...)

`T` is `double` for rollout and plan shift and a dual number for the linearisation; `+ - * /`, comparisons and
`sin cos tan exp log sqrt tanh atan atan2 pow(T, double) fabs fmin fmax` work on both.  The object enters everything a built-in
model name enters: `solve(..., device=..., builtin_model=)`, `MPCController(builtin_model=)`, and through `DeviceSolver.load_model`
the id-taking methods `linearize`, `rollout`, `shift_plan`, `scp_loop`.  Compiling needs no GPU.
"""
from __future__ import annotations

from typing import Optional

from .custom_jit import CustomCode

MAX_DIM = 16  # states, controls, parameters: the solver's own limits


class CustomModel(CustomCode):
    def __init__(self, step_source: str, xdim: int, udim: int, pdim: int, name: Optional[str] = None):
        self.step_source, self.name = str(step_source), name
        self.xdim, self.udim, self.pdim = int(xdim), int(udim), int(pdim)
        for what, d in (("xdim", self.xdim), ("udim", self.udim), ("pdim", self.pdim)):
            if not 1 <= d <= MAX_DIM:
                raise ValueError(f"CustomModel: {what} = {d} is outside 1 .. {MAX_DIM}")

    def __repr__(self):
        return f"CustomModel({self.name or 'unnamed'}, xdim={self.xdim}, udim={self.udim}, pdim={self.pdim})"

    def compile(self, arch: str = "gfx950") -> bytes:
        """The code object for `arch` (a target id; what follows a ':' is dropped), compiled once per object and architecture.
        A compile error is a ValueError that carries the compiler's log."""
        return self._compile("pmpc_model_compile", "custom models", self.step_source, (self.xdim, self.udim, self.pdim), arch)

    def check_problem(self, M: int, xdim: int, udim: int, params) -> None:
        """Refuse a problem whose Q / R dimensions or `params` (M, pdim) are not this model's (host-side: no device is touched)."""
        import numpy as np

        if (int(xdim), int(udim)) != (self.xdim, self.udim):
            raise ValueError(f"{self!r}: the problem has Q (.., {xdim}, {xdim}) and R (.., {udim}, {udim}), not the model's dimensions")
        n = params.numel() if hasattr(params, "numel") else np.size(params)
        if n != int(M) * self.pdim:
            raise ValueError(f"{self!r}: params must be (M, pdim) = ({M}, {self.pdim}), got {n} values")
